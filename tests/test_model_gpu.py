"""Model-level parity on the MI355X: the HIP path (gct_plus_amd.Model.*, through the C ABI)
against (1) the committed golden fixtures produced by the REAL reference and (2) the CPU
oracle on fresh seeded inputs.  Stated fp32 tolerances: logits/mu/log_var
atol 1e-4 rtol 1e-4; gradients rtol 1e-3 (+1e-5*max|g| atol); loss rtol 1e-5 (2e-5 here to
cover summation-order differences); argmax token ids bit-exact."""
import json
import logging
import os
from types import SimpleNamespace

import pytest
import torch

from gct_plus_amd import synthetic

pytestmark = pytest.mark.gpu
TYPES = ["vaetf", "pvaetf", "scavaetf", "pscavaetf"]
TINY = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
PAD = synthetic.PAD_ID


def build(mtype, dropout=0.0, full=False, seed=1, **over):
    from gct_plus_amd.Model import model_dict
    vs, vt = synthetic.vocab_sizes(mtype)
    kw = dict(N=6, d_model=512, dff=2048, h=8, latent_dim=128) if full else dict(TINY)
    kw.update(over)
    torch.manual_seed(seed)
    m = model_dict[mtype](vs, vt, dropout=dropout, nconds=synthetic.n_conds(mtype),
                          use_cond2dec=False, use_cond2lat=True, **kw)
    return m.cuda()


def set_eps(model, eps):
    (model.sampler if hasattr(model, "sampler") else model.encoder).eps_override = eps


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def run_fwd_loss(model, mtype, batch, beta):
    from gct_plus_amd.Model import forward_propagation
    from gct_plus_amd.Train.trainer1 import loss_function
    b = to_dev(batch)
    prop, mol, mu, lv, z = forward_propagation[mtype](model, b, PAD, False)
    ys = b["trg"][:, 1:].contiguous().view(-1)
    nc = synthetic.n_conds(mtype)
    ys_cond = b["dconds"].unsqueeze(2).contiguous().view(-1, nc, 1) if nc else None
    loss, rce, _, kld = loss_function(beta, prop, mol, ys_cond, ys, mu, lv, False, PAD)
    return prop, mol, mu, lv, z, loss, rce, kld


def grad_floor(grads):
    """Absolute floor for gradient comparisons: 2e-6 x the largest gradient entry of the whole
    model.  Needed for tensors whose gradient is analytically ZERO -- every k_linear.bias (a key
    bias shifts all scores of a softmax row equally) -- where reference and HIP both hold pure
    fp32 rounding noise (~1e-7) and a per-tensor relative tolerance is meaningless."""
    return 2e-6 * max(float(g.abs().max()) for g in grads if g is not None)


def assert_close(got, ref, atol, rtol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: max err {err.max():.3e}, ref max {ref.abs().max():.3e}, bad {int(bad.sum())}"


@pytest.mark.parametrize("mtype", TYPES)
def test_golden_forward_loss_grads(golden_dir, mtype):
    fx = torch.load(os.path.join(golden_dir, f"g2_{mtype}.pt"), weights_only=True)
    model = build(mtype).train()
    assert list(model.state_dict().keys()) == list(fx["init_sha256"].keys())
    set_eps(model, fx["eps"])
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, mtype, fx["batch"], fx["beta"])
    assert (prop is None) == fx["prop_is_none"]
    for got, key in ((mol, "logits"), (mu, "mu"), (lv, "log_var"), (z, "z")):
        assert_close(got, fx[key], 1e-4, 1e-4, key)
    assert torch.equal(mol.argmax(-1).cpu(), fx["logits"].argmax(-1))
    for got, key in ((loss, "loss"), (rce, "rce"), (kld, "kld")):
        assert abs(got.item() - fx[key]) <= 2e-5 * abs(fx[key]), (key, got.item(), fx[key])
    loss.backward()
    named = dict(model.named_parameters())
    assert list(named) == fx["param_order"]
    floor = grad_floor(fx["grads"].values())
    for name in fx["param_order"]:
        p = named[name]
        if name in fx["no_grad_params"]:
            assert p.grad is None, name
            continue
        e = fx["grads"][name]
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)
    assert model.grads_are_flat()          # kernels wrote straight into the flat buffer


@pytest.mark.parametrize("mtype", ["vaetf", "pscavaetf"])
def test_oracle_fresh_inputs(mtype):
    """HIP vs the CPU oracle on inputs no fixture covers (ragged lengths, B=6, S=24)."""
    from oracle import gct_oracle as O
    model = build(mtype, seed=3).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(6, max_len=24, model_type=mtype, seed=99)
    eps = torch.randn(6, 24 + nc, TINY["latent_dim"], generator=torch.Generator().manual_seed(4))
    set_eps(model, eps)
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, mtype, ds, 0.1)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, ds.get("econds"),
                                      ds.get("dconds"), eps=eps, train=True)
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    assert_close(mu, omu, 1e-4, 1e-4, "mu")
    assert_close(z, oz, 1e-4, 1e-4, "z")
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    ys_cond = ds["dconds"].unsqueeze(2).contiguous().view(-1, nc, 1) if nc else None
    oloss, _, _, _ = O.loss_function(0.1, None, omol, ys_cond, ys, omu, olv, False, PAD)
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            assert p.grad is None
            continue
        e = P[name].grad
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_full_size_config_vs_oracle():
    """BASELINE config dims (vaetf 6+6, d512, h8, dff2048, lat128), B=4, S=80."""
    from oracle import gct_oracle as O
    model = build("vaetf", full=True).train()
    cfg = O.make_cfg("vaetf", 28, 30, dropout=0.0, nconds=0, use_cond2lat=True)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(4, max_len=80, model_type="vaetf", seed=5)
    eps = torch.randn(4, 80, 128, generator=torch.Generator().manual_seed(6))
    set_eps(model, eps)
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, "vaetf", ds, 0.04)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, eps=eps, train=True)
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    assert_close(mu, omu, 1e-4, 1e-4, "mu")
    assert_close(lv, olv, 1e-4, 1e-4, "log_var")
    assert torch.equal(mol.argmax(-1).cpu(), omol.argmax(-1))
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    oloss, _, _, _ = O.loss_function(0.04, None, omol, None, ys, omu, olv, False, PAD)
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            continue
        e = P[name].grad
        assert_close(p.grad, e, 2e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_full_size_pscavaetf_large_batch_vs_oracle():
    """BASELINE dims, pscavaetf (3 conditions, scaffold prefix), B=96: 7 700+ token rows, so EVERY large GEMM of
    the step -- forward, dgrad and wgrad, N = 512 / 1024 / 1536 / 2048 -- runs on the bf16x6 kernels (tail-balanced
    where the tile count asks for it) and is checked against the CPU oracle at the fp32 tolerances."""
    from oracle import gct_oracle as O
    from gct_plus_amd import ops
    mtype, B = "pscavaetf", 96          # 96 x 83 and 96 x 81 token rows: multiples of 32, so wgrad qualifies too
    model = build(mtype, full=True).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=3, use_cond2lat=True)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(B, max_len=80, model_type=mtype, seed=11)
    eps = torch.randn(B, 83, 128, generator=torch.Generator().manual_seed(12))
    set_eps(model, eps)
    c0 = ops.gemm_launch_counts()
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, mtype, ds, 0.04)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, ds["econds"], ds["dconds"], eps=eps, train=True)
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    assert_close(mu, omu, 1e-4, 1e-4, "mu")
    assert_close(lv, olv, 1e-4, 1e-4, "log_var")
    assert torch.equal(mol.argmax(-1).cpu(), omol.argmax(-1))
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    oloss = O.loss_function(0.04, None, omol, ds["dconds"].unsqueeze(2), ys, omu, olv, False, PAD)[0]
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    c1 = ops.gemm_launch_counts()
    assert c1[1] - c0[1] >= 190, ("bf16x6 launches", c1[1] - c0[1])     # 67 fwd + 68 dgrad + 68 wgrad qualify
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            continue
        e = P[name].grad
        assert_close(p.grad, e, 2e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_full_size_batch_128_vs_oracle():
    """BASELINE dims, vaetf, B=128 (the reference scripts' batch size), MOSES-like lengths: the compacted decoder
    backward has ~5 000 live rows, a tile count at which the GELU-backward dgrad (reading the pre-activation through the
    quad map) is tail-balanced -- the combination that used to read out of bounds.  Loss and all gradients against the
    CPU oracle."""
    from oracle import gct_oracle as O
    mtype, B = "vaetf", 128
    model = build(mtype, full=True).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=0, use_cond2lat=True)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(B, max_len=80, model_type=mtype, seed=21)
    eps = torch.randn(B, 80, 128, generator=torch.Generator().manual_seed(22))
    set_eps(model, eps)
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, mtype, ds, 0.04)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, eps=eps, train=True)
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    oloss, _, _, _ = O.loss_function(0.04, None, omol, None, ys, omu, olv, False, PAD)
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            continue
        e = P[name].grad
        assert_close(p.grad, e, 2e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_full_size_batch_512_vs_oracle():
    """BASELINE configs[1] itself -- vaetf at the benchmarked per-GPU batch of 512, MOSES-like lengths: the routes a
    launch takes depend on its tile counts (tail balancing, quad compaction, visible-row K/V), so the shape bench.py
    times is checked as such: logits, loss and every gradient against the CPU oracle (~1 min of CPU;
    Train/trainer1.py:19-30 of the reference)."""
    from oracle import gct_oracle as O
    from gct_plus_amd import ops
    mtype, B = "vaetf", 512
    model = build(mtype, full=True).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=0, use_cond2lat=True)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(B, max_len=80, model_type=mtype, seed=0)
    eps = torch.randn(B, 80, 128, generator=torch.Generator().manual_seed(23))
    set_eps(model, eps)
    c0 = ops.gemm_launch_counts()[1]
    prop, mol, mu, lv, z, loss, rce, kld = run_fwd_loss(model, mtype, ds, 0.04)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, eps=eps, train=True)
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    assert_close(mu, omu, 1e-4, 1e-4, "mu")
    assert torch.equal(mol.argmax(-1).cpu(), omol.argmax(-1)) or \
        _only_ties_differ(mol.detach().cpu(), omol.detach()), "argmax ids differ away from fp32 ties"
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    oloss, _, _, _ = O.loss_function(0.04, None, omol, None, ys, omu, olv, False, PAD)
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    oloss.backward()
    if ops.gemm_get_mode() == ops.GEMM_BF16X6:
        assert ops.gemm_launch_counts()[1] - c0 >= 190      # the bf16x6 kernels really served the step
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            continue
        e = P[name].grad
        assert_close(p.grad, e, 2e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def _only_ties_differ(got, ref, gap=1e-4):
    """argmax ids may differ only where the reference's two best logits are closer than `gap` (both sides take the
    argmax of fp32 logits computed in different summation orders)."""
    ga, ra = got.argmax(-1), ref.argmax(-1)
    bad = ga != ra
    if not bool(bad.any()):
        return True
    top2 = ref[bad].topk(2, dim=-1).values
    return bool(((top2[:, 0] - top2[:, 1]) < gap).all())


def _args(mtype, d_model):
    nc = synthetic.n_conds(mtype)
    return SimpleNamespace(model_type=mtype, pad_id=PAD, use_cond2dec=False,
                           property_list=["logP", "tPSA", "QED"][:nc], lr_scheduler="WarmUpDefault",
                           lr_WarmUpSteps=8000, d_model=d_model, print_every=1000)


class _Loader(list):
    pass


@pytest.mark.parametrize("mtype", TYPES)
def test_five_step_history_vs_reference(golden_dir, mtype):
    """G3: run_epoch + FusedAdam reproduce the reference's 5-step history (eps drawn from the
    CPU generator exactly like the reference's randn_like)."""
    from gct_plus_amd.Train.trainer1 import run_epoch
    from gct_plus_amd.optim import FusedAdam
    g3 = json.load(open(os.path.join(golden_dir, "g3_history.json")))[mtype]
    model = build(mtype).train()
    (model.sampler if hasattr(model, "sampler") else model.encoder).eps_mode = "cpu"
    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, model=model)
    ds = synthetic.make_dataset(20, max_len=20, model_type=mtype, seed=11)
    loader = _Loader(to_dev(b) for b in synthetic.batches(ds, 4))
    torch.manual_seed(2024)
    hist, step = run_epoch(_args(mtype, 64), model, opt, loader, 0, 0.04, logging.getLogger("t"), True)
    assert step == 5
    for k in ("RCE", "KLD", "LOSS"):
        for a, b in zip(hist[k], g3[k]):
            assert abs(a - b) <= 1e-4 * abs(b), (k, hist[k], g3[k])
    for a, b in zip(hist["LR"], g3["LR"]):
        assert abs(a - b) <= 1e-12


def test_loss_curve_100_steps_full_size(golden_dir):
    """G4 (north-star criterion): config 1 -- vaetf 6+6/d512, B=64, S=80, dropout 0, seed 1 --
    100 optimisation steps stay within 1e-3 (relative) of the reference's CPU curve."""
    from gct_plus_amd.Train.trainer1 import run_epoch
    from gct_plus_amd.optim import FusedAdam
    path = os.path.join(golden_dir, "g4_curve_vaetf.json")
    if not os.path.exists(path):
        pytest.skip("g4 curve fixture not generated")
    g4 = json.load(open(path))
    model = build("vaetf", full=True).train()            # seed 1: same RNG stream as the reference
    model.sampler.eps_mode = "cpu"
    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, model=model)
    ds = synthetic.make_dataset(1000, max_len=80, model_type="vaetf", seed=0)
    loader = _Loader(to_dev(b) for b in synthetic.batches(ds, 64))
    hist = {"RCE": [], "KLD": [], "LOSS": [], "LR": []}
    step, args, log = 0, _args("vaetf", 512), logging.getLogger("t")
    while step < 100:
        need = min(len(loader), 100 - step)
        h, step = run_epoch(args, model, opt, _Loader(loader[:need]), step, 0.04, log, True)
        for k in hist:
            hist[k] += h[k]
    worst = max(abs(a - b) / abs(b) for a, b in zip(hist["LOSS"], g4["LOSS"]))
    assert worst <= 1e-3, f"max relative loss deviation over 100 steps {worst:.3e}"
    worst_rce = max(abs(a - b) / abs(b) for a, b in zip(hist["RCE"], g4["RCE"]))
    assert worst_rce <= 1e-3, worst_rce
    assert hist["LOSS"][-1] < hist["LOSS"][0]


def test_dropout_training_and_eval_modes():
    model = build("pvaetf", dropout=0.1, seed=2)
    ds = synthetic.make_dataset(8, max_len=20, model_type="pvaetf", seed=1)
    model.train()
    set_eps(model, torch.zeros(8, 23, 16))
    out1 = run_fwd_loss(model, "pvaetf", ds, 0.04)
    out2 = run_fwd_loss(model, "pvaetf", ds, 0.04)
    assert not torch.equal(out1[1], out2[1])                 # fresh masks every call
    out1[5].backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    model.eval()
    with torch.no_grad():
        e1 = run_fwd_loss(model, "pvaetf", ds, 0.04)
        e2 = run_fwd_loss(model, "pvaetf", ds, 0.04)
    assert torch.equal(e1[1], e2[1])                         # eval is deterministic (p = 0)


def test_dropout_gradient_matches_finite_difference_direction():
    """With dropout active the backward must use the forward's masks: check
    <grad, v> against a central difference of the loss along v under a FIXED seed."""
    from gct_plus_amd import engine
    model = build("vaetf", dropout=0.2, seed=4).train()
    ds = synthetic.make_dataset(4, max_len=20, model_type="vaetf", seed=2)
    set_eps(model, torch.randn(4, 20, 16, generator=torch.Generator().manual_seed(1)))

    def loss_at():
        torch.manual_seed(77)                                # same Philox seeds every call
        engine._SEED["base"] = None
        return run_fwd_loss(model, "vaetf", ds, 0.04)[5]

    loss = loss_at()
    loss.backward()
    p = model.decoder.layers[0].ff.linear_1.weight
    g = p.grad.clone()
    v = torch.randn_like(p)
    v /= v.norm()
    h = 1e-2
    with torch.no_grad():
        p.add_(h * v)
        lp = loss_at().item()
        p.add_(-2 * h * v)
        lm = loss_at().item()
        p.add_(h * v)
    fd = (lp - lm) / (2 * h)
    an = float((g * v).sum())
    assert abs(fd - an) <= 2e-2 * max(1.0, abs(an)), (fd, an)


def test_checkpoint_layout_roundtrip(tmp_path, golden_dir):
    from gct_plus_amd.Model import load_state
    from gct_plus_amd.Train.trainer1 import save_checkpoint
    from gct_plus_amd.optim import FusedAdam
    fx = torch.load(os.path.join(golden_dir, "g2_pscavaetf.pt"), weights_only=True)
    model = build("pscavaetf").train()
    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, model=model)
    set_eps(model, fx["eps"])
    run_fwd_loss(model, "pscavaetf", fx["batch"], 0.04)[5].backward()
    opt.step()
    args = SimpleNamespace(property_list=["logP", "tPSA", "QED"], N=2, d_model=64, d_ff=128, H=4,
                           latent_dim=16, dropout=0.0, use_cond2dec=False, use_cond2lat=True,
                           variational=True)
    path = str(tmp_path / "model_1.pt")
    save_checkpoint(args, model, opt, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"model_state_dict", "opt_state_dict", "model_params"}
    assert list(ck["model_state_dict"].keys()) == list(fx["init_sha256"].keys())
    assert ck["model_params"]["nconds"] == 3
    # stock torch Adam accepts the optimiser state (reference resume path train1.py:125-129)
    ref_opt = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()],
                               lr=1e-4, betas=(0.9, 0.98), eps=1e-9)
    ref_opt.load_state_dict(ck["opt_state_dict"])
    # 'module.'-prefixed checkpoints (saved from a DDP wrapper) load too
    pref = {"model_state_dict": {"module." + k: v for k, v in ck["model_state_dict"].items()}}
    torch.save(pref, path)
    m2 = load_state(build("pscavaetf", seed=9), path)
    for (k, a), (_, b) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k


@pytest.mark.parametrize("name,mtype", [("g6_ckpt_pvaetf.pt", "pvaetf"), ("g6_ckpt_pvaetf_module.pt", "pvaetf"),
                                        ("g6_ckpt_vaetf.pt", "vaetf")])
def test_reference_written_checkpoint_continues_on_hip(golden_dir, name, mtype):
    """G6: a checkpoint written by the REFERENCE's own save_checkpoint (model + stock
    torch.optim.Adam state after 3 of its run_epoch steps; bare and 'module.'-prefixed keys; vaetf: no Adam state
    for the 4 dead encoder.fc_* tensors) is loaded through load_state / FusedAdam.load_state_dict; model.encode and
    the next two training steps reproduce what the reference itself produced from that state."""
    from gct_plus_amd.Model import get_src_mask, load_checkpoint, load_state
    from gct_plus_amd.Train.trainer1 import run_epoch
    from gct_plus_amd.optim import FusedAdam
    path = os.path.join(golden_dir, name)
    exp = json.load(open(os.path.join(golden_dir, "g6_expect.json")))[mtype]
    nc = synthetic.n_conds(mtype)
    model = load_state(build(mtype, seed=9), path)
    opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, model=model)
    opt.load_state_dict(load_checkpoint(path)["opt_state_dict"])
    ds = synthetic.make_dataset(20, max_len=20, model_type=mtype, seed=11)
    loader = [to_dev(b) for b in synthetic.batches(ds, 4)]
    # encode path (Inference/sampling_tool.py:225-236): mu, log_var, z against the reference's values
    model.eval()
    b = loader[0]
    set_eps(model, torch.randn(4, 20 + nc, 16, generator=torch.Generator().manual_seed(exp["encode_eps_seed"])))
    with torch.no_grad():
        sm = get_src_mask(b["src"], PAD, b.get("econds"))
        z, mu, lv = model.encode(b["src"], sm, b["econds"]) if nc else model.encode(b["src"], sm)
    for got, key in ((z, "z"), (mu, "mu"), (lv, "log_var")):
        assert_close(got, torch.tensor(exp["encode"][key]), 1e-4, 1e-4, f"encode {key}")
    set_eps(model, None)
    model.train()
    (model.sampler if hasattr(model, "sampler") else model.encoder).eps_mode = "cpu"
    torch.manual_seed(77)
    hist, step = run_epoch(_args(mtype, 64), model, opt, _Loader(loader[3:5]), 3, 0.04, logging.getLogger("t"), True)
    assert step == exp["final_step"] == 5
    for k in ("RCE", "KLD", "LOSS"):
        for a, e in zip(hist[k], exp["continued"][k]):
            assert abs(a - e) <= 1e-4 * abs(e), (k, hist[k], exp["continued"][k])
    for a, e in zip(hist["LR"], exp["continued"]["LR"]):
        assert abs(a - e) <= 1e-12


def test_two_forwards_one_backward_accumulates(golden_dir):
    """ADVICE r1 (engine.GradSink): the model used twice inside ONE autograd graph -- (loss_a + loss_b).backward()
    -- must give g_a + g_b; both Function backwards run before AccumulateGrad, so the second one may not be handed
    the same flat-gradient slot.  Checked against the two gradients computed in separate passes and the oracle."""
    from oracle import gct_oracle as O
    mtype = "pscavaetf"
    fx = torch.load(os.path.join(golden_dir, f"g2_{mtype}.pt"), weights_only=True)
    ds = synthetic.make_dataset(4, max_len=20, model_type=mtype, seed=21)
    model = build(mtype).train()
    set_eps(model, fx["eps"])
    sep = {}
    for batch in (fx["batch"], ds):
        model.zero_grad(set_to_none=True)
        run_fwd_loss(model, mtype, batch, 0.04)[5].backward()
        for n, p in model.named_parameters():
            sep[n] = sep.get(n, 0) + p.grad.detach().clone()
    model.zero_grad(set_to_none=True)
    la = run_fwd_loss(model, mtype, fx["batch"], 0.04)[5]
    lb = run_fwd_loss(model, mtype, ds, 0.04)[5]
    (la + lb).backward()
    floor = grad_floor(list(sep.values()))
    for n, p in model.named_parameters():
        assert_close(p.grad, sep[n], 1e-6 * float(sep[n].abs().max()) + floor, 1e-5, f"joint vs separate {n}")
    # and against the oracle (CPU restatement of the reference) on the joint loss
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=3, use_cond2lat=True, **TINY)
    P = O.make_leaves(O.init_state(cfg, seed=1))
    tot = 0
    for batch in (fx["batch"], ds):
        sm, tm, trg_in = O.batch_masks(cfg, batch, PAD)
        _, mol, mu, lv, _ = O.forward(P, cfg, batch["src"], trg_in, sm, tm, batch["econds"], batch["dconds"],
                                      eps=fx["eps"], train=True)
        tot = tot + O.loss_function(0.04, None, mol, batch["dconds"].unsqueeze(2), batch["trg"][:, 1:].reshape(-1),
                                    mu, lv, False, PAD)[0]
    tot.backward()
    for n, p in model.named_parameters():
        e = P[n].grad
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, f"joint vs oracle {n}")
    # the usual single-use step afterwards still writes straight into the flat buffer
    model.zero_grad(set_to_none=True)
    run_fwd_loss(model, mtype, ds, 0.04)[5].backward()
    assert model.grads_are_flat()


@pytest.mark.parametrize("case", ["last_token_loss", "no_trg_mask", "left_padded", "right_padded_reference"])
def test_zero_gradient_rows_with_arbitrary_masks_vs_oracle(case):
    """VERDICT r1 2a / ADVICE (engine.py:340): the decoder backward reduces its weight gradients over the token tiles
    that hold a non-zero incoming gradient.  That is exact only while no live query attends to a dead row; the guard
    (ops.LiveRows, csrc/liverows.hip) checks it on the device from the gradient and the mask of THIS call.  B*T = 512
    rows (% 32 == 0) with >= 32 consecutive zero-gradient rows in every case; all gradients against the oracle.
      last_token_loss : causal mask, loss on the last position only -> live query sees 63 dead keys (guard must trip)
      no_trg_mask     : trg_mask=None, padded ys                   -> dead rows are visible keys    (guard must trip)
      left_padded     : tokens right-aligned, pad & causal mask    -> the first live row of a sample (target <sos>, its own
                        input is <pad>) sees NO key: masked_fill gives it uniform attention over ALL keys, dead ones
                        included, so they do receive dV                                            (guard must trip)
      right_padded_reference : the reference's own masks            -> shortcut taken"""
    from gct_plus_amd import ops
    from gct_plus_amd.Model import get_src_mask, get_trg_mask
    from gct_plus_amd.Train.trainer1 import loss_function
    from oracle import gct_oracle as O
    mtype, B, S = "pvaetf", 8, 63
    T = S + 1
    model = build(mtype, seed=3).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=3, use_cond2lat=True, **TINY)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    g = torch.Generator().manual_seed(17)
    ds = synthetic.make_dataset(B, max_len=S, model_type=mtype, seed=41)
    lens = torch.randint(8, 20, (B,), generator=g)                # short samples: > 40 padded positions each
    src = torch.full((B, S), PAD, dtype=torch.long)
    trg = torch.full((B, S + 2), PAD, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        toks = ds["src"][0, :n]
        if case == "left_padded":
            src[b, S - n:] = toks
            trg[b, S + 2 - (n + 2):] = torch.cat([torch.tensor([synthetic.SOS_ID]), toks + 2,
                                                  torch.tensor([synthetic.EOS_ID])])
        else:
            src[b, :n] = toks
            trg[b, :n + 2] = torch.cat([torch.tensor([synthetic.SOS_ID]), toks + 2, torch.tensor([synthetic.EOS_ID])])
    if case == "last_token_loss":
        src, trg = ds["src"].clone(), ds["trg"].clone()           # full-length rows; only the loss is sparse
        src[:, :] = ds["src"][0]
        trg[:, :] = ds["trg"][0]
    trg_in, ys = trg[:, :-1].contiguous(), trg[:, 1:].contiguous()
    if case == "last_token_loss":
        ys = ys.clone()
        ys[:, :-1] = PAD                                           # ignore_index everywhere but the last position
    econds = ds["econds"]
    src_mask = get_src_mask(src, PAD, econds)
    trg_mask = None if case == "no_trg_mask" else get_trg_mask(trg_in, PAD, False, econds)
    eps = torch.randn(B, S + 3, TINY["latent_dim"], generator=g)
    set_eps(model, eps)
    cu = lambda t: None if t is None else t.cuda()                 # noqa: E731
    prop, mol, mu, lv, z = model(cu(src), cu(trg_in), cu(src_mask), cu(trg_mask), cu(econds), cu(econds))
    yc = econds.unsqueeze(2).contiguous().view(-1, 3, 1).cuda()
    loss = loss_function(0.04, prop, mol, yc, ys.view(-1).cuda(), mu, lv, False, PAD)[0]
    _, omol, omu, olv, _ = O.forward(P, cfg, src, trg_in, src_mask, trg_mask, econds, econds, eps=eps, train=True)
    oloss = O.loss_function(0.04, None, omol, econds.unsqueeze(2), ys.view(-1), omu, olv, False, PAD)[0]
    assert_close(mol, omol, 1e-4, 1e-4, "logits")
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    # what the guard sees for this call's decoder gradient
    dmol = torch.autograd.grad(loss, mol, retain_graph=True)[0]
    lr = ops.LiveRows(dmol.reshape(B * T, -1).contiguous(), B, T, ops.to_mask_u8(cu(trg_mask)))
    h = lr.host()
    dead_run = 0
    run_len = 0
    for f in lr.live[:B * T].tolist():
        run_len = 0 if f else run_len + 1
        dead_run = max(dead_run, run_len)
    assert dead_run >= 32, dead_run
    assert h["n_live"] == int((ys != PAD).sum())
    if case in ("last_token_loss", "no_trg_mask", "left_padded"):
        assert h["violations"] > 0 and h["tiles"] == B * T // 32      # every tile listed: dense reduction
    else:
        assert h["violations"] == 0 and h["tiles"] < B * T // 32      # shortcut in force
    assert (h["nonprefix"] > 0) == (case in ("left_padded", "last_token_loss"))
    loss.backward()
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        e = P[name].grad
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, f"{case}: grad {name}")


@pytest.mark.parametrize("mtype,kw,B,S,p", [("pscavaetf", {}, 9, 70, 0.0), ("pvaetf", {}, 16, 77, 0.2),
                                            ("vaetf", dict(N=2, d_model=512, dff=2048, h=8, latent_dim=128), 48, 80, 0.1)])
def test_compacted_decoder_backward_matches_dense(mtype, kw, B, S, p, monkeypatch):
    """The decoder backward on quad-compacted live rows (engine.decoder_trunk_bwd, csrc/liverows.hip) and the
    cross-attention K / V path on the visible rows of the encoder memory only (engine.RowPlan, ops.KeyRows)
    against the dense paths on the same inputs, seeds and dropout masks: loss and every parameter gradient.  The dropout cases prove that
    the mask of a compact quad is regenerated from its ORIGINAL quad (GEMM epilogue, dropout backward, attention)."""
    from gct_plus_amd import engine
    ds = synthetic.make_dataset(B, S, mtype, seed=31)
    nc = synthetic.n_conds(mtype)
    eps = torch.randn(B, S + nc, kw.get("latent_dim", TINY["latent_dim"]), generator=torch.Generator().manual_seed(2))
    grads, took = {}, {}
    for mode in (True, False):
        monkeypatch.setattr(engine, "COMPACT_BWD", mode)
        monkeypatch.setattr(engine, "COMPACT_KV", mode)          # cross-attention over the visible memory rows only
        monkeypatch.setattr(engine, "COMPACT_ENC_KV", mode)      # encoder self-attention K | V over the visible rows only
        seen = []
        real = engine.ops.LiveRows.gather
        monkeypatch.setattr(engine.ops.LiveRows, "gather", lambda self, *a, **k: (seen.append(1), real(self, *a, **k))[1])
        torch.manual_seed(77)
        engine._SEED["base"] = None                      # same dropout seeds in both runs
        model = build(mtype, dropout=p, seed=5, **kw).train()
        set_eps(model, eps)
        loss = run_fwd_loss(model, mtype, ds, 0.04)[5]
        loss.backward()
        torch.cuda.synchronize()
        grads[mode] = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
        grads[mode]["__loss__"] = loss.detach().reshape(1).clone()
        took[mode] = len(seen)
        monkeypatch.setattr(engine.ops.LiveRows, "gather", real)
    assert took[True] > 0 and took[False] == 0           # the compact path really ran (and only when enabled)
    floor = grad_floor(list(grads[False].values()))
    for n, e in grads[False].items():
        assert_close(grads[True][n], e, 2e-6 * float(e.abs().max()) + floor, 2e-5, f"compact vs dense: {n}")


def _fwd_loss_skip(model, mtype, batch, beta, skip):
    from gct_plus_amd.Model import forward_propagation
    from gct_plus_amd.Train.trainer1 import loss_function
    b = to_dev(batch)
    prop, mol, mu, lv, z = forward_propagation[mtype](model, b, PAD, False, skip_ignored=skip)
    ys = b["trg"][:, 1:].contiguous().view(-1)
    nc = synthetic.n_conds(mtype)
    ys_cond = b["dconds"].unsqueeze(2).contiguous().view(-1, nc, 1) if nc else None
    loss = loss_function(beta, prop, mol, ys_cond, ys, mu, lv, False, PAD)[0]
    return mol, loss


@pytest.mark.parametrize("mtype,kw,B,S,p", [("pscavaetf", {}, 9, 70, 0.0), ("pvaetf", {}, 16, 77, 0.2),
                                            ("scavaetf", {}, 12, 60, 0.1),
                                            ("vaetf", dict(N=2, d_model=512, dff=2048, h=8, latent_dim=128), 48, 80, 0.1)])
def test_decoder_forward_over_loss_rows_matches_dense(mtype, kw, B, S, p, monkeypatch):
    """forward_propagation(..., skip_ignored=True) -- the trainer's mode: the decoder forward AND backward run on the
    quad-compacted rows whose logits reach the ignore_index loss (engine.RowPlan.live) -- against
    the dense model on the same inputs, seeds and dropout masks: the loss, every parameter gradient, the logits of the
    rows the loss reads; the skipped rows come back as zeros (the vocabulary head runs on the compact rows too).  The dropout cases prove that
    every dropout site of the compact forward (GEMM epilogues, attention) draws the bits of the ORIGINAL coordinates."""
    from gct_plus_amd import engine
    ds = synthetic.make_dataset(B, S, mtype, seed=31)
    nc = synthetic.n_conds(mtype)
    eps = torch.randn(B, S + nc, kw.get("latent_dim", TINY["latent_dim"]), generator=torch.Generator().manual_seed(2))
    res, took = {}, {}
    for name in ("COMPACT_FWD", "COMPACT_BWD", "COMPACT_KV", "COMPACT_ENC_KV"):
        monkeypatch.setattr(engine, name, True)
    for skip in (True, False):
        seen = []
        real = engine.ops.LiveRows.scatter
        monkeypatch.setattr(engine.ops.LiveRows, "scatter", lambda self, *a, **k: (seen.append(self.fwd), real(self, *a, **k))[1])
        torch.manual_seed(77)
        engine._SEED["base"] = None                      # same dropout seeds in both runs
        model = build(mtype, dropout=p, seed=5, **kw).train()
        set_eps(model, eps)
        mol, loss = _fwd_loss_skip(model, mtype, ds, 0.04, skip)
        loss.backward()
        torch.cuda.synchronize()
        res[skip] = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
        res[skip]["__loss__"] = loss.detach().reshape(1).clone()
        res[skip]["__logits__"] = mol.detach().clone()
        res[skip]["__bias__"] = model.out.bias.detach().clone()
        took[skip] = [f for f in seen if f]
        monkeypatch.setattr(engine.ops.LiveRows, "scatter", real)
    assert len(took[True]) >= 2 and not took[False]      # forward and backward both ran on the forward's compact rows
    keep = (ds["trg"][:, 1:] != PAD).cuda()
    lt, lf = res[True].pop("__logits__"), res[False].pop("__logits__")
    assert_close(lt[keep], lf[keep], 1e-5, 1e-5, "logits of the rows the loss reads")
    bias = res[True].pop("__bias__")
    res[False].pop("__bias__")
    # skipped rows: zero -- except the (at most 3 + 3 per sample) padded rows that share an aligned group of four
    # rows with a live one: those travel with their quad and hold finite, meaningless values
    flat_keep = keep.reshape(-1)
    quads = torch.nn.functional.pad(flat_keep, (0, (-flat_keep.numel()) % 4)).view(-1, 4).any(1)
    in_live_quad = quads.repeat_interleave(4)[:flat_keep.numel()].view_as(keep)
    assert float(lt[~in_live_quad].abs().max()) == 0.0 and bias is not None
    assert torch.isfinite(lt).all()
    floor = grad_floor(list(res[False].values()))
    for n, e in res[False].items():
        assert_close(res[True][n], e, 2e-6 * float(e.abs().max()) + floor, 2e-5, f"loss-row forward vs dense: {n}")


def test_full_size_batch_512_skip_ignored_vs_oracle():
    """BASELINE configs[1] in the TRAINER's mode (skip_ignored=True: what bench.py times): loss and every gradient
    against the CPU oracle, logits on the rows the loss reads."""
    from oracle import gct_oracle as O
    mtype, B = "vaetf", 512
    model = build(mtype, full=True).train()
    vs, vt = synthetic.vocab_sizes(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=0, use_cond2lat=True)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ds = synthetic.make_dataset(B, max_len=80, model_type=mtype, seed=0)
    eps = torch.randn(B, 80, 128, generator=torch.Generator().manual_seed(23))
    set_eps(model, eps)
    mol, loss = _fwd_loss_skip(model, mtype, ds, 0.04, True)
    sm, tm, trg_in = O.batch_masks(cfg, ds, PAD)
    _, omol, omu, olv, oz = O.forward(P, cfg, ds["src"], trg_in, sm, tm, eps=eps, train=True)
    keep = ds["trg"][:, 1:] != PAD
    assert_close(mol.detach().cpu()[keep], omol.detach()[keep], 1e-4, 1e-4, "logits (loss rows)")
    ys = ds["trg"][:, 1:].contiguous().view(-1)
    oloss, _, _, _ = O.loss_function(0.04, None, omol, None, ys, omu, olv, False, PAD)
    assert abs(loss.item() - oloss.item()) <= 2e-5 * abs(oloss.item())
    loss.backward()
    oloss.backward()
    floor = grad_floor(v.grad for v in P.values())
    for name, p in model.named_parameters():
        if P[name].grad is None:
            continue
        e = P[name].grad
        assert_close(p.grad, e, 2e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_gradient_on_a_skipped_row_is_reported(monkeypatch):
    """A forward that skipped decoder rows cannot honour a gradient on them: the backward counts such rows on the device
    and the next read-back (the next forward's row maps) raises instead of training on a silently wrong gradient."""
    from gct_plus_amd import _lib, engine, ops
    monkeypatch.setattr(engine, "COMPACT_FWD", True)
    mtype = "vaetf"
    model = build(mtype).train()
    ds = synthetic.make_dataset(16, 60, mtype, seed=3)     # large enough for the compact forward to be taken
    ops.skipped_row_gradients().zero_()
    mol, _ = _fwd_loss_skip(model, mtype, ds, 0.04, True)
    mol.sum().backward()                                  # a loss that reads EVERY row, unlike the ignore_index CE
    # the optimizer step that follows must NOT apply that gradient: FusedAdam's launch is guarded by the device counter
    from gct_plus_amd.optim import FusedAdam
    opt = FusedAdam(model.parameters(), lr=1e-2, betas=(0.9, 0.98), eps=1e-9, model=model)
    before = model.flat_params().clone()
    opt.step()
    assert torch.equal(model.flat_params(), before), "a gradient on skipped rows was applied"
    with pytest.raises(_lib.GctError, match="skipped"):
        ops.assert_no_skipped_row_gradients()             # what run_epoch calls at the end of an epoch
    mol, _ = _fwd_loss_skip(model, mtype, ds, 0.04, True)
    mol.sum().backward()
    with pytest.raises(_lib.GctError, match="skipped"):
        _fwd_loss_skip(model, mtype, ds, 0.04, True)
    assert int(ops.skipped_row_gradients().item()) == 0   # reported once, then cleared
    mol, loss = _fwd_loss_skip(model, mtype, ds, 0.04, True)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()                                            # counter is zero: the guarded step updates as usual
    assert not torch.equal(model.flat_params(), before)
    _fwd_loss_skip(model, mtype, ds, 0.04, True)          # the reference's loss: nothing to report


def test_greedy_decode_token_ids_bit_exact(golden_dir):
    """G5: argmax-decoded ids from model.decode equal the reference's."""
    from gct_plus_amd.Model import get_trg_mask
    g5 = torch.load(os.path.join(golden_dir, "g5_decode.pt"), weights_only=True)
    for mtype, fx in g5.items():
        model = build(mtype).eval()
        z = fx["z"].cuda()
        dconds = fx["dconds"].cuda() if fx["dconds"] is not None else None
        n, L = z.shape[0], z.shape[1]
        src_mask = torch.ones(n, 1, L, dtype=torch.bool, device="cuda")
        ys = torch.full((n, 1), synthetic.SOS_ID, dtype=torch.long, device="cuda")
        with torch.no_grad():
            for _ in range(15):
                trg_mask = get_trg_mask(ys, PAD, False, dconds)
                logits = model.decode(ys, z, src_mask, trg_mask, dconds)
                ys = torch.cat([ys, logits[:, -1].argmax(-1, keepdim=True)], dim=1)
        assert torch.equal(ys.cpu(), fx["ys"]), mtype
        assert_close(logits[:, -1], fx["last_logits"], 1e-4, 1e-4, "last logits")


def test_get_attn_and_submodules():
    from gct_plus_amd.Model import model_dict
    torch.manual_seed(0)
    m = model_dict["vaetf"](28, 30, dropout=0.0, nconds=0, use_cond2lat=True, get_attn=True, **TINY).cuda().eval()
    ds = to_dev(synthetic.make_dataset(3, max_len=20, model_type="vaetf", seed=3))
    from gct_plus_amd.Model import get_src_mask, get_trg_mask
    trg_in = ds["trg"][:, :-1]
    out = m(ds["src"], trg_in, get_src_mask(ds["src"], PAD), get_trg_mask(trg_in, PAD, False))
    assert len(out) == 8
    for plist in out[5:]:
        assert len(plist) == 2
        for pr in plist:
            assert torch.allclose(pr.sum(-1), torch.ones_like(pr.sum(-1)), atol=1e-5)
    # standalone sub-modules (Norm, FeedForward, MultiHeadAttention, layers) run on the kernels
    x = torch.randn(3, 20, 64, device="cuda", requires_grad=True)
    layer = m.encoder.layers[0]
    y = layer.ff(layer.norm_2(x))
    y.sum().backward()
    ref = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(
        layer.norm_2(x.detach()), layer.ff.linear_1.weight, layer.ff.linear_1.bias)),
        layer.ff.linear_2.weight, layer.ff.linear_2.bias)
    assert torch.allclose(y, ref, atol=1e-4)
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_side_stream_wgrad_gives_identical_gradients(golden_dir, monkeypatch):
    """GCT_SIDE_STREAM=1 (weight-gradient GEMMs on a second stream) must not change a single bit."""
    from gct_plus_amd import ops
    fx = torch.load(os.path.join(golden_dir, "g2_pscavaetf.pt"), weights_only=True)
    grads = []
    for side in (False, True):
        monkeypatch.setattr(ops, "SIDE_ENABLED", side)
        model = build("pscavaetf").train()
        set_eps(model, fx["eps"])
        for _ in range(3):                                   # several backward passes, buffers recycled
            for p in model.parameters():
                p.grad = None
            run_fwd_loss(model, "pscavaetf", fx["batch"], fx["beta"])[5].backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


@pytest.mark.parametrize("mtype,full,batch", [("pscavaetf", False, 6), ("vaetf", True, 48), ("pvaetf", True, 24)])
def test_deferred_slab_reductions_give_identical_gradients(mtype, full, batch, monkeypatch):
    """The slab reductions of a layer's backward pass run as one launch at the end of the layer
    (ops.deferred_reductions): same lanes and summation order per destination, so not a single bit may change against
    the launch-per-reduction path -- with dropout on (the masks depend on the seed alone), over several passes (the
    arena is sized by the first layer, recycled by the later ones) and with a batch change in between (regrowth)."""
    from gct_plus_amd import ops
    lib = ops._L()
    grads = []
    for defer in (False, True):
        monkeypatch.setattr(ops, "DEFER_REDUCTIONS", defer)
        model = build(mtype, dropout=0.1, full=full).train()
        for it, n in enumerate((batch, batch, 2 * batch)):
            ds = synthetic.make_dataset(n, max_len=40, model_type=mtype, seed=5 + it)
            for p in model.parameters():
                p.grad = None
            torch.manual_seed(100 + it)
            run_fwd_loss(model, mtype, ds, 0.3)[5].backward()
            assert lib.gct_reduce_defer_pending() == 0
        torch.cuda.synchronize()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
    assert not ops._DEFER_TL.d["on"]


@pytest.mark.parametrize("mtype", ["vaetf", "pscavaetf"])
def test_announced_batch_gives_the_same_step(mtype, monkeypatch):
    """forward_propagation1.prefetch queues a batch's masks and row maps ahead of the forward that uses them (the
    trainer: between the previous step's forward and its backward).  Same logits, loss and gradients, bit for bit, as the
    un-announced call; an announcement for ANOTHER batch, for a batch modified since, or for a batch dict whose tensors
    are views of the announced ones (same address, shape and version) is dropped: that forward plans its own rows."""
    from gct_plus_amd import engine
    from gct_plus_amd.Model import forward_propagation
    from gct_plus_amd.Model.forward_propagation1 import prefetch
    from gct_plus_amd.Train.trainer1 import loss_function
    model = build(mtype, dropout=0.0).train()
    nc = synthetic.n_conds(mtype)
    b1 = to_dev(synthetic.make_dataset(9, max_len=24, model_type=mtype, seed=11))
    b2 = to_dev(synthetic.make_dataset(9, max_len=24, model_type=mtype, seed=12))
    plans = []
    real = engine.plan_rows
    monkeypatch.setattr(engine, "plan_rows", lambda caller, *a, **k: (plans.append(caller), real(caller, *a, **k))[1])

    def step(batch):
        for p in model.parameters():
            p.grad = None
        n0 = len(plans)
        prop, mol, mu, lv, _ = forward_propagation[mtype](model, batch, PAD, False, skip_ignored=True)
        ys = batch["trg"][:, 1:].contiguous().view(-1)
        ys_cond = batch["dconds"].unsqueeze(2).contiguous().view(-1, nc, 1) if nc else None
        loss = loss_function(0.3, prop, mol, ys_cond, ys, mu, lv, False, PAD)[0]
        loss.backward()
        torch.cuda.synchronize()
        step.planned = plans[n0:].count(engine.MODEL)           # row plans the forward launched itself
        return mol.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()
                                                              if p.grad is not None}

    mu = forward_propagation[mtype](model, b1, PAD, False, skip_ignored=True)[2]
    set_eps(model, torch.randn(mu.shape, generator=torch.Generator().manual_seed(3)).cuda())   # same noise every call
    ref = step(b1)
    assert step.planned == 1
    prefetch(mtype, model, b1, PAD, False, skip_ignored=True)
    got = step(b1)                                             # announced: uses the queued maps
    assert step.planned == 0
    assert step(b1) and step.planned == 1                      # an announcement is used once
    prefetch(mtype, model, b2, PAD, False, skip_ignored=True)
    other = step(b1)                                           # announced another batch: dropped, built as usual
    assert step.planned == 1
    prefetch(mtype, model, b1, PAD, False, skip_ignored=True)
    views = {k: v.view(v.shape) for k, v in b1.items()}       # same address, shape and version: not the same batch
    assert all(views[k].data_ptr() == b1[k].data_ptr() and views[k]._version == b1[k]._version for k in b1)
    viewed = step(views)
    assert step.planned == 1
    prefetch(mtype, model, b1, PAD, False, skip_ignored=True)
    b1["trg"][0, 3] = b1["trg"][0, 3]                          # an in-place write bumps the version: announcement stale
    stale = step(b1)
    assert step.planned == 1
    live = (b1["trg"][:, 1:] != PAD)                           # (skipped rows hold no meaningful logits)
    for out in (got, other, viewed, stale):
        assert torch.equal(out[0][live], ref[0][live]) and torch.equal(out[1], ref[1])
        assert out[2].keys() == ref[2].keys()
        for k in ref[2]:
            assert torch.equal(out[2][k], ref[2][k]), k


def test_cond2dec_path_vs_reference(golden_dir):
    """HIP path with -use_cond2dec against the reference fixture: decoder cond tokens, [B,T+3,T+3]
    block mask, prop_fc head (N=1 GEMM) and the MSE term."""
    from gct_plus_amd.Model import forward_propagation, model_dict
    from gct_plus_amd.Train.trainer1 import loss_function
    fx = torch.load(os.path.join(golden_dir, "g2_pvaetf_cond2dec.pt"), weights_only=True)
    torch.manual_seed(1)
    model = model_dict["pvaetf"](28, 30, dropout=0.0, nconds=3, use_cond2dec=True, use_cond2lat=False,
                                 **TINY).cuda().train()
    assert list(model.state_dict().keys()) == list(fx["init_sha256"].keys())
    set_eps(model, fx["eps"])
    b = to_dev(fx["batch"])
    prop, mol, mu, lv, z = forward_propagation["pvaetf"](model, b, PAD, True)
    assert_close(prop, fx["prop"], 1e-4, 1e-4, "prop")
    assert_close(mol, fx["logits"], 1e-4, 1e-4, "logits")
    ys = b["trg"][:, 1:].contiguous().view(-1)
    ys_cond = b["dconds"].unsqueeze(2).contiguous().view(-1, 3, 1)
    loss, rce, rce_prop, kld = loss_function(fx["beta"], prop, mol, ys_cond, ys, mu, lv, True, PAD)
    for got, key in ((loss, "loss"), (rce, "rce"), (rce_prop, "rce_prop"), (kld, "kld")):
        assert abs(float(got) - fx[key]) <= 2e-5 * abs(fx[key]) + 1e-6, (key, float(got), fx[key])
    loss.backward()
    floor = grad_floor(fx["grads"].values())
    for name, p in model.named_parameters():
        if name not in fx["grads"]:
            assert p.grad is None, name
            continue
        e = fx["grads"][name]
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, "grad " + name)


def test_weight_planes_follow_the_weights():
    """bf16x6 mode keeps bf16 pieces of the flat parameter buffer.  They are refreshed on every entry into the
    model (forward / encode / decode / a trunk called directly), dropped by the fused Adam, and two GEMM modes
    give the same loss and gradients after the weights were changed behind the model's back."""
    from gct_plus_amd import ops
    from gct_plus_amd.Model import forward_propagation
    from gct_plus_amd.Train.trainer1 import loss_function
    from gct_plus_amd.optim import FusedAdam
    m = build("vaetf", dropout=0.0).train()
    ds = synthetic.make_dataset(8, 20, "vaetf", seed=3)
    b = to_dev(ds)
    set_eps(m, torch.randn(8, 20, TINY["latent_dim"], generator=torch.Generator().manual_seed(0)))
    w = m.decoder.layers[0].ff.linear_1.weight
    assert ops.gemm_get_mode() == ops.GEMM_BF16X6

    def step_loss():
        for p in m.parameters():
            p.grad = None
        prop, mol, mu, lv, _ = forward_propagation["vaetf"](m, b, PAD, False)
        ys = b["trg"][:, 1:].contiguous().view(-1)
        loss = loss_function(0.1, prop, mol, None, ys, mu, lv, False, PAD)[0]
        loss.backward()
        return float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    l0, g0 = step_loss()
    assert ops._plane_ptr([w])[0] is not None                 # registered by the forward
    opt = FusedAdam(m.parameters(), lr=1e-3, model=m)
    opt.step()
    assert opt._flat is not None and ops._plane_ptr([w])[0] is None    # the fused Adam invalidated them
    with torch.no_grad():
        for p in m.parameters():                              # rewrite the weights behind everybody's back
            p.mul_(1.03)
    m.encoder(b["src"], (b["src"] != PAD).unsqueeze(-2), None)     # a trunk called directly refreshes too
    assert ops._plane_ptr([w])[0] is not None
    l1, g1 = step_loss()
    ops.gemm_set_mode(ops.GEMM_F32)
    try:
        l2, g2 = step_loss()
    finally:
        ops.gemm_set_mode(ops.GEMM_BF16X6)
    assert abs(l1 - l0) > 1e-3 * abs(l0)                       # the new weights were used ...
    assert abs(l1 - l2) <= 2e-5 * abs(l2)                      # ... and both arithmetic modes agree on them
    gmax = max(float(v.abs().max()) for v in g2.values())
    for n in g2:
        tol = 1e-5 * float(g2[n].abs().max()) + 2e-6 * gmax
        assert torch.allclose(g1[n], g2[n], atol=tol, rtol=1e-3), n
