"""Differentiable log-likelihoods on the device: gct_seq_logp_bwd against the rule (decode.seq_logp_grad_reference) in
fp64 and, bit for bit, against gct_ce_bwd; engine.SeqLogpFn under autograd; decode.sequence_logp against score_tokens
(values) and the CPU oracle's autograd (gradients); Train/finetune.reinforce_step against the same steps on the oracle;
and the samplers' return_rows / logp.

Tolerances.  Kernel: gct_ce_bwd's own (tests/test_loss_optim_edges_gpu.py: atol 1e-6, rtol 1e-5 for a weight of order
1) with the absolute part scaled by the largest weight, because the arithmetic is the same.  Model gradients: the
project's (tests/test_model_gpu.py): rtol 1e-3 + 1e-5 max|g| per tensor + grad_floor.  Objective per update step: the
loss-curve tolerance, 1e-3 relative.  Log-probabilities of a sampling call against a second forward: close_sums of
tests/test_score_gpu.py."""
import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd._lib import GctError
from gct_plus_amd.decode import (reference_style_decode, score_reference, score_tokens, seq_logp_grad_reference,
                                 sequence_logp)
from tests.test_loss_optim_edges_gpu import ce_bwd
from tests.test_mixed_scaffold_decode_gpu import EOS, PAD, SOS, TINY, build, upto_eos
from tests.test_model_gpu import assert_close, grad_floor
from tests.test_score_gpu import close_sums, cu, kernel_case, target_rows
from tests.test_seq_logp_grad_host import (UPDATE_LR, UPDATE_STEPS, objective, oracle_run, update_case, update_vocabs)
from tests.test_stream_decode_gpu import make_sampler

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def kernel_ratio(got, ref, gmax, what):
    """max |got - ref| / (1e-6 max|g| + 1e-5 |ref|); printed, asserted <= 1."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (1e-6 * gmax + 1e-5 * ref.abs()))   # (all weights 0: 0 / 0)
    r = float(ratio.max()) if got.numel() else 0.0
    print(f"{what}: worst error / tolerance {r:.4f}")
    assert r <= 1.0, what
    return r


# -------------------------------------------------------------------------------------------- 1. gct_seq_logp_bwd
SHAPES = [(1, 2, 2), (3, 8, 30), (5, 200, 31), (2, 9, 1024), (67, 5, 30), (300, 60, 30)]   # the last: 17 700 rows, past
                                                                                           # the 4096 x 4 of one grid


def weights(n, W, seed):
    """g_logp [n], g_token [n, W] of mixed sign.  Zeros: g_logp of row 1, a quarter of g_token; and in row 0 the two
    cancel exactly at column 2 (g_logp[0] = 1.5, g_token[0, 2] = -1.5: a scored row whose weight is 0)."""
    g = torch.Generator().manual_seed(seed)
    g_logp = torch.randn(n, generator=g)
    g_token = torch.randn(n, W, generator=g)
    g_token[torch.rand(n, W, generator=g) < 0.25] = 0
    g_logp[0] = 1.5
    if n > 1:
        g_logp[1] = 0
    if W > 2:
        g_token[0, 2] = -1.5
    return g_logp, g_token


@pytest.mark.parametrize("variant", ["plain", "no_lens", "ld", "shift"])
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_logp_bwd_against_the_rule(ops, n, W, V, variant):
    ys, lens, x = kernel_case(n, W, V, seed=n * 1000 + W)                         # ties and a -1e4 logit in row 0
    if V > 2:
        x[0, 0, 1] = -float("inf")                                                # beside the tie of row 0's first row
    if variant == "no_lens":
        lens = None
    t0 = torch.ones(n, dtype=torch.long) if lens is None else lens
    scored = (torch.arange(1, W)[None, :] >= t0[:, None]) & (ys[:, 1:] != PAD)
    shift = 3 if variant == "shift" else 0
    ld = V + 3 if variant == "ld" else V
    R = W - 1 + shift
    g_logp, g_token = weights(n, W, seed=W)
    worst = 0.0
    for which in ("logp", "token", "both"):
        gl, gt = (g_logp if which != "token" else None), (g_token if which != "logp" else None)
        g = (0 if gl is None else gl[:, None]) + (0 if gt is None else gt[:, 1:]) + torch.zeros(n, W - 1)
        live = scored & (g != 0)
        ref = seq_logp_grad_reference(x.double(), ys, lens, PAD, g_logp=None if gl is None else gl.double(),
                                      g_token=None if gt is None else gt.double())
        # NaN wherever the kernel has no business reading: behind V, the condition rows in front of a shifted sequence,
        # the logits rows that are not scored and those whose weight is 0; dlogits starts as NaN everywhere
        big = torch.full((n, R, ld), NAN)
        xs = x.clone()
        xs[~live] = NAN
        big[:, shift:, :V] = xs
        dev = big.cuda().view(n * R, ld)[:, :V]
        args = (dev, ys.cuda(), None if lens is None else lens.int().cuda(), PAD)
        outs = []
        for _ in range(2):
            buf = torch.full((n * R, ld), NAN, device="cuda")
            ops.seq_logp_bwd(*args, row_shift=shift, rows_per_seq=R, g_logp=cu(gl), g_token=cu(gt), out=buf[:, :V])
            outs.append(buf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:, :V], outs[1][:, :V])                        # two runs: the same bits
        assert bool(torch.isnan(outs[0][:, V:]).all())                            # nothing written behind V
        got = outs[0][:, :V].cpu().view(n, R, V)
        assert bool(torch.isfinite(got).all()), f"{which}: dlogits not finite (a row never written, or a poisoned one read)"
        assert not got[:, :shift].any() and not got[:, shift:][~live].any()       # exact zeros
        gmax = float(g.abs().max())
        worst = max(worst, kernel_ratio(got[:, shift:], ref, gmax, f"seq_logp_bwd {n, W, V} {variant} {which}"))
        if which == "both" and W > 2 and lens is None:
            assert bool(scored[0, 1]) and not bool(live[0, 1])                    # the cancelling weights were in play
        if V > 2 and bool(live[0, 0]):
            assert float(got[0, shift, 1]) == 0.0                                 # the -inf logit
        if W > 3 and bool(live[0, 2]):
            assert float(got[0, shift + 2, (int(ys[0, 3]) + 1) % V]) == 0.0       # the -1e4 logit
            assert float(ref[0, 2, (int(ys[0, 3]) + 1) % V]) == 0.0
    print(f"seq_logp_bwd {n, W, V} {variant}: worst error / tolerance {worst:.4f}")


def test_seq_logp_bwd_edge_values(ops):
    """One row each: a -1e4 logit, a -inf logit (gradient exactly 0 there), and a tie at the maximum (both maxima get the
    same probability; the target's entry carries the one-hot term)."""
    V = 30
    ys = torch.tensor([[SOS, 7, 9, 11]])
    x = torch.randn(1, 3, V, generator=torch.Generator().manual_seed(2)) * 3
    x[0, 0, 5] = -1e4
    x[0, 1, 5] = -float("inf")
    x[0, 2, 11] = x[0, 2, 20] = 14.0
    gl = torch.tensor([-2.5])
    got = ops.seq_logp_bwd(x.cuda().view(3, V), ys.cuda(), None, PAD, g_logp=gl.cuda()).cpu()
    ref = seq_logp_grad_reference(x.double(), ys, None, PAD, g_logp=gl.double())[0]
    assert float(got[0, 5]) == 0.0 and float(got[1, 5]) == 0.0 and bool(torch.isfinite(got).all())
    kernel_ratio(got, ref, 2.5, "edge values")
    p = torch.softmax(x[0, 2].double(), -1)
    assert abs(float(got[2, 20]) - 2.5 * float(p[20])) <= 1e-5 and abs(float(got[2, 11]) - 2.5 * (float(p[11]) - 1)) <= 1e-5


# ------------------------------------------------------------------------------------------ 2. the bits of gct_ce_bwd
@pytest.mark.parametrize("n,W,V", [(7, 9, 30), (3, 5, 130)])
def test_seq_logp_bwd_is_ce_bwd_bit_for_bit(ops, n, W, V):
    g = torch.Generator().manual_seed(V)
    ys = torch.randint(0, V, (n, W), generator=g)
    ys[ys == PAD] = 0
    ys[torch.rand(n, W, generator=g) < 0.25] = PAD                                # pad targets, inside the rows too
    x = (torch.randn(n, W - 1, V, generator=g) * 4).cuda().view(n * (W - 1), V)
    gval = 1.7
    want = ce_bwd(ops, x, ys[:, 1:].contiguous().view(-1).cuda(), torch.tensor(gval, device="cuda"), PAD)
    got = ops.seq_logp_bwd(x, ys.cuda(), None, PAD, g_logp=torch.full((n,), -gval, device="cuda"))
    torch.cuda.synchronize()
    assert bool((ys[:, 1:] == PAD).any()) and bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------ 3. refusals
def test_seq_logp_bwd_refuses_before_a_launch(ops):
    one = torch.ones(1, device="cuda")
    ys = torch.zeros(1, 257, dtype=torch.long, device="cuda")
    with pytest.raises(GctError, match="257"):
        ops.seq_logp_bwd(torch.zeros(256, 30, device="cuda"), ys, None, PAD, g_logp=one)
    with pytest.raises(GctError, match="null"):
        ops.seq_logp_bwd(None, ys[:, :9], None, PAD, g_logp=one, V=30)
    with pytest.raises(GctError, match="both gradients"):
        ops.seq_logp_bwd(torch.zeros(8, 30, device="cuda"), ys[:, :9], None, PAD)
    with pytest.raises(GctError, match="do not hold"):
        ops.seq_logp_bwd(torch.zeros(8, 30, device="cuda"), ys[:, :9], None, PAD, rows_per_seq=7, g_logp=one)
    torch.cuda.synchronize()


def test_seq_logp_bwd_of_no_sequences_writes_nothing(ops):
    x, out = torch.zeros(8, 30, device="cuda"), torch.full((8, 30), NAN, device="cuda")
    ys, one = torch.zeros(1, 9, dtype=torch.long, device="cuda"), torch.ones(1, device="cuda")
    rc = ops._L().gct_seq_logp_bwd(x.data_ptr(), 30, 30, 8, 0, ys.data_ptr(), 9, None, PAD, 0, 9, one.data_ptr(), None, 0,
                                   out.data_ptr(), 30, ops._st())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(out).all())
    assert ops.seq_logp_bwd(x, ys[:0], None, PAD, g_logp=one[:0]).shape == (8, 30)   # the binding: no call at all


# ----------------------------------------------------------------------------------------------------- 4. SeqLogpFn
@pytest.mark.parametrize("use", ["both", "logp", "token"])
def test_seq_logp_fn_under_autograd(use):
    from gct_plus_amd import engine
    n, W, V = 5, 11, 31
    ys, lens, x = kernel_case(n, W, V, seed=77)
    w, u = weights(n, W, seed=5)
    xd = x.cuda().requires_grad_()
    logp, token_logp, tokens, hits = engine.SeqLogpFn.apply(xd, ys.cuda(), lens.int().cuda(), PAD, 0)
    assert logp.requires_grad and token_logp.requires_grad and not tokens.requires_grad and not hits.requires_grad
    ref_tl, ref_lp, ref_nt, ref_nh = score_reference(x.double(), ys, lens, PAD)
    assert torch.equal(tokens.cpu(), ref_nt) and torch.equal(hits.cpu(), ref_nh)
    assert float((logp.detach().cpu().double() - ref_lp).abs().max()) <= W * 1e-4
    gl, gt = (None if use == "token" else w), (None if use == "logp" else u)       # an unused output's gradient is None
    obj = sum((g.cuda() * out).sum() for g, out in ((gl, logp), (gt, token_logp)) if g is not None)
    obj.backward()
    assert xd.grad.shape == xd.shape
    ref = seq_logp_grad_reference(x.double(), ys, lens, PAD, g_logp=None if gl is None else gl.double(),
                                  g_token=None if gt is None else gt.double())
    g = (0 if gl is None else gl[:, None]) + (0 if gt is None else gt[:, 1:]) + torch.zeros(n, W - 1)
    kernel_ratio(xd.grad, ref, float(g.abs().max()), f"SeqLogpFn {use}")


# ------------------------------------------------------------------------------------------------- 5. sequence_logp
def oracle_grads(model, mtype, c2d, extra, t, w):
    """The CPU oracle's autograd through score_reference: gradients of sum_r w_r logp_r for every parameter and z."""
    from oracle import gct_oracle as O
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, **dict(dict(use_cond2lat=True), **extra), **TINY)
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    z = t["z"].clone().requires_grad_()
    trg = t["ys"][:, :-1]
    logits = O.decode(P, cfg, trg, z, t["src_mask"], O.get_trg_mask(trg, PAD, c2d, t["dconds"] if nc else None),
                      t["dconds"])[:, nc if c2d else 0:]
    (w * score_reference(logits, t["ys"], t["lens"], PAD)[1]).sum().backward()
    return P, z.grad


@pytest.mark.parametrize("mtype,c2d", [("vaetf", False), ("pvaetf", False), ("scavaetf", False), ("pscavaetf", False),
                                       ("pvaetf", True)])
def test_sequence_logp_values_and_gradients_vs_oracle(ops, mtype, c2d):
    extra = dict(use_cond2dec=True, use_cond2lat=False) if c2d else {}
    model = build(mtype, seed=31, **extra)                                        # eval mode
    t = target_rows(mtype, 7)
    w = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.0, -1.25])
    z = t["z"].cuda().requires_grad_()
    args = (cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda())
    logp, tokens, hits, token_logp = sequence_logp(model, z, *args, prefix_lens=t["lens"], pad_id=PAD)
    want = score_tokens(model, z.detach(), *args, prefix_lens=t["lens"], pad_id=PAD)
    assert torch.equal(logp.detach(), want[0]) and torch.equal(tokens, want[1]) and torch.equal(hits, want[2])
    assert torch.equal(token_logp.detach(), want[3])
    assert logp.requires_grad and token_logp.requires_grad and not tokens.requires_grad and not hits.requires_grad
    model.zero_grad(set_to_none=True)
    (w.cuda() * logp).sum().backward()
    ops.assert_no_skipped_row_gradients()
    P, zg = oracle_grads(model, mtype, c2d, extra, t, w)
    floor = grad_floor([v.grad for v in P.values()] + [zg])
    seen = 0
    for name, p in model.named_parameters():
        e = P[name].grad
        if not name.startswith(("decoder.", "out.")):
            assert e is None or not e.any(), name                                 # the oracle agrees: z is an input
            assert p.grad is None or not p.grad.any(), f"{name}: the encoder side got a gradient"
            continue
        if e is None:
            assert p.grad is None or not p.grad.any(), name
            continue
        assert p.grad is not None, name
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad {name}")
        seen += 1
    assert seen > 20
    assert_close(z.grad, zg, 1e-5 * float(zg.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad z")
    assert not z.grad.cpu()[w == 0].any() and bool(z.grad.cpu()[w != 0].any())                # a zero weight contributes nothing


def test_sequence_logp_gradients_do_not_depend_on_the_row_plan(ops, monkeypatch):
    """24 rows: the planner takes the live rows (178 of 456, tests/test_score_gpu.py).  The same gradients with every
    live-row shortcut switched off, within test_compacted_decoder_backward_matches_dense's tolerance."""
    from gct_plus_amd import engine
    model = build("pscavaetf", seed=32)
    t = target_rows("pscavaetf", 8, lengths=(5, 20, 8, 12, 6, 16) + (6, 7, 9, 5, 8, 10) * 3)
    w = torch.randn(24, generator=torch.Generator().manual_seed(1))
    w[::5] = 0
    took = []
    finish = engine.RowPlan.finish

    def spy(self):
        plan = finish(self)
        took.append(plan.live is not None)
        return plan
    monkeypatch.setattr(engine.RowPlan, "finish", spy)
    grads = {}
    for mode in (True, False):
        for name in ("COMPACT_FWD", "COMPACT_BWD", "COMPACT_KV", "COMPACT_ENC_KV"):
            monkeypatch.setattr(engine, name, mode)
        took.clear()
        z = t["z"].cuda().requires_grad_()
        model.zero_grad(set_to_none=True)
        logp = sequence_logp(model, z, cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda(), prefix_lens=t["lens"],
                             pad_id=PAD)[0]
        (w.cuda() * logp).sum().backward()
        ops.assert_no_skipped_row_gradients()
        assert any(took) == mode                                                  # the shortcut ran, and only when it may
        grads[mode] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        grads[mode]["__z__"], grads[mode]["__logp__"] = z.grad.clone(), logp.detach().clone()
    floor = grad_floor(list(grads[False].values()))
    for n, e in grads[False].items():
        assert_close(grads[True][n], e, 2e-6 * float(e.abs().max()) + floor, 2e-5, f"live rows vs every row: {n}")


def test_sequence_logp_refuses_before_device_work():
    model = build("vaetf", seed=33)
    z, m = torch.randn(2, 8, TINY["latent_dim"]).cuda(), torch.ones(2, 1, 8, dtype=torch.bool).cuda()
    with pytest.raises(ValueError, match="positional table"):
        sequence_logp(model, z, m, None, torch.full((2, 202), 5), pad_id=PAD)
    with pytest.raises(ValueError):
        sequence_logp(model, z, m, None, torch.full((2, 9), 999), pad_id=PAD)
    with pytest.raises(ValueError, match="no column"):
        sequence_logp(model, z, m, None, torch.full((2, 9), PAD), pad_id=PAD)
    ys = torch.full((2, 9), PAD)
    ys[0, :4] = torch.tensor([SOS, 6, 7, EOS])                                    # row 1 scores nothing: value 0, grad 0
    zr = z.clone().requires_grad_()
    logp, tokens, _, _ = sequence_logp(model, zr, m, None, ys, pad_id=PAD)
    logp.sum().backward()
    assert float(logp.detach()[1]) == 0.0 and tokens.tolist() == [3, 0] and not zr.grad[1].any() and bool(zr.grad[0].any())


# --------------------------------------------------------------------------------------------------- 6. update step
def policy_sampler(mtype):
    """A greedy sampler over the update test's model: dropout 0, the oracle's initial state."""
    from gct_plus_amd.Inference import sampling_tool
    from gct_plus_amd.Model import model_dict
    cfg, state, t, reward = update_case(mtype)
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    model = model_dict[mtype](vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).cuda()
    model.load_state_dict(state)
    SRC, TRG = update_vocabs(mtype)
    sp = sampling_tool.sampling_tool_dict[mtype](model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=20,
                                                 cond_dim=nc, decode_algo="greedy")
    assert (sp.pad_id, sp.sos_id, sp.eos_id) == (PAD, SOS, EOS)
    return sp, t, reward


def greedy_matches_uncached(sp, z, src_mask, dconds, ys0):
    """The sampler's greedy decode of a uniform prefix against reference_style_decode on the same model: equal up to
    each row's first <eos>, or different first at a step where the un-cached logits have a top-2 gap under 1e-4."""
    from gct_plus_amd.Model.modules import get_trg_mask
    got = sp.decode(z, ys0, src_mask, dconds).cpu()
    ref = reference_style_decode(sp.model, z.cuda(), src_mask.cuda(), cu(dconds), ys0.cuda(), PAD, EOS, sp.max_strlen)
    t0 = ys0.shape[1]
    for r in range(ys0.shape[0]):
        a, b = upto_eos(got[r, t0:]), upto_eos(ref[r, t0:].cpu())
        if a == b:
            continue
        k = next(i for i, (x, y) in enumerate(zip(a + [None], b + [None])) if x != y)
        seen = ref[r:r + 1, :t0 + k]
        dc = None if dconds is None else dconds[r:r + 1].cuda()
        with torch.no_grad():
            last = sp.model.decode(seen, z[r:r + 1].cuda(), src_mask[r:r + 1].cuda(), get_trg_mask(seen, PAD, False, dc),
                                   dc)[0, -1]
        top2 = last.topk(2).values
        assert float(top2[0] - top2[1]) < 1e-4, (r, k, top2.tolist(), a, b)
    return got


@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_reinforce_steps_follow_the_oracle(ops, mtype):
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import reinforce_step
    sp, t, reward = policy_sampler(mtype)
    model = sp.model
    rows = DecodedRows(t["z"], t["ys"], t["src_mask"], t["dconds"], t["lens"])
    n = t["ys"].shape[0]
    t0 = 1 if t["lens"] is None else int(t["lens"][0])
    ys0 = t["ys"][:1, :t0].repeat(n, 1)                                           # one prefix for the un-cached loop
    greedy_matches_uncached(sp, t["z"], t["src_mask"], t["dconds"], ys0)          # folds the projections of the old weights
    fold_before = sp.kv._fold_key
    frozen = {k: p.detach().clone() for k, p in model.named_parameters() if not k.startswith(("decoder.", "out."))}
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = FusedAdam(model.parameters(), lr=UPDATE_LR, betas=(0.9, 0.98), eps=1e-9, model=model)
    lens = torch.ones(n, dtype=torch.long) if t["lens"] is None else t["lens"]
    n_scored = int(((torch.arange(t["ys"].shape[1])[None, :] >= lens[:, None]) & (t["ys"] != PAD)).sum())
    got = []
    for _ in range(UPDATE_STEPS):
        stats = reinforce_step(sp, opt, rows, reward)
        assert not model.training and set(stats) == {"loss", "mean_reward", "mean_logp", "tokens"}
        assert stats["tokens"] == n_scored
        assert abs(stats["mean_reward"] - float(reward.mean())) <= 1e-6
        got.append(-stats["loss"])
    with torch.no_grad():
        got.append(objective(sp.logp(*rows).logp, reward))
    ops.assert_no_skipped_row_gradients()
    want, P = oracle_run(mtype)
    print(f"{mtype}: objective per step, device {[round(v, 6) for v in got]}\n{' ' * len(mtype)}  oracle "
          f"{[round(v, 6) for v in want]}; worst relative difference "
          f"{max(abs(a - b) / abs(b) for a, b in zip(got, want)):.3e}")
    assert all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(got, want)), (got, want)
    assert all(b > a for a, b in zip(got, got[1:])), got                          # the device objective rises every step
    for k, p in model.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach(), frozen[k]), f"{k}: the encoder side moved"
    assert any(not torch.equal(p.detach(), start[k]) for k, p in model.named_parameters() if k.startswith("decoder."))
    greedy_matches_uncached(sp, t["z"], t["src_mask"], t["dconds"], ys0)          # the sampler decodes with the new weights
    assert sp.kv._fold_key != fold_before                                         # (its folded projections were redone)


# ------------------------------------------------------------------------------------------------------ 7. front end
SCAFFOLD = "c1ccccc1"
SCAFFOLDS = [SCAFFOLD, "CC", "C1CCNCC1"]


def entry_points(n, z, dconds):
    """The six sampling entry points as (class, model type, callable(sampler, **kw))."""
    many = (SCAFFOLDS * n)[:n]
    return [
        ("VaetfSampling", "vaetf", lambda sp, **kw: sp.sample_smiles(n, zs=z, **kw)),
        ("CvaetfSampling", "pvaetf", lambda sp, **kw: sp.sample_smiles(dconds, zs=z, transform=False, **kw)),
        ("ScaVaeSampling", "scavaetf", lambda sp, **kw: sp.sample_smiles(n, SCAFFOLD, zs=z, **kw)),
        ("ScaVaeSampling", "scavaetf", lambda sp, **kw: sp.sample_multiple_smiles(many, zs=z, **kw)),
        ("PscavaetfSampling", "pscavaetf", lambda sp, **kw: sp.sample_smiles(dconds, SCAFFOLD, zs=z, transform=False,
                                                                           **kw)),
        ("PscavaetfSampling", "pscavaetf", lambda sp, **kw: sp.sample_multiple_smiles(dconds, many, zs=z, transform=False,
                                                                                    **kw)),
    ]


def check_rows(sp, out, n, what):
    """out = (smiles, toklen, toklen_gen, logp, DecodedRows) of a with_logp sampler: shapes, and logp(*rows) against the
    log-probabilities the decode recorded."""
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    assert len(out) == 5 and isinstance(out[-1], DecodedRows), what
    smiles, logp, rows = out[0], out[3], out[4]
    assert len(smiles) == n and logp.shape == (n,)
    L = rows.ys.shape[1]
    assert rows.zs.shape[0] == n and rows.ys.shape == (n, L) and rows.src_mask.shape == (n, 1, rows.zs.shape[1])
    assert rows.ys.dtype == torch.int64 and rows.ys.is_cuda and rows.prefix_lens.shape == (n,)
    assert (rows.dconds is None) == (sp.cond_dim == 0)
    for r in range(n):                                                            # the rows hold the returned molecules
        t0 = int(rows.prefix_lens[r])
        assert sp.id_to_smi(rows.ys[r, t0:].tolist()).replace("<pad>", "") == smiles[r].replace("<pad>", ""), (what, r)
    with torch.no_grad():
        s = sp.logp(*rows)
    assert s.logp.is_cuda and s.token_logp.shape == (n, L) and bool((s.tokens >= 1).all())
    close_sums(logp, s.token_logp, f"{what}: logp(*rows) vs the decode's own log-probabilities")
    cpu = sp.score(*rows)
    assert torch.equal(cpu.logp, s.logp.cpu()) and not cpu.logp.is_cuda


@pytest.mark.parametrize("i", range(6))
def test_return_rows_on_every_entry_point(i):
    n = 6
    g = torch.Generator().manual_seed(6)
    z = torch.randn(n, 30, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    cls, mtype, call = entry_points(n, z, dconds)[i]
    algo = "multinomial" if i % 2 else "greedy"
    base = call(make_sampler(cls, mtype, algo, None))
    assert len(base) == 3 and isinstance(base[0], list)                           # the default: unchanged
    with_rows = call(make_sampler(cls, mtype, algo, None), return_rows=True)
    assert len(with_rows) == 4 and with_rows[:3] == base                          # (a fresh sampler: the same seed)
    sp = make_sampler(cls, mtype, algo, None, with_logp=True)
    assert len(call(sp)) == 4
    check_rows(sp, call(sp, return_rows=True), n, f"{cls} entry {i} {algo}")
    assert sp.logp(*with_rows[3]).logp.requires_grad                              # attached to the graph


@pytest.mark.parametrize("kw", [dict(stream_rows=4), dict(well_formed=True), dict(stream_rows=4, well_formed=True),
                                dict(top_k=5, temperature=0.8)])
def test_return_rows_with_stream_rows_and_grammar(kw):
    n = 9
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, 30, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    kw = dict(kw)
    rows = kw.pop("stream_rows", None)
    sp = make_sampler("PscavaetfSampling", "pscavaetf", "multinomial", rows, with_logp=True, **kw)
    check_rows(sp, sp.sample_smiles(dconds, SCAFFOLD, zs=z, transform=False, return_rows=True), n, f"sample_smiles {kw}")
    check_rows(sp, sp.sample_multiple_smiles(dconds, (SCAFFOLDS * 3), zs=z, transform=False, return_rows=True), n,
               f"sample_multiple_smiles {kw}")


def test_return_rows_refuses_beam_search():
    n = 3
    z = torch.randn(n, 30, 16, generator=torch.Generator().manual_seed(1))
    dconds = torch.rand(n, 3).numpy()
    sp = make_sampler("PscavaetfSampling", "pscavaetf", "beam", None)
    with pytest.raises(ValueError, match="beam"):
        sp.sample_smiles(dconds, SCAFFOLD, zs=z, transform=False, return_rows=True)
    with pytest.raises(ValueError, match="beam"):
        sp.sample_multiple_smiles(dconds, SCAFFOLDS, zs=z, transform=False, return_rows=True)
    sv = make_sampler("VaetfSampling", "vaetf", "beam", None)
    with pytest.raises(ValueError, match="beam"):
        sv.sample_smiles(n, zs=z, return_rows=True)
    assert len(sv.sample_smiles(n, zs=z)) == 3
