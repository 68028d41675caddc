"""The backward rule of the sequence log-likelihood on the CPU (decode.seq_logp_grad_reference) against torch.autograd
through decode.score_reference in fp64, Train/finetune.reinforce_loss against its formula, and the oracle leg of the
policy-gradient update test (tests/test_seq_logp_grad_gpu.py runs the device leg against it): five Adam steps on the
CPU oracle whose own objective must rise at every step."""
import pytest
import torch

from gct_plus_amd import data, synthetic
from gct_plus_amd.decode import score_reference, seq_logp_grad_reference
from gct_plus_amd.Train.finetune import reinforce_loss
from tests.test_mixed_scaffold_decode_gpu import PAD, TINY
from tests.test_score_gpu import target_rows

SHAPES = [(1, 2, 2), (3, 8, 30), (4, 12, 31)]


def grad_case(n, W, V, seed):
    """ys [n, W] with pad inside the rows (not only behind them), mixed prefix lengths -- the last row's prefix fills
    it (t0 = W) --, logits fp64 [n, W - 1, V], g_logp [n] and g_token [n, W] of mixed sign; row 0's g_logp and a few
    entries of g_token are 0."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.randint(0, V, (n, W), generator=g)
    ys[ys == PAD] = 0
    ys[torch.rand(n, W, generator=g) < 0.2] = PAD
    lens = torch.randint(1, W + 1, (n,), generator=g)
    lens[0] = 1
    if n > 1:
        lens[-1] = W
    if V > 2:
        ys[0, 1] = 2                                                              # row 0 scores at least one token
    x = torch.randn(n, W - 1, V, generator=g, dtype=torch.float64) * 3
    g_logp = torch.randn(n, generator=g, dtype=torch.float64)
    g_token = torch.randn(n, W, generator=g, dtype=torch.float64)
    g_token[torch.rand(n, W, generator=g) < 0.25] = 0
    return ys, lens, x, g_logp, g_token


@pytest.mark.parametrize("which", ["logp", "token", "both", "zero_weight"])
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_rule_against_autograd_through_score_reference(n, W, V, which):
    ys, lens, x, g_logp, g_token = grad_case(n, W, V, seed=100 * n + W)
    if which == "logp":
        g_token = None
    elif which == "token":
        g_logp = None
    elif which == "zero_weight":
        g_logp, g_token = torch.zeros_like(g_logp), g_token.clone()
        g_token[0] = 0                                                            # every weight of row 0 is 0
    for pl in (lens, None):
        xa = x.clone().requires_grad_()
        token_logp, logp, _, _ = score_reference(xa, ys, pl, PAD)
        obj = torch.zeros((), dtype=torch.float64)
        if g_logp is not None:
            obj = obj + (g_logp * logp).sum()
        if g_token is not None:
            obj = obj + (g_token * token_logp).sum()
        want, = torch.autograd.grad(obj, xa, allow_unused=True)
        want = torch.zeros_like(x) if want is None else want
        got = seq_logp_grad_reference(x, ys, pl, PAD, g_logp=g_logp, g_token=g_token)
        assert got.dtype == torch.float64 and got.shape == x.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (which, pl is None)
        t0 = torch.ones(n, dtype=torch.long) if pl is None else pl
        scored = (torch.arange(1, W)[None, :] >= t0[:, None]) & (ys[:, 1:] != PAD)
        assert not got[~scored].any()                                             # exact zeros off the scored rows
        if which == "zero_weight":
            assert not got[0].any()
    if n > 1:
        assert not seq_logp_grad_reference(x, ys, lens, PAD, g_logp=g_logp, g_token=g_token)[-1].any()   # t0 = W


def test_rule_never_looks_at_a_row_it_does_not_score():
    """NaN logits in every row that is not scored or has weight 0: the gradient is finite and exactly 0 there; fp32
    logits give an fp32 gradient."""
    n, W, V = 4, 12, 31
    ys, lens, x, g_logp, g_token = grad_case(n, W, V, seed=9)
    g_logp[1] = 0
    g_token[1] = 0
    scored = (torch.arange(1, W)[None, :] >= lens[:, None]) & (ys[:, 1:] != PAD)
    live = scored & ((g_logp[:, None] + g_token[:, 1:]) != 0)
    want = seq_logp_grad_reference(x, ys, lens, PAD, g_logp=g_logp, g_token=g_token)
    xs = x.clone()
    xs[~live] = float("nan")
    got = seq_logp_grad_reference(xs, ys, lens, PAD, g_logp=g_logp, g_token=g_token)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want) and not got[~live].any()
    assert seq_logp_grad_reference(xs.float(), ys, lens, PAD, g_logp=g_logp).dtype == torch.float32
    with pytest.raises(ValueError):
        seq_logp_grad_reference(x[:, :-1], ys, lens, PAD, g_logp=g_logp)


def test_reinforce_loss_is_its_formula():
    g = torch.Generator().manual_seed(1)
    logp = -torch.rand(7, generator=g) * 30
    reward = torch.rand(7, generator=g)
    n = 7
    assert torch.allclose(reinforce_loss(logp, reward), -((reward - reward.mean()) * logp).sum() / n, rtol=1e-6, atol=0)
    assert torch.allclose(reinforce_loss(logp, reward, baseline=0.25), -((reward - 0.25) * logp).sum() / n, rtol=1e-6,
                          atol=0)
    b = torch.rand(7, generator=g)
    assert torch.allclose(reinforce_loss(logp, reward, baseline=b), -((reward - b) * logp).sum() / n, rtol=1e-6, atol=0)
    assert torch.allclose(reinforce_loss(logp, reward, baseline=None), -(reward * logp).sum() / n, rtol=1e-6, atol=0)
    # the gradient goes to logp only, with the advantage as its weight
    lp = logp.clone().requires_grad_()
    rw = reward.clone().requires_grad_()
    reinforce_loss(lp, rw).backward()
    assert rw.grad is None and torch.allclose(lp.grad, -(reward - reward.mean()) / n, rtol=1e-6, atol=1e-9)
    with pytest.raises(ValueError):
        reinforce_loss(logp, reward[:3])
    with pytest.raises(ValueError):
        reinforce_loss(logp, reward, baseline="median")


# ------------------------------------------------------------------------------------- the update step, oracle leg
UPDATE_STEPS, UPDATE_LR = 5, 1e-4
UPDATE_SEED = {"pscavaetf": 5, "vaetf": 5}               # chosen so that the ORACLE's objective rises at every step


def update_vocabs(mtype):
    """(SRC, TRG) vocabularies of synthetic.vocab_sizes(mtype) entries with the synthetic ids of the special tokens."""
    vs, vt = synthetic.vocab_sizes(mtype)
    trg = [t for t in synthetic.GRAMMAR_VOCAB if vt == 31 or t != "<sep>"]
    src = [t for t in trg if t not in ("<sos>", "<eos>")]
    assert len(trg) == vt and len(src) == vs and trg.index("<pad>") == PAD == src.index("<pad>")
    return data.Vocab(src), data.Vocab(trg)


def update_case(mtype):
    """Fixed rows and rewards of the update test: (cfg, initial state, rows dict of target_rows, reward [n])."""
    from oracle import gct_oracle as O
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY)
    state = O.init_state(cfg, seed=UPDATE_SEED[mtype])
    rows = target_rows(mtype, 40 + UPDATE_SEED[mtype])
    reward = torch.rand(rows["ys"].shape[0], generator=torch.Generator().manual_seed(3))
    return cfg, state, rows, reward


def objective(logp, reward):
    """What reinforce_step raises: the batch mean of (reward - mean reward) * logp = -reinforce_loss."""
    return float(((reward - reward.mean()) * logp.detach().cpu().float()).sum() / logp.numel())


def oracle_objectives(mtype):
    """UPDATE_STEPS steps of torch.optim.Adam (the reference's betas and eps, lr 1e-4) on the CPU oracle, the policy
    term from score_reference on the oracle's teacher-forced logits: the objective at each step's forward and after the
    last step (UPDATE_STEPS + 1 numbers), and the final state."""
    from oracle import gct_oracle as O
    cfg, state, t, reward = update_case(mtype)
    P = O.make_leaves(state)
    opt = O.make_adam(O.trainable(P, cfg), lr=UPDATE_LR)
    ys, nc = t["ys"], cfg["nconds"]
    trg = ys[:, :-1]
    trg_mask = O.get_trg_mask(trg, PAD, False, t["dconds"] if nc else None)

    def logp():
        logits = O.decode(P, cfg, trg, t["z"], t["src_mask"], trg_mask, t["dconds"], train=True)
        return score_reference(logits, ys, t["lens"], PAD)[1]
    out = []
    for _ in range(UPDATE_STEPS):
        lp = logp()
        opt.zero_grad(set_to_none=True)
        reinforce_loss(lp, reward).backward()
        opt.step()
        out.append(objective(lp, reward))
    with torch.no_grad():
        out.append(objective(logp(), reward))
    return out, P


_ORACLE = {}


def oracle_run(mtype):
    """oracle_objectives, computed once per process and shared by the host and the device test."""
    if mtype not in _ORACLE:
        _ORACLE[mtype] = oracle_objectives(mtype)
    return _ORACLE[mtype]


@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_oracle_objective_rises_at_every_step(mtype):
    from oracle import gct_oracle as O
    obj, P = oracle_run(mtype)
    print(f"{mtype}: oracle objective per step {[round(v, 6) for v in obj]}")
    assert len(obj) == UPDATE_STEPS + 1
    assert all(b > a for a, b in zip(obj, obj[1:])), obj
    cfg, state, _, _ = update_case(mtype)
    moved = [k for k in O.param_names(cfg) if not torch.equal(P[k].detach(), state[k])]
    assert moved and all(k.startswith(("decoder.", "out.")) for k in moved)       # the encoder gets no gradient
