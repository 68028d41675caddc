"""PPO's clipped surrogate on the CPU: decode.ppo_reference against min(rho A, clamp(rho) A) written with torch.minimum /
torch.clamp, decode.ppo_grad_reference against torch.autograd through that formula (both fp64), the rows the rules must
not look at, the exact identities at old == lp, check_ppo_inputs' refusals, Train/finetune.advantages and ppo_loss, and
the oracle leg of the four-epoch update test (tests/test_ppo_gpu.py runs the device leg against it).

Condition on inputs.  Autograd through min / clamp and the rule differ only at a tie (rho exactly on a boundary), so the
sampling-time table is built as old = lp_fp64 + delta with delta drawn from {0, +-0.05, +-0.5}: the ratios are 1, 0.951,
1.051, 0.607 and 1.649, each at least 0.148 away from the boundaries 0.8 and 1.2 of clip 0.2 (the nearest: 1.2 -
exp(0.05) = 0.1487).  ppo_inputs asserts it; under the asymmetric clips (0.1, 0.3) and (0.3, 0.1) the nearest pair is
1.1 - exp(0.05) = 0.0487, asserted as 0.048."""
import math

import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd.decode import (PpoTerms, check_ppo_inputs, clip_pair, ppo_grad_reference, ppo_reference,
                                 score_reference)
from gct_plus_amd.Train.finetune import advantages, ppo_loss, ppo_update, reinforce_loss
from tests.test_mixed_scaffold_decode_gpu import PAD, TINY
from tests.test_policy_terms_host import scored_columns
from tests.test_score_gpu import target_rows
from tests.test_seq_logp_grad_host import grad_case

SHAPES = [(1, 2, 2), (3, 8, 30), (4, 12, 31)]
NAN = float("nan")
CLIP = 0.2
DELTAS = (0.0, 0.05, -0.05, 0.5, -0.5)
MARGIN = 0.148                                            # every ratio's distance from a boundary of clip 0.2
MARGIN_ASYMMETRIC = 0.048                                 # ... and of the clips (0.1, 0.3) and (0.3, 0.1)


def ppo_inputs(ys, lens, x, seed, clip=(CLIP, CLIP)):
    """What the surrogate takes beside a scoring case (ys, lens, logits x), fp64: old [n, W] = lp_fp64 + delta with delta
    from DELTAS (0 and +-0.05 with probability 0.1 each, +-0.5 with 0.35 each: about a third of the scored tokens has a
    ratio beyond each boundary); advantage [n] of both signs (row 0's: positive for even W, negative for odd), row 1's
    exactly 0; g_surrogate [n] and g_token_surrogate
    [n, W] of mixed sign with zeros, row 0's pair cancelling exactly at its first scored column.  Asserts that every
    scored ratio is at least MARGIN (clip 0.2; MARGIN_ASYMMETRIC otherwise) away from 1 - clip_lo and 1 + clip_hi."""
    n, W = ys.shape
    g = torch.Generator().manual_seed(seed)
    lp = score_reference(x.double(), ys, lens, PAD)[0]
    pick = torch.multinomial(torch.tensor([0.1, 0.1, 0.1, 0.35, 0.35]), n * W, replacement=True, generator=g)
    old = lp + torch.tensor(DELTAS, dtype=torch.float64)[pick].view(n, W)
    adv = torch.randn(n, generator=g, dtype=torch.float64)
    adv[0] = adv[0].abs() if W % 2 == 0 else -adv[0].abs()                        # row 0 is the one every case scores
    if n > 1:
        adv[1] = 0
    g_s = torch.randn(n, generator=g, dtype=torch.float64)
    g_ts = torch.randn(n, W, generator=g, dtype=torch.float64)
    g_ts[torch.rand(n, W, generator=g) < 0.25] = 0
    scored = scored_columns(ys, lens)
    if bool(scored[0].any()):
        c = int(scored[0].nonzero()[0]) + 1
        g_s[0], g_ts[0, c] = 1.5, -1.5                                            # a scored column whose weight is 0
    rho = torch.exp(lp - old)[:, 1:][scored]
    lo, hi = 1 - clip[0], 1 + clip[1]
    margin = MARGIN if tuple(clip) == (CLIP, CLIP) else MARGIN_ASYMMETRIC
    assert rho.numel() == 0 or float(torch.minimum((rho - lo).abs(), (rho - hi).abs()).min()) >= margin
    return old, adv, g_s, g_ts


def textbook(x, ys, lens, old, adv, clip_lo, clip_hi):
    """PPO's surrogate as the papers write it, fp64, differentiable in x: (token_surrogate [n, W - 1], k3 terms, rho) at
    the scored columns, 0 elsewhere."""
    scored = scored_columns(ys, lens)
    lp = torch.log_softmax(x, -1).gather(-1, ys[:, 1:].unsqueeze(-1)).squeeze(-1)
    d = lp - old[:, 1:]
    rho = torch.exp(d)
    A = adv.view(-1, 1)
    s = torch.minimum(rho * A, torch.clamp(rho, 1 - clip_lo, 1 + clip_hi) * A)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(scored, s, zero), torch.where(scored, rho - 1 - d, zero), torch.where(scored, rho, zero)


# ------------------------------------------------------------------------------------------------- 1. the values
@pytest.mark.parametrize("clip", [(0.2, 0.2), (0.1, 0.3), (0.3, 0.1)])
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_rule_against_min_and_clamp(n, W, V, clip):
    ys, lens, x, _, _ = grad_case(n, W, V, seed=100 * n + W)
    ys = ys.clone()
    for pl in (lens, None):
        old, adv, _, _ = ppo_inputs(ys, pl, x, seed=7, clip=clip)
        want_s, want_k, rho = textbook(x, ys, pl, old, adv, *clip)
        scored = scored_columns(ys, pl)
        tl, ts, lp, su, kl, nt, nh, nc = ppo_reference(x, ys, pl, PAD, old, adv, *clip)
        ref = score_reference(x, ys, pl, PAD)
        assert torch.equal(tl, ref[0]) and torch.equal(lp, ref[1]) and torch.equal(nt, ref[2]) and torch.equal(nh, ref[3])
        assert ts.dtype == torch.float64 and ts.shape == (n, W) and su.shape == kl.shape == (n,) and nc.dtype == torch.int32
        assert not ts[:, 0].any() and not ts[:, 1:][~scored].any()                # exact zeros off the scored columns
        assert float((ts[:, 1:] - want_s).abs().max()) <= 1e-12
        assert float((su - want_s.sum(1)).abs().max()) <= 1e-12 * W
        assert float((kl - want_k.sum(1)).abs().max()) <= 1e-12 * W and bool((kl >= 0).all())
        A = adv.view(-1, 1)
        clipped = scored & (((A > 0) & (rho > 1 + clip[1])) | ((A < 0) & (rho < 1 - clip[0])))
        assert torch.equal(nc, clipped.sum(1).to(torch.int32))
        if n > 1:
            assert int(nc[1]) == 0 and not ts[1].any()                            # A == 0: never clipped, surrogate 0
    if n > 2:
        assert int(nc.sum()) > 0                                                  # the case does clip
    assert ppo_reference(x.float(), ys, lens, PAD, old, adv, *clip)[1].dtype == torch.float32
    with pytest.raises(ValueError):
        ppo_reference(x[:, :-1], ys, lens, PAD, old, adv, *clip)


@pytest.mark.parametrize("clip", [0.0, 0.2])
def test_old_equal_to_lp_is_exact(clip):
    """Ratios of exactly 1: surrogate = A * tokens, nothing clipped and approx_kl 0, exactly -- also with a clip of 0 --
    and the gradient is seq_logp_grad_reference's with the weight g * A.  The advantages are multiples of 1/8, so that
    the ascending sum of `tokens` copies of A is A * tokens without rounding."""
    from gct_plus_amd.decode import seq_logp_grad_reference
    n, W, V = 4, 12, 31
    ys, lens, x, g_s, g_ts = grad_case(n, W, V, seed=11)
    adv = torch.tensor([1.5, -0.25, 0.0, 2.125], dtype=torch.float64)
    for xx in (x, x.float()):
        old = score_reference(xx, ys, lens, PAD)[0]
        tl, ts, lp, su, kl, nt, nh, nc = ppo_reference(xx, ys, lens, PAD, old, adv, clip, clip)
        assert torch.equal(su, adv.to(xx.dtype) * nt) and not nc.any() and not kl.any()
        assert torch.equal(ts[:, 1:], torch.where(scored_columns(ys, lens), adv.to(xx.dtype).view(-1, 1),
                                                  torch.zeros((), dtype=xx.dtype)))
        got = ppo_grad_reference(xx, ys, lens, PAD, old, adv, clip, clip, g_surrogate=g_s, g_token_surrogate=g_ts)
        gA = (g_s.view(-1, 1) + g_ts).to(xx.dtype) * adv.to(xx.dtype).view(-1, 1)
        want = seq_logp_grad_reference(xx, ys, lens, PAD, g_token=gA)
        tol = 1e-12 if xx.dtype == torch.float64 else 1e-5                        # (two softmax forms: e / sum, exp(lsm))
        assert float((got - want).abs().max()) <= tol * float(want.abs().max())
        assert not got[2].any()                                                   # A == 0


# ---------------------------------------------------------------------------------------------- 2. the gradient
@pytest.mark.parametrize("which", ["surrogate", "token", "both"])
@pytest.mark.parametrize("clip", [(0.2, 0.2), (0.1, 0.3)])
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_gradient_rule_against_autograd_through_min_and_clamp(n, W, V, clip, which):
    ys, lens, x, _, _ = grad_case(n, W, V, seed=100 * n + W)
    for pl in (lens, None):
        old, adv, g_s, g_ts = ppo_inputs(ys, pl, x, seed=8, clip=clip)
        gs, gt = (g_s if which != "token" else None), (g_ts if which != "surrogate" else None)
        xa = x.clone().requires_grad_()
        s, _, _ = textbook(xa, ys, pl, old, adv, *clip)
        obj = torch.zeros((), dtype=torch.float64)
        if gs is not None:
            obj = obj + (gs * s.sum(1)).sum()
        if gt is not None:
            obj = obj + (gt[:, 1:] * s).sum()
        want, = torch.autograd.grad(obj, xa, allow_unused=True)
        want = torch.zeros_like(x) if want is None else want
        got = ppo_grad_reference(x, ys, pl, PAD, old, adv, *clip, g_surrogate=gs, g_token_surrogate=gt)
        assert got.dtype == torch.float64 and got.shape == x.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (which, pl is None)
        assert not got[~scored_columns(ys, pl)].any()                             # exact zeros off the scored rows
        if n > 1:
            assert not got[1].any()                                               # A == 0
        # autograd through the rule itself is the same gradient
        xb = x.clone().requires_grad_()
        out = ppo_reference(xb, ys, pl, PAD, old, adv, *clip)
        obj = (0 if gs is None else (gs * out[3]).sum()) + (0 if gt is None else (gt * out[1]).sum())
        auto, = torch.autograd.grad(obj, xb)
        assert float((got - auto).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_rules_never_look_at_a_row_they_need_not():
    """NaN logits in every row that is not scored (values) and in every row that is not scored, or has A == 0 or
    g == 0 (gradient): finite results, the same, exact zeros there.  A clipped token's row gets exact zeros as well, but
    it is looked at.  NaN in old_token_logp at columns that are not scored changes nothing either."""
    n, W, V = 4, 12, 31
    ys, lens, x, _, _ = grad_case(n, W, V, seed=9)
    old, adv, g_s, g_ts = ppo_inputs(ys, lens, x, seed=11)
    scored = scored_columns(ys, lens)
    g = g_s.view(-1, 1) + g_ts[:, 1:]
    looked = scored & (g != 0) & (adv.view(-1, 1) != 0)
    assert bool((scored & (g == 0)).any()) and bool((scored & ~looked).any())
    want_v = ppo_reference(x, ys, lens, PAD, old, adv, CLIP, CLIP)
    want_g = ppo_grad_reference(x, ys, lens, PAD, old, adv, CLIP, CLIP, g_surrogate=g_s, g_token_surrogate=g_ts)
    xs, olds = x.clone(), old.clone()
    xs[~scored] = NAN
    olds[:, 1:][~scored] = NAN
    olds[:, 0] = NAN
    got_v = ppo_reference(xs, ys, lens, PAD, olds, adv, CLIP, CLIP)
    assert all(bool(torch.isfinite(a.double()).all()) and torch.equal(a, b) for a, b in zip(got_v, want_v))
    xs[~looked] = NAN
    olds[:, 1:][~looked] = NAN
    got_g = ppo_grad_reference(xs, ys, lens, PAD, olds, adv, CLIP, CLIP, g_surrogate=g_s, g_token_surrogate=g_ts)
    assert bool(torch.isfinite(got_g).all()) and torch.equal(got_g, want_g) and not got_g[~looked].any()
    _, _, rho = textbook(x, ys, lens, old, adv, CLIP, CLIP)
    A = adv.view(-1, 1)
    clipped = looked & (((A > 0) & (rho > 1 + CLIP)) | ((A < 0) & (rho < 1 - CLIP)))
    assert bool(clipped.any()) and not got_g[clipped].any() and bool(got_g[looked & ~clipped].any(-1).all())
    assert ppo_grad_reference(xs.float(), ys, lens, PAD, olds, adv, CLIP, CLIP, g_surrogate=g_s).dtype == torch.float32


# --------------------------------------------------------------------------------------------------- 3. refusals
def test_check_ppo_inputs_refusals():
    n, W = 3, 5
    old, adv = torch.zeros(n, W), torch.zeros(n)
    assert torch.equal(check_ppo_inputs(old, adv, 0.0, 0.0, n, W), adv)
    assert check_ppo_inputs(old.double(), [0.5, -1, 2], 0.999, 7.5, n, W).shape == (n,)
    bad = [dict(old=torch.zeros(n, W, dtype=torch.long)), dict(old=torch.zeros(n, W + 1)), dict(old=torch.zeros(n * W)),
           dict(old=[[0.0] * W] * n), dict(adv=torch.zeros(n + 1)), dict(adv=torch.zeros(n, 1)),
           dict(adv=torch.tensor([0.0, NAN, 1.0])), dict(adv=torch.tensor([0.0, math.inf, 1.0])),
           dict(adv=torch.zeros(n, dtype=torch.bool)), dict(lo=-0.01), dict(lo=1.0), dict(lo=NAN), dict(hi=-0.01),
           dict(hi=NAN), dict(lo="0.2"), dict(hi=None)]
    for over in bad:
        a = dict(dict(old=old, adv=adv, lo=0.2, hi=0.2), **over)
        with pytest.raises(ValueError):
            check_ppo_inputs(a["old"], a["adv"], a["lo"], a["hi"], n, W)
    ys = torch.full((n, W), 5)
    with pytest.raises(ValueError, match="clip_lo"):
        ppo_reference(torch.zeros(n, W - 1, 9), ys, None, PAD, old, adv, 1.0, 0.2)
    with pytest.raises(ValueError, match="advantage"):
        ppo_grad_reference(torch.zeros(n, W - 1, 9), ys, None, PAD, old, adv[:2], 0.2, 0.2, g_surrogate=adv)
    assert clip_pair(0.2) == (0.2, 0.2) and clip_pair((0.1, 0.3)) == (0.1, 0.3) and clip_pair([0, 1]) == (0.0, 1.0)
    for c in (None, "0.2", (0.1,), (0.1, 0.2, 0.3), True, (0.1, "x")):
        with pytest.raises(ValueError, match="clip"):
            clip_pair(c)


# ---------------------------------------------------------------------------------------- 4. advantages, the loss
def test_advantages_follow_the_baseline_rule_of_reinforce_loss():
    g = torch.Generator().manual_seed(1)
    reward = torch.rand(7, generator=g)
    logp = (-torch.rand(7, generator=g) * 30).requires_grad_()
    b = torch.rand(7, generator=g)
    for baseline in ("mean", 0.25, b, None):
        adv = advantages(reward, baseline)
        assert adv.dtype == torch.float32 and adv.shape == (7,) and not adv.requires_grad
        grad, = torch.autograd.grad(reinforce_loss(logp, reward, baseline), logp)
        assert torch.allclose(-grad * 7, adv, rtol=1e-6, atol=1e-7)               # the weight reinforce_loss gives logp
    assert torch.equal(advantages(reward), reward - reward.mean())
    norm = advantages(reward, normalize=True)
    a = reward - reward.mean()
    assert torch.allclose(norm, a / (a.pow(2).mean().sqrt() + 1e-8), rtol=1e-6, atol=0)
    assert abs(float(norm.pow(2).mean()) - 1) <= 1e-5
    assert not advantages(torch.full((4,), 0.5), normalize=True).any()            # equal rewards: 0 / 1e-8, not NaN
    assert advantages([1, 2, 3]).tolist() == [-1.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        advantages(reward, baseline="median")
    with pytest.raises(ValueError):
        advantages(reward, baseline=torch.zeros(7, 2))


def fake_terms(n, W, seed):
    g = torch.Generator().manual_seed(seed)
    zeros, ints = torch.zeros(n, W), torch.ones(n, dtype=torch.int32)
    surrogate, entropy, kl = torch.randn(n, generator=g), torch.rand(n, generator=g) * 20, torch.rand(n, generator=g) * 5
    return PpoTerms(zeros[:, 0], ints, ints, zeros, entropy, zeros, kl, zeros, zeros[:, 0], surrogate, zeros, zeros[:, 0],
                    ints)


def test_ppo_loss_is_its_formula():
    n = 7
    t = fake_terms(n, 9, seed=2)
    assert torch.equal(ppo_loss(t), -t.surrogate.sum() / n)
    want = (-t.surrogate.sum() + 0.5 * t.kl.sum() - 0.05 * t.entropy.sum()) / n
    assert torch.allclose(ppo_loss(t, entropy_coef=0.05, kl_coef=0.5), want, rtol=1e-6, atol=0)
    s, en, k = (x.clone().requires_grad_() for x in (t.surrogate, t.entropy, t.kl))
    ppo_loss(t._replace(surrogate=s, entropy=en, kl=k), entropy_coef=0.05, kl_coef=0.5).backward()
    assert torch.equal(s.grad, torch.full((n,), -1.0) / n)
    assert torch.allclose(en.grad, torch.full((n,), -0.05 / n)) and torch.allclose(k.grad, torch.full((n,), 0.5 / n))
    bare = t._replace(entropy=None, token_entropy=None, kl=None, token_kl=None, prior_logp=None)
    assert torch.equal(ppo_loss(bare), ppo_loss(t))
    with pytest.raises(ValueError, match="prior"):
        ppo_loss(bare, kl_coef=0.5)
    with pytest.raises(ValueError, match="entropy"):
        ppo_loss(bare, entropy_coef=0.5)


def test_ppo_update_refuses_before_device_work():
    class Untouched:                                     # any use of the sampler or the optimizer would raise
        model = None
    rows = (None, torch.zeros(3, 5, dtype=torch.long))
    with pytest.raises(ValueError, match="prior"):
        ppo_update(Untouched(), None, rows, torch.zeros(3), kl_coef=0.1)
    for kw in (dict(epochs=0), dict(epochs=1.5), dict(minibatch=0), dict(clip="x"), dict(clip=(0.1, 0.2, 0.3))):
        with pytest.raises(ValueError):
            ppo_update(Untouched(), None, rows, torch.zeros(3), **kw)
    with pytest.raises(ValueError, match="rewards"):
        ppo_update(Untouched(), None, rows, torch.zeros(4))


# ------------------------------------------------------------------------------------- the update test, oracle leg
PPO_MTYPE = "vaetf"
PPO_SEED = 5
PPO_EPOCHS, PPO_LR = 4, 2.5e-4                           # lr chosen on the ORACLE alone: clip fractions 0, 0.11, 0.37, 0.61, no
                                                          # ratio within NEAR of a boundary, no loss close to 0
PPO_LENGTHS = (5, 20, 8, 12, 6, 16, 9, 14)                # n = 8, a power of two: (-1 / n) * A == -(A / n)
NEAR = 1e-3                                               # a ratio this close to a boundary is left out of the clipped sets
NEAR_CAP = 0.05                                           # ... and those may be this share of the scored tokens


def ppo_update_case():
    """Fixed rows and rewards of the PPO update test: (cfg, initial state, rows dict of target_rows, reward [8])."""
    from oracle import gct_oracle as O
    vs, vt = synthetic.vocab_sizes(PPO_MTYPE)
    cfg = O.make_cfg(PPO_MTYPE, vs, vt, dropout=0.0, nconds=synthetic.n_conds(PPO_MTYPE), use_cond2lat=True, **TINY)
    state = O.init_state(cfg, seed=PPO_SEED)
    rows = target_rows(PPO_MTYPE, 40 + PPO_SEED, lengths=PPO_LENGTHS)
    reward = torch.rand(len(PPO_LENGTHS), generator=torch.Generator().manual_seed(3))
    return cfg, state, rows, reward


def oracle_ppo_epochs():
    """PPO_EPOCHS epochs of torch.optim.Adam (the reference's betas and eps) on the CPU oracle, the surrogate from
    ppo_reference on the oracle's teacher-forced logits under torch autograd, old_token_logp = the initial policy's
    token_logp, advantages(reward), clip 0.2.  Returns dict(loss, approx_kl (per token), clip_fraction, clipped: bool
    [n, W - 1] per epoch, rho: [n, W - 1] per epoch, scored), every entry at that epoch's forward."""
    from oracle import gct_oracle as O
    cfg, state, t, reward = ppo_update_case()
    P = O.make_leaves(state)
    opt = O.make_adam(O.trainable(P, cfg), lr=PPO_LR)
    ys = t["ys"]
    trg = ys[:, :-1]
    trg_mask = O.get_trg_mask(trg, PAD, False, None)
    adv = advantages(reward)
    scored = scored_columns(ys, t["lens"])
    out = dict(loss=[], approx_kl=[], clip_fraction=[], clipped=[], rho=[], scored=scored)
    old = None
    for _ in range(PPO_EPOCHS):
        logits = O.decode(P, cfg, trg, t["z"], t["src_mask"], trg_mask, t["dconds"], train=True)
        if old is None:
            old = score_reference(logits.detach(), ys, t["lens"], PAD)[0]
        tl, ts, lp, su, kl, nt, nh, nc = ppo_reference(logits, ys, t["lens"], PAD, old, adv, CLIP, CLIP)
        loss = -su.sum() / su.numel()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        rho = torch.exp(tl.detach() - old)[:, 1:]
        A = adv.view(-1, 1)
        out["loss"].append(float(loss.detach()))
        out["approx_kl"].append(float(kl.detach().sum() / nt.sum()))
        out["clip_fraction"].append(float(nc.sum()) / float(nt.sum()))
        out["clipped"].append(scored & (((A > 0) & (rho > 1 + CLIP)) | ((A < 0) & (rho < 1 - CLIP))))
        out["rho"].append(rho)
    return out


_ORACLE = {}


def oracle_ppo_run():
    """oracle_ppo_epochs, computed once per process and shared by the host and the device test."""
    if "run" not in _ORACLE:
        _ORACLE["run"] = oracle_ppo_epochs()
    return _ORACLE["run"]


def near_a_boundary(rho, scored):
    """Scored tokens whose ratio lies within NEAR of 1 - CLIP or 1 + CLIP."""
    return scored & (((rho - (1 - CLIP)).abs() <= NEAR) | ((rho - (1 + CLIP)).abs() <= NEAR))


def test_oracle_ppo_epochs_clip_and_stay_clear_of_the_boundaries():
    run = oracle_ppo_run()
    scored = run["scored"]
    tokens = int(scored.sum())
    near = [int(near_a_boundary(rho, scored).sum()) for rho in run["rho"]]
    print(f"oracle PPO epochs: loss {[round(v, 6) for v in run['loss']]}, approx_kl "
          f"{[round(v, 7) for v in run['approx_kl']]}, clip fraction {[round(v, 4) for v in run['clip_fraction']]}, "
          f"tokens within {NEAR} of a boundary {near} of {tokens}")
    assert len(run["loss"]) == PPO_EPOCHS and all(math.isfinite(v) for v in run["loss"])
    assert run["approx_kl"][0] == 0.0 and all(v > 0 for v in run["approx_kl"][1:])
    assert run["clip_fraction"][0] == 0.0 and int(run["clipped"][-1].sum()) > 0   # some tokens are clipped in the end
    assert all(k <= NEAR_CAP * tokens for k in near), near
    assert all(b < a for a, b in zip(run["loss"], run["loss"][1:])), run["loss"]  # the surrogate rises every epoch
