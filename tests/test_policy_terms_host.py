"""The distribution terms of a policy on the CPU: decode.dist_reference (entropy of the next-token distribution, KL from
a prior) against plain torch.log_softmax / softmax formulas, decode.dist_grad_reference against torch.autograd through
dist_reference in fp64, Train/finetune.regularised_loss against its formula, and the oracle leg of the regularised
update test (tests/test_policy_terms_gpu.py runs the device leg against it): UPDATE_STEPS Adam steps on the CPU oracle
with an entropy bonus and a KL penalty against a frozen copy of the initial state."""
import math

import pytest
import torch

from gct_plus_amd.decode import PolicyTerms, dist_grad_reference, dist_reference, score_reference
from gct_plus_amd.Train.finetune import regularised_loss, reinforce_loss, reinforce_step
from tests.test_mixed_scaffold_decode_gpu import PAD
from tests.test_seq_logp_grad_host import UPDATE_LR, UPDATE_STEPS, grad_case, update_case

SHAPES = [(1, 2, 2), (3, 8, 30), (4, 12, 31)]
ENTROPY_COEF, KL_COEF = 0.05, 0.5
NAN = float("nan")


def dist_case(n, W, V, seed, neg_inf=False):
    """grad_case's rows and agent logits, an independent draw for the prior, and the four weight tables (g_entropy [n],
    g_token_entropy [n, W], g_kl [n], g_token_kl [n, W]; a quarter of the token tables is 0).  neg_inf: a -inf logit at
    one index of row 0's first logits row (scored: grad_case puts a token there for V > 2), in agent and prior."""
    ys, lens, x, g_e, g_te = grad_case(n, W, V, seed)
    g = torch.Generator().manual_seed(seed + 1)
    q = torch.randn(n, W - 1, V, generator=g, dtype=torch.float64) * 3
    g_k = torch.randn(n, generator=g, dtype=torch.float64)
    g_tk = torch.randn(n, W, generator=g, dtype=torch.float64)
    g_tk[torch.rand(n, W, generator=g) < 0.25] = 0
    if neg_inf:
        x[0, 0, V - 1] = q[0, 0, V - 1] = -math.inf
    return ys, lens, x, q, (g_e, g_te, g_k, g_tk)


def scored_columns(ys, lens):
    n, W = ys.shape
    t0 = torch.ones(n, dtype=torch.long) if lens is None else lens
    return (torch.arange(1, W)[None, :] >= t0[:, None]) & (ys[:, 1:] != PAD)


# ------------------------------------------------------------------------------------------------- 1. the values
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_rule_against_plain_softmax_formulas(n, W, V):
    ys, lens, x, q, _ = dist_case(n, W, V, seed=100 * n + W)
    for pl in (lens, None):
        scored = scored_columns(ys, pl)
        lp, lq = torch.log_softmax(x, -1), torch.log_softmax(q, -1)
        p = torch.softmax(x, -1)
        want_h = torch.where(scored, -(p * lp).sum(-1), torch.zeros(()).double())
        want_k = torch.where(scored, (p * (lp - lq)).sum(-1), torch.zeros(()).double())
        te, en, tk, kl = dist_reference(x, ys, pl, PAD, prior_logits=q)
        assert te.dtype == torch.float64 and te.shape == (n, W) and en.shape == (n,) and tk.shape == (n, W)
        assert not te[:, 0].any() and not tk[:, 0].any()
        assert float((te[:, 1:] - want_h).abs().max()) <= 1e-12 and float((tk[:, 1:] - want_k).abs().max()) <= 1e-12
        assert float((en - want_h.sum(1)).abs().max()) <= 1e-12 * W
        assert float((kl - want_k.sum(1)).abs().max()) <= 1e-12 * W
        assert not te[:, 1:][~scored].any() and not tk[:, 1:][~scored].any()      # exact zeros off the scored columns
        assert bool((tk[:, 1:][scored] > 0).all()) and bool((te[:, 1:][scored] > 0).all())
        te2, en2, none_tk, none_kl = dist_reference(x, ys, pl, PAD)
        assert none_tk is None and none_kl is None and torch.equal(te2, te) and torch.equal(en2, en)
    if n > 1:
        assert float(dist_reference(x, ys, lens, PAD)[1][-1]) == 0                # t0 = W: nothing scored
    assert dist_reference(x.float(), ys, lens, PAD, prior_logits=q.float())[2].dtype == torch.float32
    with pytest.raises(ValueError):
        dist_reference(x[:, :-1], ys, lens, PAD)
    with pytest.raises(ValueError):
        dist_reference(x, ys, lens, PAD, prior_logits=q[:, :, :-1])


def test_a_zero_probability_contributes_exactly_nothing():
    n, W, V = 3, 8, 30
    ys, lens, x, q, _ = dist_case(n, W, V, seed=5, neg_inf=True)
    assert bool(scored_columns(ys, lens)[0, 0])
    te, en, tk, kl = dist_reference(x, ys, lens, PAD, prior_logits=q)
    assert all(bool(torch.isfinite(t).all()) for t in (te, en, tk, kl))
    keep = torch.arange(V) != V - 1                                               # the same row without that entry
    lp, lq = torch.log_softmax(x[0, 0, keep], -1), torch.log_softmax(q[0, 0, keep], -1)
    assert abs(float(te[0, 1]) + float((lp.exp() * lp).sum())) <= 1e-12
    assert abs(float(tk[0, 1]) - float((lp.exp() * (lp - lq)).sum())) <= 1e-12


def test_identities():
    """KL(p || p) is exactly 0 with an exactly zero gradient when the prior's logits ARE the agent's; uniform logits
    have entropy log V per scored token."""
    n, W, V = 4, 12, 31
    ys, lens, x, q, (g_e, g_te, g_k, g_tk) = dist_case(n, W, V, seed=3, neg_inf=True)
    te, en, tk, kl = dist_reference(x, ys, lens, PAD, prior_logits=x)
    assert not tk.any() and not kl.any()
    assert not dist_grad_reference(x, ys, lens, PAD, prior_logits=x, g_kl=g_k, g_token_kl=g_tk).any()
    u = torch.full((n, W - 1, V), 0.75, dtype=torch.float64)
    tokens = score_reference(u, ys, lens, PAD)[2]
    en = dist_reference(u, ys, lens, PAD)[1]
    assert int(tokens.sum()) > 0 and float((en - tokens.double() * math.log(V)).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------- 2. the gradient
WHICH = ["entropy", "token_entropy", "kl", "token_kl", "all"]


def pick(gs, which):
    """The weight tables of one parametrisation: (g_entropy, g_token_entropy, g_kl, g_token_kl), None where unused."""
    names = ["entropy", "token_entropy", "kl", "token_kl"]
    return tuple(g if which in (name, "all") else None for name, g in zip(names, gs))


@pytest.mark.parametrize("neg_inf", [False, True])
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_gradient_rule_against_autograd_through_dist_reference(n, W, V, which, neg_inf):
    ys, lens, x, q, gs = dist_case(n, W, V, seed=100 * n + W, neg_inf=neg_inf)
    g_e, g_te, g_k, g_tk = pick(gs, which)
    for pl in (lens, None):
        xa = x.clone().requires_grad_()
        qa = q.clone().requires_grad_()
        te, en, tk, kl = dist_reference(xa, ys, pl, PAD, prior_logits=qa)
        obj = torch.zeros((), dtype=torch.float64)
        for g, out in ((g_e, en), (g_te, te), (g_k, kl), (g_tk, tk)):
            if g is not None:
                obj = obj + (g * out).sum()
        want, = torch.autograd.grad(obj, xa, allow_unused=True)
        want = torch.zeros_like(x) if want is None else want
        got = dist_grad_reference(x, ys, pl, PAD, prior_logits=q, g_entropy=g_e, g_token_entropy=g_te, g_kl=g_k,
                                  g_token_kl=g_tk)
        assert got.dtype == torch.float64 and got.shape == x.shape and bool(torch.isfinite(want).all())
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (which, pl is None)
        assert not got[~scored_columns(ys, pl)].any()                             # exact zeros off the scored rows
        if neg_inf:
            assert float(got[0, 0, V - 1]) == 0.0 and float(want[0, 0, V - 1]) == 0.0
        if which in ("entropy", "token_entropy"):                                 # without a prior: the same rule
            assert torch.equal(dist_grad_reference(x, ys, pl, PAD, g_entropy=g_e, g_token_entropy=g_te), got)
    if n > 1:
        last = dist_grad_reference(x, ys, lens, PAD, prior_logits=q, g_entropy=gs[0], g_kl=gs[2])[-1]
        assert not last.any()                                                     # t0 = W: nothing scored
    with pytest.raises(ValueError):
        dist_grad_reference(x, ys, lens, PAD, g_kl=gs[2])                         # kl weights without a prior


def test_rule_never_looks_at_a_row_it_does_not_score():
    """NaN in both models' logits in every row that is not scored or whose two weights are 0 (a cancelling pair among
    them): values and gradients are finite, the same, and exactly 0 there; autograd through dist_reference stays finite
    too."""
    n, W, V = 4, 12, 31
    ys, lens, x, q, (g_e, g_te, g_k, g_tk) = dist_case(n, W, V, seed=9)
    g_e[1], g_k[1] = 0, 0
    g_te[1], g_tk[1] = 0, 0                                                       # every weight of row 1 is 0
    c = int(scored_columns(ys, lens)[0].nonzero()[0]) + 1                         # a scored column of row 0: both cancel
    g_te[0, c], g_tk[0, c] = -g_e[0], -g_k[0]
    scored = scored_columns(ys, lens)
    a, b = g_e[:, None] + g_te[:, 1:], g_k[:, None] + g_tk[:, 1:]
    live = scored & ((a != 0) | (b != 0))
    assert bool(scored[0, c - 1]) and not bool(live[0, c - 1])
    kw = dict(g_entropy=g_e, g_token_entropy=g_te, g_kl=g_k, g_token_kl=g_tk)
    want_v = dist_reference(x, ys, lens, PAD, prior_logits=q)
    want_g = dist_grad_reference(x, ys, lens, PAD, prior_logits=q, **kw)
    xs, qs = x.clone(), q.clone()
    xs[~scored], qs[~scored] = NAN, NAN
    got_v = dist_reference(xs, ys, lens, PAD, prior_logits=qs)
    assert all(bool(torch.isfinite(g).all()) and torch.equal(g, w) for g, w in zip(got_v, want_v))
    xa = xs.clone().requires_grad_()
    te, en, tk, kl = dist_reference(xa, ys, lens, PAD, prior_logits=qs)
    auto, = torch.autograd.grad((g_e * en).sum() + (g_tk * tk).sum(), xa)
    assert bool(torch.isfinite(auto).all()) and not auto[~scored].any()
    xs[~live], qs[~live] = NAN, NAN
    got_g = dist_grad_reference(xs, ys, lens, PAD, prior_logits=qs, **kw)
    assert bool(torch.isfinite(got_g).all()) and torch.equal(got_g, want_g) and not got_g[~live].any()
    # a row whose kl weight alone is 0 does not look at the PRIOR's row
    qs2 = q.clone()
    qs2[~(scored & (b != 0))] = NAN
    assert torch.equal(dist_grad_reference(x, ys, lens, PAD, prior_logits=qs2, **kw), want_g)
    assert dist_grad_reference(xs.float(), ys, lens, PAD, g_entropy=g_e).dtype == torch.float32


# --------------------------------------------------------------------------------------------------- 3. the loss
def test_regularised_loss_is_its_formula():
    g = torch.Generator().manual_seed(2)
    n, W = 7, 9
    logp = -torch.rand(n, generator=g) * 30
    reward = torch.rand(n, generator=g)
    entropy, kl = torch.rand(n, generator=g) * 20, torch.rand(n, generator=g) * 5
    zeros = torch.zeros(n, W)
    terms = PolicyTerms(logp, torch.ones(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), zeros, entropy, zeros,
                        kl, zeros, logp.clone())
    base = reinforce_loss(logp, reward)
    assert torch.equal(regularised_loss(terms, reward), base)
    want = base + (0.5 * kl.sum() - 0.05 * entropy.sum()) / n
    assert torch.allclose(regularised_loss(terms, reward, entropy_coef=0.05, kl_coef=0.5), want, rtol=1e-6, atol=0)
    want = reinforce_loss(logp, reward, baseline=0.25) - 0.3 * entropy.sum() / n
    assert torch.allclose(regularised_loss(terms, reward, baseline=0.25, entropy_coef=0.3), want, rtol=1e-6, atol=0)
    # gradients: the advantage into logp, the coefficients into the two sums
    lp, en, k = (t.clone().requires_grad_() for t in (logp, entropy, kl))
    regularised_loss(terms._replace(logp=lp, entropy=en, kl=k), reward, entropy_coef=0.05, kl_coef=0.5).backward()
    assert torch.allclose(lp.grad, -(reward - reward.mean()) / n, rtol=1e-6, atol=1e-9)
    assert torch.allclose(en.grad, torch.full((n,), -0.05 / n)) and torch.allclose(k.grad, torch.full((n,), 0.5 / n))
    no_prior = terms._replace(kl=None, token_kl=None, prior_logp=None)
    assert torch.allclose(regularised_loss(no_prior, reward, entropy_coef=0.05), base - 0.05 * entropy.sum() / n)
    with pytest.raises(ValueError, match="prior"):
        regularised_loss(no_prior, reward, kl_coef=0.5)


def test_reinforce_step_refuses_a_kl_coefficient_without_a_prior():
    class Untouched:                                     # any use of the sampler or the optimizer would raise
        model = None
    with pytest.raises(ValueError, match="prior"):
        reinforce_step(Untouched(), None, (), torch.zeros(3), kl_coef=0.1)


# ------------------------------------------------------------------------------------- the update step, oracle leg
def oracle_regularised_steps(mtype):
    """UPDATE_STEPS steps of torch.optim.Adam on the CPU oracle (tests/test_seq_logp_grad_host.update_case: rows,
    rewards, initial state) under regularised_loss with ENTROPY_COEF and KL_COEF, the prior a frozen copy of the initial
    state; logp from score_reference and the distribution terms from dist_reference on the oracle's teacher-forced
    logits, torch autograd.  Returns dict(loss, mean_entropy, mean_kl): one number per step, at that step's forward
    (entropy and KL per scored token), as reinforce_step reports them."""
    from oracle import gct_oracle as O
    cfg, state, t, reward = update_case(mtype)
    P = O.make_leaves(state)
    prior = {k: v.detach().clone() for k, v in state.items()}
    opt = O.make_adam(O.trainable(P, cfg), lr=UPDATE_LR)
    ys, nc = t["ys"], cfg["nconds"]
    trg = ys[:, :-1]
    trg_mask = O.get_trg_mask(trg, PAD, False, t["dconds"] if nc else None)
    args = (cfg, trg, t["z"], t["src_mask"], trg_mask, t["dconds"])
    with torch.no_grad():
        prior_logits = O.decode(prior, *args, train=False)
    out = dict(loss=[], mean_entropy=[], mean_kl=[])
    for _ in range(UPDATE_STEPS):
        logits = O.decode(P, *args, train=True)
        token_logp, logp, tokens, hits = score_reference(logits, ys, t["lens"], PAD)
        te, en, tk, kl = dist_reference(logits, ys, t["lens"], PAD, prior_logits=prior_logits)
        terms = PolicyTerms(logp, tokens, hits, token_logp, en, te, kl, tk, None)
        loss = regularised_loss(terms, reward, entropy_coef=ENTROPY_COEF, kl_coef=KL_COEF)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        out["loss"].append(float(loss.detach()))
        out["mean_entropy"].append(float(en.detach().sum() / tokens.sum()))
        out["mean_kl"].append(float(kl.detach().sum() / tokens.sum()))
    for k, v in prior.items():
        assert torch.equal(v, state[k]), k
    return out


_ORACLE = {}


def oracle_regularised_run(mtype):
    """oracle_regularised_steps, computed once per process and shared by the host and the device test."""
    if mtype not in _ORACLE:
        _ORACLE[mtype] = oracle_regularised_steps(mtype)
    return _ORACLE[mtype]


@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_oracle_kl_starts_at_zero_and_grows(mtype):
    run = oracle_regularised_run(mtype)
    print(f"{mtype}: oracle regularised steps {({k: [round(x, 7) for x in v] for k, v in run.items()})}")
    assert all(len(v) == UPDATE_STEPS for v in run.values())
    assert run["mean_kl"][0] == 0.0 and all(v > 0 for v in run["mean_kl"][1:]), run["mean_kl"]
    assert all(0 < v < math.log(31) for v in run["mean_entropy"])
    assert all(math.isfinite(v) for v in run["loss"])
