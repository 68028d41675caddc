"""Per-step sampling statistics on the host: the rule (decode.step_stats_reference) on distributions whose answer is
known, the fp32 restatement of gct_step_stats against the bounds of tests/step_stats_ref.py and the one-mistake mutants
those bounds must catch, and the plumbing -- StepPlan keys, the samplers' refusal, behaviour_weights, the weighted
REINFORCE loss and step.

Measured margins (seeds 0 .. 5 at V = 5 / 30 / 130 / 1024, 6 rows each, CPU numpy; error / bound, worst over rows):
  fp32 restatement   q given: model_entropy 0.027, behaviour_logp 0.455, behaviour_entropy 0.084, behaviour_kl 0.053;
                     q = pi:  0.027 / 0.136 / 0.027 / exact;  greedy: 0.027 / exact / exact / 0.136      (asked: <= 0.5)
                     (behaviour_logp of a given q is ONE logf: its bound is two ulp, numpy's fp32 log uses 0.9 of one)
  mutants, the least error / bound over all rows in the output that shows the mistake:
                     entropy_of_pi 2.1e5, logp_of_pi 4.3e4, unnormalised_q 7.3e2, log2 5.4e4; pad_not_zeroed: a bound
                     of 0 against values of order 1                                                      (asked: > 1)
"""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd.decode import (BEAM, FILTERED, GRAMMAR, LOGP, MIXED, SBEAM, STATS, STREAM, UNIFORM, StepPlan, StepStats,
                                 step_stats_reference)
from gct_plus_amd.Train.finetune import behaviour_weights, reinforce_loss, reinforce_step
from tests.step_stats_ref import MUTANTS, NAMES, make_case, step_stats_bounds, step_stats_f32, step_stats_ref

PAD = 0
SHAPES = [(6, 5), (6, 30), (6, 130), (6, 1024)]
SEEDS = range(6)


def rule(logits, probs, tok, pad_id=PAD, greedy=False):
    out = step_stats_reference(torch.as_tensor(logits), None if probs is None else torch.as_tensor(probs),
                               torch.as_tensor(tok), pad_id, greedy)
    return np.stack([t.numpy() for t in out])


# ------------------------------------------------------------------------------------------------ 1. the rule
def test_uniform_pi_has_entropy_log_v():
    for V in (1, 2, 7, 64, 1000):
        me, bl, be, kl = rule(np.full((2, V), 3.25), None, [V - 1, V - 1], pad_id=V)
        assert np.allclose(me, math.log(V), atol=1e-12) and np.allclose(bl, -math.log(V), atol=1e-12)
        assert np.array_equal(be, me) and np.array_equal(kl, np.zeros(2))


def test_one_hot_q_and_greedy():
    x, _, _, tok = make_case(5, 30, 1, PAD, mode="greedy")
    lpi = torch.log_softmax(torch.as_tensor(x).double(), -1).numpy()
    q = np.zeros((5, 30), dtype=np.float32)
    q[np.arange(5), tok] = 1.0
    for out in (rule(x, q, tok), rule(x, None, tok, greedy=True), rule(x, make_case(5, 30, 2)[1], tok, greedy=True)):
        assert np.array_equal(out[1], np.zeros(5)) and np.array_equal(out[2], np.zeros(5))       # log 1, H(one-hot)
        assert np.allclose(out[3], -lpi[np.arange(5), tok], atol=1e-12)                           # KL = -log pi(tok)
        assert np.allclose(out[0], -(np.exp(lpi) * lpi).sum(-1), atol=1e-12)


def test_q_equal_to_pi_has_kl_exactly_zero():
    x, _, _, tok = make_case(7, 130, 3, PAD, mode="none")
    me, bl, be, kl = rule(x, None, tok)
    lpi = torch.log_softmax(torch.as_tensor(x).double(), -1).numpy()
    assert np.array_equal(kl, np.zeros(7)) and np.array_equal(be, me)
    assert np.allclose(bl, lpi[np.arange(7), tok], atol=1e-12)
    # pi handed in as probs: the same numbers to fp64 rounding, the KL no longer exact
    out = rule(x, np.exp(lpi), tok)
    assert np.allclose(out, np.stack([me, bl, be, kl]), atol=1e-12)


def test_q_with_zeros_and_a_pad_row():
    x = np.array([[0.0, 1.0, 2.0, -1.0], [0.5, 0.5, 0.5, 0.5], [3.0, 1.0, 0.0, 2.0]])
    q = np.array([[0.0, 0.25, 0.75, 0.0], [0.0, 0.0, 1.0, 0.0], [0.5, 0.5, 0.0, 0.0]])
    tok = [2, 2, PAD]                                                              # row 2 has finished
    me, bl, be, kl = rule(x, q, tok)
    lpi = x - np.log(np.exp(x).sum(-1, keepdims=True))
    assert math.isclose(be[0], -(0.25 * math.log(0.25) + 0.75 * math.log(0.75)), abs_tol=1e-12)
    assert math.isclose(kl[0], 0.25 * (math.log(0.25) - lpi[0, 1]) + 0.75 * (math.log(0.75) - lpi[0, 2]), abs_tol=1e-12)
    assert math.isclose(bl[0], math.log(0.75), abs_tol=1e-12)
    assert be[1] == 0 and bl[1] == 0 and math.isclose(kl[1], math.log(4), abs_tol=1e-12)
    assert me[2] == bl[2] == be[2] == kl[2] == 0
    assert np.isfinite(np.stack([me, bl, be, kl])).all()                            # a q = 0 term adds 0, never a NaN
    # a -inf logit (a token with pi = 0) adds 0 to the model's entropy
    me2 = rule(np.array([[0.0, -np.inf, 0.0]]), None, [2])[0]
    assert math.isclose(me2[0], math.log(2), abs_tol=1e-12)
    assert rule(x, np.tile([[0.0, 1.0, 0.0, 0.0]], (3, 1)), [2, 2, 1])[1][0] == -np.inf      # q(tok) = 0
    for bad in (dict(logits=np.zeros(3), probs=None, tok=[0]), dict(logits=x, probs=q[:2], tok=tok),
                dict(logits=x, probs=None, tok=[1, 2])):
        with pytest.raises(ValueError):
            step_stats_reference(torch.as_tensor(bad["logits"]), None if bad["probs"] is None else
                                 torch.as_tensor(bad["probs"]), bad["tok"], PAD)


def test_numpy_reference_agrees_with_the_rule():
    for mode in ("probs", "none", "greedy"):
        x, q, _, tok = make_case(6, 65, 4, PAD, mode)
        tok[3] = PAD
        a, b = rule(x, q, tok, greedy=mode == "greedy"), step_stats_ref(x, q, tok, PAD, greedy=mode == "greedy")
        assert np.allclose(a, b, atol=1e-12, rtol=0) and (a[:, 3] == 0).all()


# --------------------------------------------------------------------------------- 2. the restatement, the mutants
def ratio(got, ref, bound):
    """error / bound per entry; a bound of 0 asks for the exact value (0 where it holds, inf where it does not)."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


@pytest.mark.parametrize("mode", ["probs", "none", "greedy"])
def test_fp32_restatement_stays_under_half_of_every_bound(mode):
    worst = np.zeros(4)
    for n, V in SHAPES:
        for seed in SEEDS:
            x, q, _, tok = make_case(n, V, seed, PAD, mode)
            tok[n - 1] = PAD                                                       # a finished row
            kw = dict(greedy=mode == "greedy")
            r = ratio(step_stats_f32(x, q, tok, PAD, **kw), step_stats_ref(x, q, tok, PAD, **kw),
                      step_stats_bounds(x, q, tok, PAD, **kw))
            worst = np.maximum(worst, r.max(-1))
    print(f"restatement ({mode}): worst error / bound per output {dict(zip(NAMES, np.round(worst, 4)))}")
    assert (worst <= 0.5).all()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    least = math.inf
    for n, V in SHAPES:
        for seed in SEEDS:
            x, q, w, tok = make_case(n, V, seed, PAD, "probs")
            if mutant == "pad_not_zeroed":
                tok[:] = PAD
            given = w if mutant == "unnormalised_q" else q                         # the weights before their own sum
            r = ratio(step_stats_f32(x, given, tok, PAD, mutant=mutant), step_stats_ref(x, q, tok, PAD),
                      step_stats_bounds(x, q, tok, PAD))
            assert (r.max(0) > 1).all(), (mutant, V, seed)                         # every row gives the mutant away
            least = min(least, float(r.max(0).min()))
    print(f"mutant {mutant}: error / bound at least {least:.3g} in the output that shows it")


# -------------------------------------------------------------------------------------------------- 3. plumbing
def test_step_plan_keys_with_stats():
    for m in (0, 1, FILTERED):
        assert StepPlan(m, UNIFORM, stats=True).key == (m, UNIFORM, STATS)
        for L in (UNIFORM, MIXED, STREAM):
            assert StepPlan(m, L, False, False, True).key == (m, L, STATS)
            assert StepPlan(m, L, True, False, True).key == (m, L, GRAMMAR, STATS)
            assert StepPlan(m, L, False, True, True).key == (m, L, LOGP, STATS)
            assert StepPlan(m, L, True, True, True).key == (m, L, GRAMMAR, LOGP, STATS)
            # plans without stats keep their keys
            assert StepPlan(m, L, True, True, False).key == StepPlan(m, L, True, True).key == (m, L, GRAMMAR, LOGP)
        assert StepPlan(m, stats=False).key == StepPlan(m).key == m
    keys = {StepPlan(m, L, g, lp, s).key for m in (0, 1, FILTERED) for L in (UNIFORM, MIXED, STREAM)
            for g in (False, True) for lp in (False, True) for s in (False, True)}
    assert len(keys) == 3 * 3 * 8
    assert STATS == "stats" and StepPlan().stats is False


def test_beam_units_refuse_stats():
    for sel in (BEAM, SBEAM):
        with pytest.raises(ValueError, match="step statistics"):
            StepPlan(sel, stats=True)


def test_samplers_refuse_stats_with_beam_search():
    from gct_plus_amd.Inference.sampling_tool import Sampling

    class Out:
        weight = torch.zeros(30, 4)

    class Model:
        out = Out()

    for algo in ("beam", "stochastic_beam"):
        with pytest.raises(ValueError, match="with_stats is not supported with decode_algo"):
            Sampling(Model(), None, None, 8, decode_algo=algo, with_stats=True)


def test_step_stats_tuple_fields():
    assert StepStats._fields == NAMES + ("behaviour_logp_sum",)


def test_behaviour_weights():
    lp, lq = torch.tensor([-3.0, -2.0, -7.5, -1.0]), torch.tensor([-2.5, -2.0, -9.0, -0.25])
    rho = behaviour_weights(lp, lq)
    assert rho.dtype == torch.float32 and torch.equal(rho, torch.exp(lp - lq)) and float(rho[1]) == 1.0
    cut = behaviour_weights(lp, lq, clip=1.5)
    assert torch.equal(cut, torch.exp(lp - lq).clamp(max=1.5)) and float(cut[2]) == 1.5 and float(cut[0]) == float(rho[0])
    assert not behaviour_weights(lp.requires_grad_(), lq).requires_grad
    lp = lp.detach()
    for a, b, kw in ((lp, lq[:3], {}), (lp.view(2, 2), lq.view(2, 2), {}), (lp, lq, dict(clip=0)),
                     (lp, lq, dict(clip=-1.0)), (lp, lq, dict(clip=math.inf)), (lp, lq, dict(clip="x")),
                     (lp, lq, dict(clip=True)), (torch.tensor([0.0, math.nan]), lq[:2], {}),
                     (lp[:2], torch.tensor([-math.inf, 0.0]), {})):
        with pytest.raises(ValueError):
            behaviour_weights(a, b, **kw)


def test_reinforce_loss_weight_paths():
    g = torch.Generator().manual_seed(0)
    logp, reward, w = -torch.rand(6, generator=g) * 9, torch.randn(6, generator=g), torch.rand(6, generator=g) * 2
    for baseline in ("mean", None, 0.25, torch.randn(6, generator=g)):
        b = 0.0 if baseline is None else reward.mean() if isinstance(baseline, str) else torch.as_tensor(baseline)
        plain = reinforce_loss(logp, reward, baseline)
        assert torch.equal(plain, -((reward - b) * logp).sum() / 6)                 # weight=None: today's expression
        assert torch.equal(reinforce_loss(logp, reward, baseline, weight=None), plain)
        assert torch.equal(reinforce_loss(logp, reward, baseline, weight=torch.ones(6)), plain)
        assert torch.equal(reinforce_loss(logp, reward, baseline, weight=w), -((w * (reward - b)) * logp).sum() / 6)
    lp = logp.clone().requires_grad_()
    reinforce_loss(lp, reward, "mean", weight=w).backward()                         # the weight scales the advantage
    assert torch.allclose(lp.grad, -(w * (reward - reward.mean())) / 6, atol=0, rtol=1e-6)
    for bad in (torch.ones(5), torch.tensor([1.0, 1, 1, 1, 1, -0.5]), torch.tensor([1.0, 1, 1, 1, 1, math.inf])):
        with pytest.raises(ValueError):
            reinforce_loss(logp, reward, "mean", weight=bad)


class StubSampler:
    """What reinforce_step uses of a sampler (test_ppo_host.py's stub, with a parameter to update): logp(*rows) scores
    the rows with one weight vector."""
    device = "cpu"

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.theta = torch.nn.Parameter(torch.linspace(-1, 1, 5))

    class Scores:
        def __init__(self, logp, tokens):
            self.logp, self.tokens = logp, tokens

    def __init__(self):
        self.model = self.Model()

    def logp(self, feats, ys):
        return self.Scores(-(feats @ self.model.theta) ** 2, (ys != PAD).sum(1).int())


def run_stub_step(weight, **kw):
    torch.manual_seed(3)
    s = StubSampler()
    opt = torch.optim.SGD(s.model.parameters(), lr=0.1)
    rows = (torch.randn(4, 5), torch.randint(0, 9, (4, 7)))
    out = reinforce_step(s, opt, rows, torch.tensor([1.0, -0.5, 2.0, 0.25]), weight=weight, **kw)
    assert not s.model.training
    return out, s.model.theta.detach().clone()


def test_reinforce_step_weight_paths():
    base, theta = run_stub_step(None)
    assert set(base) == {"loss", "mean_reward", "mean_logp", "tokens"}              # today's dict
    ones, theta1 = run_stub_step(torch.ones(4))
    assert torch.equal(theta, theta1) and {k: ones[k] for k in base} == base
    assert ones["weight_mean"] == 1.0 and ones["weight_max"] == 1.0
    w = torch.tensor([0.5, 2.0, 0.0, 1.25])
    got, theta_w = run_stub_step(w, max_grad_norm=1e6)
    assert not torch.equal(theta_w, theta) and got["weight_mean"] == float(w.mean()) and got["weight_max"] == 2.0
    assert "grad_norm" in got and got["clipped"] is False                          # the clip's numbers keep their places
    for bad in (torch.ones(3), torch.tensor([1.0, 1.0, math.nan, 1.0]), torch.tensor([1.0, -1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            run_stub_step(bad)


def test_ppo_update_refuses_a_bad_weight_before_device_work():
    from gct_plus_amd.Train.finetune import ppo_update

    class Untouched:
        model = None
    rows = (None, torch.zeros(3, 5, dtype=torch.long))
    for bad in (torch.ones(4), torch.tensor([1.0, math.inf, 1.0]), torch.tensor([1.0, -2.0, 1.0])):
        with pytest.raises(ValueError, match="weights"):
            ppo_update(Untouched(), None, rows, torch.zeros(3), weight=bad)
