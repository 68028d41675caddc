"""Stochastic beam search, the host statement of the rules (decode.sbs_step_reference, sbs_importance_weights, StepPlan's
SBEAM): step invariants on random states, a toy model whose sequence distribution is known exactly -- distinct beams,
the first beam an ordinary sample, the importance-weighted estimator unbiased -- and the near-tie share of the cases
tests/test_sbs_gpu.py runs the kernel on.  No GPU, no native library call."""
import math

import pytest
import torch

from gct_plus_amd.decode import (GRAMMAR, MIXED, SBEAM, STREAM, UNIFORM, StepPlan, beam_log_softmax,
                                 sbs_importance_weights, sbs_init, sbs_step_reference)
from tests import sbs_ref

PAD, EOS = 1, 3
CHI2_2DOF_P1E3 = 13.815510557964274          # chi-square quantile, 2 degrees of freedom, upper tail 1e-3: -2 ln(1e-3)


def gumbel(shape, g):
    return -torch.log(-torch.log(torch.rand(shape, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)))


# ------------------------------------------------------------------------------------------- step invariants
@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("V", [5, 30, 300])
def test_step_invariants(k, V):
    g = torch.Generator().manual_seed(31 * k + V)
    n = 12
    logits = torch.randn(n * k, V, generator=g, dtype=torch.float64) * 3
    logits[torch.rand(n * k, V, generator=g) < 0.25] = -math.inf
    logits[:, 0] = 0.0                                         # (every row keeps a finite token)
    scores = -torch.rand(n, k, generator=g, dtype=torch.float64) * 20
    gum = scores + gumbel((n, k), g)
    order = torch.sort(gum, dim=1, descending=True).indices
    scores, gum = scores.gather(1, order), gum.gather(1, order)
    fin = torch.rand(n, k, generator=g) < 0.3
    lens = torch.randint(1, 15, (n, k), generator=g)
    s0, g0, f0, l0 = sbs_init(1, k)
    scores[0], gum[0], fin[0], lens[0] = s0[0].double(), g0[0].double(), f0[0], l0[0]
    logp = beam_log_softmax(logits)
    noise = gumbel((n * k, V), g)
    parent, tok, sc2, gum2, fin2, len2 = sbs_step_reference(scores, gum, fin, lens, logp, noise, k, PAD, EOS)
    real = gum2 > -math.inf                                    # (a slot no candidate was left for is a beam at -inf)
    assert not torch.isnan(gum2).any() and not torch.isnan(sc2).any()
    pg = gum.gather(1, parent)
    assert bool((gum2[real] <= pg[real]).all())                # every child's Gumbel value <= its parent's
    assert bool((gum2[:, :-1] >= gum2[:, 1:]).all())           # children are sorted
    phi = scores.unsqueeze(-1) + logp.view(n, k, V)
    for s in range(n):
        for b in range(k):
            kids = [c for c in range(k) if real[s, c] and parent[s, c] == b]
            if not kids:
                continue
            best = kids[0]                                     # sorted: the first is the parent's best child
            assert gum2[s, best].item() == gum[s, b].item()    # bit for bit
        for c in range(k):
            b, t = int(parent[s, c]), int(tok[s, c])
            if not real[s, c]:
                assert sc2[s, c] == -math.inf and bool(fin2[s, c]) and t == PAD
                continue
            if fin[s, b]:                                      # a frozen beam passes through unchanged
                assert t == PAD and sc2[s, c] == scores[s, b] and gum2[s, c] == gum[s, b]
                assert bool(fin2[s, c]) and len2[s, c] == lens[s, b]
            else:
                assert phi[s, b, t] > -math.inf                # -inf logits are never chosen
                assert sc2[s, c] == phi[s, b, t] and len2[s, c] == lens[s, b] + 1
                assert bool(fin2[s, c]) == (t == EOS)
        # a frozen beam appears at most once, a (parent, token) pair at most once
        pairs = [(int(parent[s, c]), int(tok[s, c])) for c in range(k) if real[s, c]]
        assert len(set(pairs)) == len(pairs)
    # the first expansion offers beam 0 only
    assert bool((parent[0][real[0]] == 0).all())


# ------------------------------------------------------------------------------------------- the toy model
TOY_V, TOY_PAD, TOY_EOS, TOY_STEPS, TOY_K = 4, 0, 1, 4, 5
TOY_FIRST = (0.020, 0.910, 0.070)                               # p(<eos>), p(token 2), p(token 3) after the empty prefix


def toy_table():
    """log-probabilities [4^TOY_STEPS codes, V] of the next token after each prefix (code: the prefix's tokens as base-4
    digits behind a leading 1); <pad> is never generated."""
    g = torch.Generator().manual_seed(2019)
    ncode = 2 * TOY_V ** TOY_STEPS
    p = torch.rand(ncode, 3, generator=g, dtype=torch.float64) + 0.05
    p[1] = torch.tensor(TOY_FIRST, dtype=torch.float64)        # code 1: the empty prefix
    p = p / p.sum(1, keepdim=True)
    logp = torch.full((ncode, TOY_V), -math.inf, dtype=torch.float64)
    logp[:, 1:] = torch.log(p)
    return logp


def toy_enumerate(table):
    """{code: probability} of every sequence the toy can produce in TOY_STEPS steps (ended by <eos>, or cut)."""
    out = {}

    def walk(code, lp, depth):
        if depth == TOY_STEPS:
            out[code] = math.exp(lp)
            return
        for t in (1, 2, 3):
            c = code * TOY_V + t
            if t == TOY_EOS:
                out[c] = math.exp(lp + table[code, t].item())
            else:
                walk(c, lp + table[code, t].item(), depth + 1)
    walk(1, 0.0, 0)
    return out


def toy_run(n, seed):
    """n independent samples ("seeds": each has its own variates) of TOY_K beams, the root's Gumbel value drawn:
    (codes [n, k] of the sequences, scores, gumbels, first tokens [n, k])."""
    table = toy_table()
    g = torch.Generator().manual_seed(seed)
    k = TOY_K
    scores, gum, fin, lens = (t.double() if t.is_floating_point() else t for t in sbs_init(n, k))
    gum[:, 0] = gumbel((n,), g)                                 # (sbs_init(root=) in float64)
    codes = torch.ones(n, k, dtype=torch.int64)
    first = None
    for step in range(TOY_STEPS):
        logp = table[codes.view(-1)]
        parent, tok, scores, gum, fin2, lens = sbs_step_reference(scores, gum, fin, lens, logp, gumbel((n * k, TOY_V), g),
                                                                  k, TOY_PAD, TOY_EOS)
        pc, pf = codes.gather(1, parent), fin.gather(1, parent)
        codes = torch.where(pf, pc, pc * TOY_V + tok)
        fin = fin2
        first = tok if first is None else first.gather(1, parent)
        assert bool((gum[:, :-1] >= gum[:, 1:]).all())          # the Gumbel values stay sorted
    return codes, scores, gum, first


def test_toy_beams_are_distinct_and_scored():
    codes, scores, gum, _ = toy_run(300, seed=0)
    prob = toy_enumerate(toy_table())
    assert len(prob) >= TOY_K and abs(sum(prob.values()) - 1.0) < 1e-12
    dup = sum(TOY_K - len(set(row)) for row in codes.tolist())
    assert dup == 0                                            # a sample without replacement: zero duplicates in all
    want = torch.tensor([[math.log(prob[c]) for c in row] for row in codes.tolist()], dtype=torch.float64)
    torch.testing.assert_close(scores, want, rtol=0, atol=1e-12)


def chi_square(counts, probs):
    total = sum(counts)
    return sum((c - total * p) ** 2 / (total * p) for c, p in zip(counts, probs))


def test_first_beam_is_an_ordinary_sample():
    _, _, _, first = toy_run(4000, seed=1)
    counts = [int((first[:, 0] == t).sum()) for t in (1, 2, 3)]
    print("first-token frequencies", [c / 4000 for c in counts], "against", TOY_FIRST)
    assert sum(counts) == 4000
    assert chi_square(counts, TOY_FIRST) < CHI2_2DOF_P1E3


def test_importance_weights_are_unbiased_on_the_toy():
    codes, scores, gum, _ = toy_run(4000, seed=2)
    prob = toy_enumerate(toy_table())
    f = {c: math.sin(0.37 * c) + 0.01 * (c % 7) for c in prob}             # a fixed table over the toy's sequences
    exact = sum(prob[c] * f[c] for c in prob)
    w, wn = sbs_importance_weights(scores, gum)
    fv = torch.tensor([[f[c] for c in row] for row in codes.tolist()], dtype=torch.float64)
    est = (w * fv).sum(1)
    se = est.std(unbiased=True).item() / math.sqrt(est.numel())
    print(f"estimator mean {est.mean().item():.5f} exact {exact:.5f} standard error {se:.5f}")
    assert abs(est.mean().item() - exact) <= 4 * se
    assert bool((w[:, -1] == 0).all()) and bool((w[:, :-1] > 0).all())
    torch.testing.assert_close(wn.sum(1), torch.ones(4000, dtype=torch.float64))
    torch.testing.assert_close(wn, w / w.sum(1, keepdim=True))


def test_init_and_root():
    from gct_plus_amd.decode import sbs_root_gumbels
    scores, gum, fin, lens = sbs_init(3, 4)
    want = torch.tensor([[0.0] + [-math.inf] * 3] * 3)
    assert torch.equal(scores, want) and torch.equal(gum, want) and scores.dtype == torch.float32
    assert not fin.any() and fin.dtype == torch.bool and not lens.any() and lens.dtype == torch.int64
    root = sbs_root_gumbels(3, seed=11)
    assert root.shape == (3,) and root.dtype == torch.float32 and bool(torch.isfinite(root).all())
    assert torch.equal(root, sbs_root_gumbels(5, seed=11)[:3]) and not torch.equal(root, sbs_root_gumbels(3, seed=12))
    scores, gum, _, _ = sbs_init(3, 4, root=root)
    assert torch.equal(scores, want) and torch.equal(gum[:, 0], root) and torch.equal(gum[:, 1:], want[:, 1:])
    big = sbs_root_gumbels(20000, seed=0).double()              # Gumbel(0): mean Euler's constant, variance pi^2 / 6
    assert abs(big.mean().item() - 0.5772156649) < 4 * math.sqrt(math.pi ** 2 / 6 / 20000)


def test_importance_weights_refuse_k_one_and_bad_shapes():
    with pytest.raises(ValueError, match="k = 1"):
        sbs_importance_weights(torch.zeros(3, 1), torch.zeros(3, 1))
    with pytest.raises(ValueError):
        sbs_importance_weights(torch.zeros(3, 2), torch.zeros(3, 3))
    assert "unbiased" in sbs_importance_weights.__doc__ and "ValueError" in sbs_importance_weights.__doc__


def test_importance_weights_formula():
    scores = torch.tensor([[-0.5, -2.0, -3.0]], dtype=torch.float64)
    gum = torch.tensor([[0.3, -1.0, -1.5]], dtype=torch.float64)
    w, _ = sbs_importance_weights(scores, gum)
    want = [math.exp(s) / (1.0 - math.exp(-math.exp(s + 1.5))) for s in (-0.5, -2.0)] + [0.0]
    torch.testing.assert_close(w, torch.tensor([want], dtype=torch.float64))


# ------------------------------------------------------------------------------------------- StepPlan
def test_step_plan_sbeam():
    assert SBEAM == "sbeam" and StepPlan(SBEAM).key == "sbeam"
    for kw in (dict(layout=MIXED), dict(layout=STREAM), dict(grammar=True), dict(logp=True)):
        with pytest.raises(ValueError, match="stochastic beam step"):
            StepPlan(SBEAM, **kw)
    assert StepPlan("beam").key == "beam" and StepPlan(1).key == 1
    assert StepPlan(1, UNIFORM, True).key == (1, UNIFORM, GRAMMAR)


# ------------------------------------------------------------------------------------------- near-tie share
def test_kernel_cases_rarely_sit_on_a_near_tie():
    """A condition on the cases of tests/test_sbs_gpu.py::test_select_gumbel_matches_reference, checked on the fp64 rules
    alone.  GAP = 1e-3: a plain fp32 restatement of the g~ formula differed from fp64 by at most 1.7e-4 on such inputs,
    and GAP is more than twice that figure.  A sample counts when ANY two adjacent values among its k+1 best lie
    closer than GAP (the k-th and (k+1)-th, which the rule names, and also pairs inside the k best, whose order may
    swap): a superset of the rule's count, held to the same 10 %."""
    counted = total = 0
    for k, V in sbs_ref.kernel_cases():
        case = sbs_ref.kernel_case(k, V, PAD, EOS)
        _, top, _ = sbs_ref.kernel_reference(case, k, PAD, EOS)
        tie = sbs_ref.near_tie(top)
        counted += int(tie.sum())
        total += tie.numel()
    print(f"near-tie samples: {counted} of {total}")
    assert total == 5 * len(sbs_ref.kernel_cases())
    assert counted <= 0.10 * total
