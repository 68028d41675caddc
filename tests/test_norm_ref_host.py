"""tests/norm_ref.py on the CPU: the bounds hold, with a margin of 2 x, for an fp32 restatement of the Norm kernels;
every mutant of that restatement breaks some bound by >= 10 x on inputs that tests/test_norm_gpu.py uses; unit randn
rows -- all that the older Norm tests feed the kernels -- cannot see the two eps mistakes; and the reference itself
reproduces the known answer and passes gradcheck."""
import itertools

import pytest
import torch

from tests import norm_ref as N

MUTANT_WIDTHS = (4, 260, 2048)                                 # a subset of N.WIDTHS keeps the 8 mutants quick
CASES = list(itertools.product(N.FAMILIES, N.WIDTHS, N.EPSES, (False, True)))


def _ratios(name, d, eps, with_dres, mutant=None):
    p, ref, bnd = N.case(name, N.ROWS, d, eps, with_dres)
    return N.ratios(N.kernel32(p, mutant), ref, bnd)


def test_families_stay_in_the_normal_range():
    tiny, huge = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).max
    for name in N.FAMILIES:
        x = N.family_x(name, N.ROWS, 2048).double()
        c = x - x.mean(-1, keepdim=True)
        for sums in ((x * x).sum(-1), (c * c).sum(-1)):          # a square that underflows is < 1e-10 of its row's sum
            assert float(sums.min()) > 1e10 * tiny and float(sums.max()) < 1e-4 * huge, name
    x = N.family_x("mixed", N.ROWS, 512)
    assert torch.equal(x[1::7], N.family_x("offset", N.ROWS, 512)[1::7])      # row i is family i % 7's row i
    sd = N.family_x("half-1e-5", N.ROWS, 512).double().std(-1)
    assert 0.8e-5 < float(sd.min()) and float(sd.max()) < 1.2e-5               # survives the rounding of 0.5 + 1e-5 z


def test_the_bounds_hold_for_the_restated_kernel_with_a_margin_of_two():
    worst = {q: (0.0, None) for q in N.QUANTITIES}
    for name, d, eps, with_dres in CASES:
        for q, v in _ratios(name, d, eps, with_dres).items():
            if v > worst[q][0]:
                worst[q] = (v, (name, d, eps, with_dres))
    for q, (v, where) in worst.items():
        print(f"[norm_ref] K_{q} = {N.K[q]:g}: worst error / bound {v:.3f} at {where}")
    for q, (v, where) in worst.items():
        assert v <= 0.5, f"{q}: the fp32 restatement is at {v:.3f} x the bound at {where}"


@pytest.mark.parametrize("mutant", N.MUTANTS)
def test_every_mutant_breaks_a_bound_by_ten(mutant):
    best = (0.0, None)
    for name, d, eps, with_dres in itertools.product(N.FAMILIES, MUTANT_WIDTHS, N.EPSES, (False, True)):
        for q, v in _ratios(name, d, eps, with_dres, mutant).items():
            if v > best[0]:
                best = (v, (q, name, d, eps, with_dres))
    print(f"[norm_ref] {mutant}: {best[0]:.3g} x the bound at {best[1]}")
    assert best[0] >= 10.0, f"{mutant} stays within {best[0]:.2f} x every bound"


@pytest.mark.parametrize("mutant", N.EPS_MUTANTS)
def test_unit_rows_cannot_see_the_eps_mistakes(mutant):
    """Why the other families exist.  On unit randn rows at the default eps the two eps mistakes stay inside the bounds
    of everything the older tests compare (y, dx, dalpha, dbias) at every width from 12 up, tight as these bounds are
    next to the flat 1e-5; the small-sigma families put the same mistakes >= 1e4 x outside.  (rstd itself, which nothing
    compared before, shows the forward mistake at 1.3 x its bound, and four-element rows, whose sigma can be 0.1, at
    8 x: neither is what the older tests look at.)"""
    seen = ("y", "dx", "dalpha", "dbias")
    for d in N.WIDTHS[1:]:
        r = _ratios("unit", d, 1e-6, True, mutant)
        assert max(r[q] for q in seen) <= 1.0, (d, r)
    far = max(max(_ratios(name, d, 1e-6, True, mutant).values()) for name in ("sigma-eps", "sigma-below-eps")
              for d in MUTANT_WIDTHS)
    assert far >= 1e4, far


def test_one_pass_variance_is_invisible_on_unit_rows():
    for d in MUTANT_WIDTHS:
        assert max(_ratios("unit", d, 1e-6, True, "fwd-one-pass-variance").values()) <= 1.0
    assert max(_ratios("offset", 260, 1e-6, True, "fwd-one-pass-variance").values()) >= 100.0


def test_the_reference_reproduces_the_known_answer():
    p = N.Problem(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), torch.ones(4), torch.zeros(4), torch.ones(1, 4), None, N.eps32(1e-6))
    ref = N.reference(p)
    want = torch.tensor([[-1.161894, -0.387298, 0.387298, 1.161894]], dtype=torch.float64)      # Norm(4)([1, 2, 3, 4])
    assert float((ref.y - want).abs().max()) < 1e-6
    assert float(ref.mean[0]) == 2.5 and abs(float(ref.rstd[0]) - 1.0 / ((5.0 / 3.0) ** 0.5 + p.eps)) < 1e-15


def test_the_reference_passes_gradcheck_and_matches_its_closed_form():
    def norm(x, a, b):
        return a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-2) + b
    g = torch.Generator().manual_seed(0)
    x, a, b = (torch.randn(s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((3, 8), (8,), (8,)))
    assert torch.autograd.gradcheck(norm, (x, a, b), eps=1e-6, atol=1e-7)
    # the kernels' closed form of dx, evaluated in fp64, is the autograd gradient
    p, ref, _ = N.case("unit", N.ROWS, 12, 1e-2, True)
    X, A, DY = p.x.double(), p.alpha.double(), p.dy.double()
    c = X - X.mean(-1, keepdim=True)
    sigma = c.pow(2).sum(-1, keepdim=True).div(11).sqrt()
    r = 1.0 / (sigma + p.eps)
    G = DY * A
    dx = r * (G - G.mean(-1, keepdim=True)) - c * (G * c).sum(-1, keepdim=True) * r * r / (sigma * 11) + p.dres.double()
    assert float((dx - ref.dx).abs().max()) < 1e-12
    assert float(((DY * c * r).sum(0) - ref.dalpha).abs().max()) < 1e-12 and torch.equal(DY.sum(0), ref.dbias)


def test_addends_follow_the_launch_geometry():
    assert [N.norm_blocks(r) for r in (0, 1, 4, 5, 37, 4096, 4097, 32773)] == [1, 1, 1, 2, 10, 1024, 1024, 1024]
    assert N.addends(37) == 4 + 4 + 10 and N.addends(32773) == 12 + 4 + 1024 and N.addends(1) == 4 + 4 + 1
