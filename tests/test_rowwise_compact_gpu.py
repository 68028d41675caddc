"""gct_norm_bwd under a quad map (with src_rows and with drop_out), gct_dropout_bwd under a quad map, and the Norm
forward on zero-variance rows (compact buffers carry all-zero gap rows).

A compact row is one wave's arithmetic on that row's inputs only, so the rows of the live quads must equal the dense
call's rows bit for bit; dalpha / dbias are sums over rows in another order and keep test_norm's fp64 tolerance."""
import math

import pytest
import torch

from tests.rowmap_ref import causal_pad_mask, compact_rows, prefix_live, row_plan_reference
from tests.test_kernels_gpu import close, ref_norm, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.25
P, SEED, SITE = 0.2, 4321, 6

# (B, T, live prefix): the first has shared quads (T = 7), an empty sample, -1 padding quads and M = 21 with a live last
# quad that reaches past M (the srow >= src_rows branch); the second the same with more rows; the third no padding at all
PLANS = [(3, 7, (2, 0, 7)), (5, 33, (33, 1, 0, 17, 33)), (1, 128, (128,))]


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def _plan(ops, B, T, n):
    live, mask = prefix_live(B, T, n), causal_pad_mask(B, T, n)
    ref = row_plan_reference(live, mask)
    L = ops.LiveRows.from_rows(live.to(torch.uint8).to(DEV), B, T, mask.to(DEV))
    L.host()
    assert L.Mc == ref["Mc"] and L.quad_list[:L.Mc // 4].cpu().tolist() == ref["quad_list"].tolist()
    orig, _ = compact_rows(ref)
    return L, ref, orig


def _ratio(got, ref, atol, rtol):
    return float(((got.detach().cpu().double() - ref.double()).abs() / (atol + rtol * ref.double().abs())).max())


def test_the_plans_cover_the_branches():
    p = row_plan_reference(prefix_live(3, 7, (2, 0, 7)))
    orig, _ = compact_rows(p)
    nq = p["info"][5]
    assert p["M"] % 4 and (orig[:4 * nq] < 0).any() and p["Mc"] > 4 * nq and (p["n_b"] == 0).any()
    assert int(p["cstart"][2]) % 4                                     # sample 2 starts inside a quad it shares
    p = row_plan_reference(prefix_live(1, 128, (128,)))
    assert (compact_rows(p)[0] >= 0).all()


@pytest.mark.parametrize("d", [12, 64, 512, 2048])
def test_norm_bwd_under_a_quad_map(ops, d):
    worst = {"dx": 0.0, "dalpha": 0.0, "dbias": 0.0}
    for B, T, n in PLANS:
        L, ref, orig = _plan(ops, B, T, n)
        M, Mc = B * T, L.Mc
        ok = orig >= 0
        rows = orig[ok]
        x, a, b = rnd(M, d, seed=1), rnd(d, seed=2) + 1, rnd(d, seed=3)
        dy, dres = rnd(M, d, seed=4), rnd(M, d, seed=5)
        xg, ag, bg, dyg, dresg = (t.to(DEV) for t in (x, a, b, dy, dres))
        _, mean, rstd = ops.norm_fwd(xg, ag, bg)
        # fp64 over the rows of the live quads
        xd, ad, bd = x[rows].double().requires_grad_(), a.double().requires_grad_(), b.double().requires_grad_()
        ref_norm(xd, ad, bd).backward(dy[rows].double())
        da, db = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
        dyc, dresc = L.gather(dyg), L.gather(dresg)
        for fwd in (False, True):
            L.fwd = fwd
            if fwd:       # the forward ran on the compact rows: x, mean and rstd are compact (zero rows where nothing is)
                xin = L.gather(xg)
                _, m_in, r_in = ops.norm_fwd(xin, ag, bg)
                assert torch.equal(m_in.cpu()[ok], mean.cpu()[rows]) and torch.equal(r_in.cpu()[ok], rstd.cpu()[rows])
            else:
                xin, m_in, r_in = xg, mean, rstd
            for with_res in (True, False):
                full = ops.norm_bwd(dyg, xg, ag, mean, rstd, da, db, dres=dresg if with_res else None)
                dropped = ops.dropout_bwd(full, P, SEED, SITE)
                for with_drop in (False, True):
                    out = torch.full((Mc + L.SLACK, d), SENT, device=DEV)
                    buf = torch.full((Mc + L.SLACK, d), SENT, device=DEV)
                    dac, dbc = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
                    got = ops.norm_bwd(dyc, xin, ag, m_in, r_in, dac, dbc, dres=dresc if with_res else None, out=out[:Mc],
                                       live=L, drop=(buf[:Mc], P, SEED, SITE) if with_drop else None)
                    what = f"d={d} plan={n} fwd={fwd} dres={with_res} drop={with_drop}"
                    goth = got.cpu()
                    # one wave's arithmetic per row on that row's inputs: bit equality with the dense call's rows
                    assert torch.equal(goth[ok], full.cpu()[rows]), f"dx rows of the live quads: {what}"
                    assert not goth[~ok].any(), f"dx padding rows: {what}"
                    assert (out[Mc:] == SENT).all(), f"dx wrote behind Mc: {what}"
                    want = xd.grad + (dres[rows].double() if with_res else 0.0)
                    worst["dx"] = max(worst["dx"], _ratio(goth[ok], want, 2e-5, 1e-4))
                    close(goth[ok], want, 2e-5, 1e-4, f"dx vs fp64: {what}")
                    if with_drop:
                        bh = buf.cpu()
                        assert torch.equal(bh[:Mc][ok], dropped.cpu()[rows]), f"drop_out rows: {what}"
                        assert not bh[:Mc][~ok].any() and (bh[Mc:] == SENT).all(), f"drop_out padding / slack rows: {what}"
                    else:
                        assert (buf == SENT).all()
                    tol = 1e-4 * math.sqrt(len(rows))
                    worst["dalpha"] = max(worst["dalpha"], _ratio(dac, ad.grad, tol, 1e-4))
                    worst["dbias"] = max(worst["dbias"], _ratio(dbc, bd.grad, tol, 1e-4))
                    close(dac, ad.grad, tol, 1e-4, f"dalpha: {what}")
                    close(dbc, bd.grad, tol, 1e-4, f"dbias: {what}")
    print(f"norm_bwd(live) d={d}: worst error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("d", [12, 64, 512, 2048])
def test_dropout_bwd_under_a_quad_map(ops, d):
    """The mask of compact quad i is that of original quad quad_list[i]: equal to the dense call on the scattered input,
    gathered back, bit for bit."""
    for B, T, n in PLANS:
        L, ref, orig = _plan(ops, B, T, n)
        g = rnd(B * T, d, seed=8).to(DEV)
        gc = L.gather(g)
        scattered = L.scatter(gc)                                      # zero outside the live quads
        want = L.gather(ops.dropout_bwd(scattered, P, SEED, SITE))
        got = ops.dropout_bwd(gc, P, SEED, SITE, live=L)
        assert torch.equal(got, want), f"d={d} plan={n}"
        assert not got[~(orig >= 0).to(DEV)].any()                     # padding rows stay zero
        if ref["quad_list"][:ref["info"][5]].tolist() != list(range(ref["info"][5])):
            assert not torch.equal(got, ops.dropout_bwd(gc, P, SEED, SITE)), "the mask was drawn at the compact coordinates"


@pytest.mark.parametrize("d", [12, 64, 512, 2048])
def test_norm_fwd_on_zero_variance_rows(ops, d):
    """A constant row and an all-zero row (the gap rows of a compact buffer) have std = 0: y = bias, finite.  Forward
    only: the reference's own backward is NaN there."""
    x = rnd(9, d, seed=1)
    x[1] = 0.0
    x[4] = 3.5                                        # sums of 3.5 are exact in fp32 up to d = 2048: mean = 3.5, x - mean = 0
    x[8] = -0.0
    a, b = rnd(d, seed=2) + 1, rnd(d, seed=3)
    y, mean, rstd = ops.norm_fwd(x.to(DEV), a.to(DEV), b.to(DEV))
    assert torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    for r in (1, 4, 8):
        close(y[r], b, 1e-6, 0.0, f"zero-variance row {r}")
    keep = [0, 2, 3, 5, 6, 7]
    close(y[keep], ref_norm(x[keep].double(), a.double(), b.double()), 1e-5, 1e-5, "the rows next to them")
