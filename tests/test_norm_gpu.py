"""gct_norm_fwd / gct_norm_bwd against tests/norm_ref.py (fp64 on the CPU, bounds derived from the data) through raw
library calls:

  A  values: every input family x every width of norm_ref.WIDTHS (all four chunk instantiations with full, partial and
     wholly empty chunks) x eps 1e-6 / 1e-2 x with / without dres; y, mean, rstd, dx, dalpha, dbias
  B  rows = 1, 3, 4, 5 (partial and single quads), 32 773 (both grid-stride loops wrap, the last quad is partial), 0
  C  the engine's in-place forms: dx over dy (enc_layer_bwd) and dx over dres (dec_layer_bwd), with and without the
     drop_out second output, bit-equal to the out-of-place call
  D  constant, all-zero and -0.0 rows among ordinary ones (sigma = 0: the k2 guard)
  E  refusals before a launch: unsupported d, misaligned x / dy / ws, a quad map over rows % 4 != 0, p = 1 with drop_out

Every call: all outputs start as NaN; the backward reads the mean and rstd the forward call wrote; its workspace is
exactly gct_rowred_ws_bytes(rows, 2 d) plus a 4 KiB guard that must stay untouched, once NaN-filled and once
zero-filled (bit-equal results).  tests/test_norm_ref_host.py shows that these inputs put a kernel's likely mistakes
>= 10 x outside the bounds.

Measured on MI355X, worst error / bound per family (y, mean, rstd, dx, dalpha, dbias), printed at the end of the
module with -s:
  unit 0.320 0.088 0.316 0.334 0.055 0.092          offset 0.285 0.285 0.328 0.278 0.081 0.092
  sigma-eps 0.333 0.070 0.243 0.339 0.044 0.092     sigma-below-eps 0.332 0.074 0.170 0.329 0.050 0.092
  half-1e-5 0.388 0.388 0.151 0.384 0.097 0.092     scale-1e12 0.313 0.088 0.244 0.268 0.037 0.092
  scale-1e-12 0.333 0.154 0.160 0.286 0.037 0.092   mixed 0.503 0.503 0.385 0.477 0.240 0.169 (rows = 32 773, d = 12)
  zero-variance 0.219 0.057 0.277 0.315 0.030 0.051
The 48 tests take 6 s.  With rsqrtf(var + eps) patched into the forward, section A fails on every family but scale-1e12
(sigma-eps: y at 9.8e5 x the bound), and with sigma = 1 / r patched into the backward on the small-sigma families (dx at
1.3e5 x), while test_kernels_gpu.py::test_norm passes both."""
import pytest
import torch

from tests import norm_ref as N
from tests.test_wgrad_gpu import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
BIG = 32773                      # > 32 768 rows (forward grid of 8192 blocks) and > 16 384 (backward grid of 1024); % 4 = 1
DROP = (0.1, 1234, 5)            # p, seed, site of the second output
WORST = {}                       # worst error / bound per (family, quantity)


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib
    yield _lib.load()
    for fam in sorted({k[0] for k in WORST}):
        print(f"[norm] worst err / bound  {fam:16s} " + "  ".join(f"{q} {WORST.get((fam, q), 0.0):.3f}" for q in N.QUANTITIES))


def _st():
    return torch.cuda.current_stream().cuda_stream


def nanf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts if t is not None)


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + off


def raw_fwd(lib, x, a, b, eps, rows, d, x_off=0):
    """rc and the NaN-prefilled (y, mean, rstd) of one gct_norm_fwd"""
    y, mean, rstd = nanf(max(rows, 1), d), nanf(max(rows, 1)), nanf(max(rows, 1))
    rc = lib.gct_norm_fwd(_ptr(x, x_off), _ptr(a), _ptr(b), _ptr(y), _ptr(mean), _ptr(rstd), rows, d, eps, _st())
    torch.cuda.synchronize()
    return rc, y, mean, rstd


def raw_bwd(lib, dy, x, a, mean, rstd, dres, eps, rows, d, fill=float("nan"), alias=None, drop=False, p=DROP[0],
            qmap=None, off=None):
    """rc and the NaN-prefilled (dx, dalpha, dbias, drop_out) of one gct_norm_bwd whose workspace holds `fill`.
    alias: dx is written over (a copy of) "dy" or "dres"; off: {"x" | "dy" | "ws": bytes} pushes that pointer off"""
    off = off or {}
    need = int(lib.gct_rowred_ws_bytes(rows, 2 * d))
    assert need % 16 == 0
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
    ws[:need].view(torch.float32).fill_(fill)
    ws[need:] = 0xA5
    dy = dy.clone()
    dres = None if dres is None else dres.clone()
    dx = dy if alias == "dy" else dres if alias == "dres" else nanf(max(rows, 1), d)
    dalpha, dbias = nanf(d), nanf(d)
    dropo = nanf(max(rows, 1), d) if drop else None
    rc = lib.gct_norm_bwd(_ptr(dy, off.get("dy", 0)), _ptr(x, off.get("x", 0)), _ptr(a), _ptr(mean), _ptr(rstd), _ptr(dres),
                          _ptr(dx), _ptr(dalpha), _ptr(dbias), _ptr(ws, off.get("ws", 0)), rows, d, eps, _ptr(qmap), 0,
                          _ptr(dropo), p if drop else 0.0, DROP[1] if drop else 0, DROP[2] if drop else 0, _st())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), f"rows {rows} d {d}: the call wrote past gct_rowred_ws_bytes = {need}"
    return rc, dx, dalpha, dbias, dropo


def bwd(lib, *args, **kw):
    """raw_bwd over a NaN-filled and over a zero-filled workspace: rc 0 and bit-equal results; returns the first"""
    first = raw_bwd(lib, *args, fill=float("nan"), **kw)
    again = raw_bwd(lib, *args, fill=0.0, **kw)
    assert first[0] == 0 and again[0] == 0, (first[0], again[0])
    for name, u, v in zip(("dx", "dalpha", "dbias", "drop_out"), first[1:], again[1:]):
        assert bits_equal(u, v), f"{name} depends on what the workspace held"
    return first[1:]


def hold(family, key, got, ref, bnd, quantities=N.QUANTITIES, rows=None):
    """every quantity within its bound (rows: compare y / dx on these rows only)"""
    for q in quantities:
        g, w, b = getattr(got, q).cpu(), getattr(ref, q), getattr(bnd, q)
        if rows is not None and q in ("y", "dx"):
            g, w, b = g[rows], w[rows], b[rows]
        r = N.ratio(g, w, b)
        WORST[(family, q)] = max(WORST.get((family, q), 0.0), r)
        assert r <= 1.0, f"{key} {q}: worst error is {r:.3g} x the bound"


def run(lib, family, key, p, ref, bnd, **kw):
    """forward, then backward on the forward's mean / rstd; all six outputs against the reference"""
    rows, d = p.x.shape
    x, a, b, dy = (t.to(DEV) for t in (p.x, p.alpha, p.bias, p.dy))
    dres = None if p.dres is None else p.dres.to(DEV)
    rc, y, mean, rstd = raw_fwd(lib, x, a, b, p.eps, rows, d)
    assert rc == 0
    dx, dalpha, dbias, _ = bwd(lib, dy, x, a, mean, rstd, dres, p.eps, rows, d)
    got = N.Out(y, mean, rstd, dx, dalpha, dbias)
    hold(family, key, got, ref, bnd, **kw)
    return got


# ------------------------------------------------------------------------------------------------ A: values
@pytest.mark.parametrize("eps", N.EPSES)
@pytest.mark.parametrize("family", list(N.FAMILIES))
def test_values(lib, family, eps):
    for d in N.WIDTHS:
        for with_dres in (False, True):
            p, ref, bnd = N.case(family, N.ROWS, d, eps, with_dres)
            run(lib, family, f"{family} d={d} eps={eps} dres={with_dres}", p, ref, bnd)


# ------------------------------------------------------------------------------------------------ B: row counts
@pytest.mark.parametrize("d", [12, 512])
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_few_rows(lib, rows, d):
    for eps in N.EPSES:
        p, ref, bnd = N.case("mixed", rows, d, eps, True)
        run(lib, "mixed", f"rows={rows} d={d} eps={eps}", p, ref, bnd)


@pytest.mark.parametrize("d", [12, 260])
def test_rows_that_wrap_both_grids(lib, d):
    assert (BIG + 3) // 4 > 8192 and BIG % 4 == 1 and N.norm_blocks(BIG) == 1024
    p = N.problem("mixed", BIG, d, 1e-6, True)
    run(lib, "mixed", f"rows={BIG} d={d}", p, N.reference(p), N.bounds(p))


@pytest.mark.parametrize("d", [12, 260])
def test_no_rows(lib, d):
    x, a, b = nanf(1, d), torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    rc, y, mean, rstd = raw_fwd(lib, x, a, b, 1e-6, 0, d)
    assert rc == 0 and all_nan(y, mean, rstd)                  # OK, and nothing written
    dx, dalpha, dbias, _ = bwd(lib, x, x, a, mean, rstd, None, 1e-6, 0, d)
    assert all_nan(dx) and not dalpha.any() and not dbias.any()                # exact zeros, not what ws held


# ------------------------------------------------------------------------------------------------ C: in-place forms
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop-out"])
@pytest.mark.parametrize("rows", [N.ROWS, BIG])
@pytest.mark.parametrize("d", [260, 512])
def test_in_place_forms_equal_the_out_of_place_call(lib, d, rows, drop):
    g = torch.Generator(device=DEV).manual_seed(d + rows)
    x, dy, dres = (torch.randn(rows, d, device=DEV, generator=g) for _ in range(3))
    a, b = torch.randn(d, device=DEV, generator=g) + 1.0, torch.randn(d, device=DEV, generator=g)
    rc, _, mean, rstd = raw_fwd(lib, x, a, b, 1e-6, rows, d)
    assert rc == 0
    plain = bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, rows, d, drop=drop)
    assert not all_nan(plain[0]) and bool(torch.isfinite(plain[0]).all())
    if drop:
        kept = float((plain[3] != 0).float().mean())
        assert abs(kept - (1 - DROP[0])) < 0.02, kept          # the second output is a masked copy, not a plain one
    for alias in ("dy", "dres"):                               # enc_layer_bwd: out = dy; dec_layer_bwd: out = dres
        inplace = bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, rows, d, drop=drop, alias=alias)
        for name, u, v in zip(("dx", "dalpha", "dbias", "drop_out"), plain, inplace):
            assert bits_equal(u, v), f"dx over {alias}: {name} differs from the out-of-place call"


# ------------------------------------------------------------------------------------------------ D: rows at the guard
DEGENERATE = {5: 2.5, 6: 0.0, 17: -0.0}                        # row -> its constant; sums of 2.5 are exact in fp32


@pytest.mark.parametrize("eps", N.EPSES)
@pytest.mark.parametrize("d", [12, 260])
def test_rows_of_zero_variance(lib, d, eps):
    base = N.problem("unit", N.ROWS, d, eps, True)
    x, dy = base.x.clone(), base.dy.clone()
    deg = torch.zeros(N.ROWS, dtype=torch.bool)
    for row, v in DEGENERATE.items():
        x[row] = v
        deg[row] = True
    assert bool(torch.signbit(x[17]).all())

    # dy = 0 on the degenerate rows: they add exact zeros to dalpha / dbias, which then are sums over the other rows.
    # d sigma / dx does not exist at sigma = 0 (torch.std's backward happens to put 0 there): on these rows dx is held
    # to the closed form below, not to autograd
    dy0 = dy.clone()
    dy0[deg] = 0
    p = base._replace(x=x, dy=dy0)
    ref, bnd = N.reference(p), N.bounds(p, rows=~deg)
    assert bool(torch.isfinite(ref.dalpha).all()) and bool(torch.isfinite(ref.dbias).all())
    got = run(lib, "zero-variance", f"d={d} eps={eps}", p, ref, bnd, rows=~deg)
    y, mean, rstd, dx = (t.cpu() for t in (got.y, got.mean, got.rstd, got.dx))
    assert torch.equal(y[deg], p.bias.expand(3, d))            # y = bias exactly
    assert torch.equal(mean[deg], torch.tensor([2.5, 0.0, 0.0])) and bool(torch.isfinite(rstd).all())
    assert torch.equal(dx[deg], p.dres[deg])                   # r (0 - 0) - 0 k2 + dres

    # dy != 0 on them: dx = r (g - mean g) + dres with r = 1 / eps, and finite whatever 1 / r - eps rounds to
    p = base._replace(x=x, dy=dy)
    rc, _, mean, rstd = raw_fwd(lib, p.x.to(DEV), p.alpha.to(DEV), p.bias.to(DEV), eps=p.eps, rows=N.ROWS, d=d)
    assert rc == 0
    dx, _, _, _ = bwd(lib, p.dy.to(DEV), p.x.to(DEV), p.alpha.to(DEV), mean, rstd, p.dres.to(DEV), p.eps, N.ROWS, d)
    dx = dx.cpu()
    g = p.dy.double() * p.alpha.double()
    want = (g - g.mean(-1, keepdim=True)) / p.eps + p.dres.double()
    assert bool(torch.isfinite(dx).all())
    r = N.ratio(dx[deg], want[deg], N.bounds(p).dx[deg])
    WORST[("zero-variance", "dx")] = max(WORST.get(("zero-variance", "dx"), 0.0), r)
    assert r <= 1.0, f"dx of the zero-variance rows: {r:.3g} x the bound"


# ------------------------------------------------------------------------------------------------ E: refusals
def _operands(rows, d):
    """buffers long enough for any d of this section, one float4 of slack for the pushed pointers"""
    wide = max(d, 2052) + 4
    x, dy, dres = (torch.ones(rows, wide, device=DEV) for _ in range(3))
    return x, dy, dres, torch.ones(wide, device=DEV), torch.zeros(wide, device=DEV), nanf(rows), nanf(rows)


@pytest.mark.parametrize("d", [2, 6, 2052])
def test_unsupported_widths_are_refused(lib, d):
    x, dy, dres, a, b, mean, rstd = _operands(8, d)
    rc, *outs = raw_fwd(lib, x, a, b, 1e-6, 8, d)
    assert rc != 0 and all_nan(*outs)
    rc, *outs = raw_bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, 8, d, drop=True)
    assert rc != 0 and all_nan(*outs)


@pytest.mark.parametrize("which", ["x", "dy", "ws"])
def test_misaligned_pointers_are_refused(lib, which):
    d = 260
    x, dy, dres, a, b, mean, rstd = _operands(8, d)
    if which == "x":
        rc, *outs = raw_fwd(lib, x, a, b, 1e-6, 8, d, x_off=4)
        assert rc != 0 and all_nan(*outs)
    rc, *outs = raw_bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, 8, d, drop=True, off={which: 4})
    assert rc != 0 and all_nan(*outs)
    rc, *outs = raw_bwd(lib, dy, x, a, torch.zeros(8, device=DEV), torch.ones(8, device=DEV), dres, 1e-6, 8, d, drop=True)
    assert rc == 0 and not all_nan(outs[0])                    # the same call with the pointer in place goes through


def test_a_quad_map_over_partial_quads_is_refused(lib):
    d = 260
    x, dy, dres, a, b, mean, rstd = _operands(N.ROWS, d)
    qmap = torch.arange(16, dtype=torch.int32, device=DEV)
    rc, *outs = raw_bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, N.ROWS, d, drop=True, qmap=qmap)
    assert N.ROWS % 4 and rc != 0 and all_nan(*outs)


def test_dropping_everything_is_refused(lib):
    d = 260
    x, dy, dres, a, b, mean, rstd = _operands(8, d)
    rc, *outs = raw_bwd(lib, dy, x, a, mean, rstd, dres, 1e-6, 8, d, drop=True, p=1.0)
    assert rc != 0 and all_nan(*outs)
