"""The ends of a bf16x6 GEMM tile (gemm_x6.inc): the peeled last K-tiles (reductions of 1, 2, 3 and 4 K-tiles are the
edge cases, 16 and 64 the training shapes), the epilogue operands requested from the last K-tile, and the epilogue that
starts without a workgroup barrier -- through ops.linear_fwd / ops.linear_dgrad with every epilogue the kernels can be
launched with.  Expected values come from the fp32-MFMA mode of the same call, at the bound of
test_kernels_gpu.py::test_linear_bf16x6_epilogues_and_dropout_masks; dropout masks must match exactly."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = [32, 64, 96, 128, 512, 2048]
# 67 row tiles (the last one ragged: M is odd) x 4 column tiles = 268 tiles of 128 x 256: more than one per CU, so the
# large-tile kernel runs, and the 12 tiles of the partial last round take the tail-split routes where the planner
# splits (K = 512: small-tile tail; K = 2048: K-split tail + fix-up)
M_ODD, N_OUT = 128 * 66 + 41, 1024


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def close(got, ref, atol, rtol, what=""):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} (ref scale {ref.abs().max().item():.3e}), {int(bad.sum())} bad"


def _mm64(a, b):
    """fp64 product of two fp32 CPU matrices (computed on the device: the reference, not the code under test)."""
    return (a.to(DEV).double() @ b.to(DEV).double()).cpu()


def _planes_for(ops, ws):
    flat = torch.cat([w.reshape(-1) for w in ws]).to(DEV).contiguous()
    views, o = [], 0
    for w in ws:
        views.append(flat[o:o + w.numel()].view(w.shape))
        o += w.numel()
    ops.register_planes(flat, ops.split_planes(flat))
    return flat, views


def _both_modes(ops, flat, run):
    """run() -> list of tensors, once per arithmetic mode; the bf16x6 run must launch only bf16x6 kernels for its GEMMs."""
    out = {}
    try:
        for mode in (ops.GEMM_F32, ops.GEMM_BF16X6):
            ops.gemm_set_mode(mode)
            c0, k0 = ops.gemm_launch_counts(), ops._L().gct_gemm_x6_kernel_launches()
            res, calls = run()
            c1, k1 = ops.gemm_launch_counts(), ops._L().gct_gemm_x6_kernel_launches()
            if mode == ops.GEMM_BF16X6:
                assert c1[1] - c0[1] == calls, f"{c1[1] - c0[1]} of {calls} calls took the bf16x6 kernels"
                assert k1 - k0 >= calls
            else:
                assert c1[1] == c0[1] and k1 == k0
            out[mode] = [t.cpu() for t in res]
    finally:
        ops.gemm_set_mode(ops.GEMM_BF16X6)
        ops.unregister_planes(flat)
    return out[ops.GEMM_F32], out[ops.GEMM_BF16X6]


@pytest.mark.parametrize("K", KS)
def test_forward_epilogues(ops, K):
    """EPI_BIAS, EPI_GELU_DROP_SAVE and EPI_DROP_RESID at p = 0 and p = 0.1, ragged M."""
    M, N = M_ODD, N_OUT
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    xg, bg, rg = x.to(DEV), b.to(DEV), r.to(DEV)
    bg1 = (b + 1.0).to(DEV)
    flat, (wg,) = _planes_for(ops, [w])

    def run():
        res = []
        y = torch.empty(M, N, device=DEV)
        ops.linear_fwd(xg, [wg], [bg], [y], N)
        res.append(y)
        for p in (0.0, 0.1):
            y1, sv, y2 = (torch.empty(M, N, device=DEV) for _ in range(3))
            ops.linear_fwd(xg, [wg], [bg], [y1], N, epi=ops.EPI_GELU_DROP_SAVE, pre=sv, p=p, seed=99, site=3)
            ops.linear_fwd(xg, [wg], [bg], [y2], N, epi=ops.EPI_DROP_RESID, resid=rg, p=p, seed=99, site=4)
            res += [y1, sv, y2]
        # zero residual: the dropped elements show as zeros.  So does a kept element whose product cancels the bias
        # exactly (x.w == -b in fp32: about one element in 10^7 here, and not the same one in the two arithmetic modes),
        # hence a second run with another bias: x.w cannot equal both -b and -(b + 1), so the elements that are zero in
        # both runs are exactly the dropped ones
        zero = torch.zeros_like(rg)
        y3, y4 = (torch.empty(M, N, device=DEV) for _ in range(2))
        ops.linear_fwd(xg, [wg], [bg], [y3], N, epi=ops.EPI_DROP_RESID, resid=zero, p=0.1, seed=99, site=4)
        ops.linear_fwd(xg, [wg], [bg1], [y4], N, epi=ops.EPI_DROP_RESID, resid=zero, p=0.1, seed=99, site=4)
        return res + [y3, y4], 7

    a, c = _both_modes(ops, flat, run)
    names = ["bias"] + [f"{n} p={p}" for p in (0.0, 0.1) for n in ("gelu+drop", "saved gelu'", "drop+resid")]
    for i, what in enumerate(names):
        close(c[i], a[i].double(), 5e-5, 1e-4, f"K={K} {what}")
    close(c[7], a[7].double(), 5e-5, 1e-4, f"K={K} drop, zero residual")
    close(c[8], a[8].double(), 5e-5, 1e-4, f"K={K} drop, zero residual, bias + 1")
    close(c[0], _mm64(x, w.t()) + b.double(), 2e-5, 2e-5, f"K={K} bias vs fp64")
    # p = 0.1: the same elements dropped in both modes
    mask_a, mask_c = (a[7] == 0) & (a[8] == 0), (c[7] == 0) & (c[8] == 0)
    assert torch.equal(a[5] == 0, c[5] == 0) and torch.equal(mask_a, mask_c)
    # the GELU output is also zero where erf saturates (x < -5.5 or so), which depends on the value, not on the mask:
    # every dropped element is zero, and any other zero is a saturated GELU in the fp32-mode run too
    dropped = a[5] == 0
    for t in (a[4], c[4]):
        assert (t[dropped] == 0).all()
    assert (a[4][(c[4] == 0) & ~dropped].abs() < 1e-6).all() and (c[4][(a[4] == 0) & ~dropped].abs() < 1e-6).all()
    for t in (c[5] == 0, mask_c):
        frac = t.float().mean().item()
        assert 0.09 < frac < 0.11, frac
    assert not (c[2] == 0).any()           # p = 0: nothing dropped


@pytest.mark.parametrize("K", KS)
def test_forward_three_segments(ops, K):
    """Q | K | V: three weight segments, three output blocks inside one [M][1536] buffer."""
    M, nper = M_ODD, 512
    N = 3 * nper
    x = rnd(M, K, seed=1)
    ws = [rnd(nper, K, seed=10 + s, scale=K ** -0.5) for s in range(3)]
    bs = [rnd(nper, seed=20 + s) for s in range(3)]
    xg, bg = x.to(DEV), [b.to(DEV) for b in bs]
    flat, wg = _planes_for(ops, ws)

    def run():
        y = torch.empty(M, N, device=DEV)
        ops.linear_fwd(xg, wg, bg, [y[:, s * nper:] for s in range(3)], N)
        return [y], 1

    a, c = _both_modes(ops, flat, run)
    close(c[0], a[0].double(), 5e-5, 1e-4, f"K={K} qkv")
    close(c[0], _mm64(x, torch.cat(ws).t()) + torch.cat(bs).double(), 2e-5, 2e-5, f"K={K} qkv vs fp64")


@pytest.mark.parametrize("K", KS)
def test_dgrad_epilogues(ops, K):
    """DEPI_STORE, DEPI_ACCUM and DEPI_MUL_SAVED over a reduction of K, ragged M."""
    M, N, p = M_ODD, N_OUT, 0.1
    dy, w = rnd(M, K, seed=6), rnd(K, N, seed=5, scale=0.05)
    base = rnd(M, N, seed=7)
    g = torch.Generator().manual_seed(8)
    saved = rnd(M, N, seed=9) * (torch.rand(M, N, generator=g) >= p)      # gelu' where kept, 0 where dropped
    dyg, sg = dy.to(DEV), saved.to(DEV)
    flat, (wg,) = _planes_for(ops, [w])

    def run():
        d0 = torch.empty(M, N, device=DEV)
        ops.linear_dgrad([dyg], K, M, [wg], d0)
        d1 = base.to(DEV)
        ops.linear_dgrad([dyg], K, M, [wg], d1, depi=ops.DEPI_ACCUM)
        d2 = torch.empty(M, N, device=DEV)
        ops.linear_dgrad([dyg], K, M, [wg], d2, depi=ops.DEPI_MUL_SAVED, pre=sg, p=p, seed=99, site=3)
        return [d0, d1, d2], 3

    a, c = _both_modes(ops, flat, run)
    for i, what in enumerate(("store", "accumulate", "mul saved")):
        close(c[i], a[i].double(), 5e-5, 1e-4, f"K={K} {what}")
    u = _mm64(dy, w)
    close(c[0], u, 5e-5, 5e-5, f"K={K} store vs fp64")
    close(c[1], u + base.double(), 5e-5, 5e-5, f"K={K} accumulate vs fp64")
    # zero where the saved factor is zero -- and where the product itself is exactly zero, which the plain store of the
    # same mode shows (same accumulators)
    for t in (a, c):
        assert torch.equal(t[2] == 0, (saved == 0) | (t[0] == 0))


@pytest.mark.parametrize("nper", [32, 64, 512])
def test_dgrad_three_segments(ops, nper):
    """dQ | dK | dV -> dx: the reduction runs over three dY segments of nper columns (3, 6 and 48 K-tiles in all)."""
    M, N = M_ODD, N_OUT
    dy = rnd(M, 3 * nper, seed=6)
    ws = [rnd(nper, N, seed=30 + s, scale=0.05) for s in range(3)]
    dyg = dy.to(DEV)
    flat, wg = _planes_for(ops, ws)

    def run():
        d0 = torch.empty(M, N, device=DEV)
        ops.linear_dgrad([dyg[:, s * nper:] for s in range(3)], 3 * nper, M, wg, d0)
        return [d0], 1

    a, c = _both_modes(ops, flat, run)
    close(c[0], a[0].double(), 5e-5, 1e-4, f"reduction 3 x {nper}")
    close(c[0], _mm64(dy, torch.cat(ws)), 5e-5, 5e-5, f"reduction 3 x {nper} vs fp64")


@pytest.mark.parametrize("K", KS)
def test_dgrad_mul_saved_through_quad_map(ops, K):
    """DEPI_MUL_SAVED on quad-compacted rows whose saved derivative stays in the forward's row space (pre_full): the rows
    are found through the quad map, padding quads (-1) give zero rows.  Against the same call on a gathered copy, bit for
    bit, and against the fp32-MFMA mode."""
    Mfull, Mc, N, p = 2 * (128 * 66 + 40), 128 * 66 + 40, N_OUT, 0.1
    g = torch.Generator().manual_seed(5)
    quads = torch.randperm(Mfull // 4, generator=g)[:Mc // 4].sort().values.to(torch.int32)
    quads[-5:] = -1                                        # padding quads at the end, as LiveRows leaves them
    qpad = torch.cat([quads, torch.full((32,), -1, dtype=torch.int32)])
    live = types.SimpleNamespace(quad_list=qpad.to(DEV), Mc=Mc)
    saved = rnd(Mfull, N, seed=1) * (torch.rand(Mfull, N, generator=g) >= p)
    rows = (quads.long().clamp(min=0)[:, None] * 4 + torch.arange(4)[None, :]).reshape(-1)
    saved_c = saved[rows] * (quads.long() >= 0).repeat_interleave(4)[:, None]
    dy, w = rnd(Mc, K, seed=2), rnd(K, N, seed=3, scale=0.05)
    dyg, sg, scg = dy.to(DEV), saved.to(DEV), saved_c.contiguous().to(DEV)
    flat, (wg,) = _planes_for(ops, [w])

    def run():
        d0, d1 = (torch.empty(Mc, N, device=DEV) for _ in range(2))
        ops.linear_dgrad([dyg], K, Mc, [wg], d0, depi=ops.DEPI_MUL_SAVED, pre=sg, p=p, seed=11, site=3, live=live,
                         pre_full=True)
        ops.linear_dgrad([dyg], K, Mc, [wg], d1, depi=ops.DEPI_MUL_SAVED, pre=scg, p=p, seed=11, site=3, live=live,
                         pre_full=False)
        d2 = torch.empty(Mc, N, device=DEV)      # the product itself: where it is exactly zero, so is d0
        ops.linear_dgrad([dyg], K, Mc, [wg], d2)
        return [d0, d1, d2], 3

    a, c = _both_modes(ops, flat, run)
    assert torch.equal(c[0], c[1]), "quad map vs gathered copy"
    close(c[0], a[0].double(), 5e-5, 1e-4, f"K={K} mul saved through the quad map")
    assert torch.equal(c[0] == 0, (saved_c == 0) | (c[2] == 0))
    assert (c[0][-20:] == 0).all()
