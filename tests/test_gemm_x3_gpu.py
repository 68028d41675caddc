"""The opt-in bf16x3 GEMM mode (ops.GEMM_BF16X3, gemm_x6.inc with 2 pieces) against fp64 on every route the bf16x6
mode takes: large tiles with and without tail balancing, small tiles, split-K over the whole problem, 128-row weight
segments, wgrad.  Per output element the error stays inside the bound stated in gemm_x6.inc,
    |err| <= (3.02 * 2^-16 + 1.5 * r32) * sum_k |a_k b_k|  +  flush floor,
with r32 the fp32-MFMA kernel's worst relative error on the same data (the shared accumulation term).  The launch
counters prove which kernels ran: the 2-piece kernels, launched exactly where bf16x6 mode launches the 3-piece ones."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
X3_REL = 3.02 * 2.0 ** -16
# x3 / x6 mean error against fp64 on random data, per GEMM that ran on the bf16 kernels.  The dropped am*bm + ah*bl +
# al*bh terms are ~2^-16 relative where bf16x6 leaves ~2^-26 plus fp32 accumulation rounding.  Measured on MI355X over
# ROUTE_SHAPES: 7.6x (a wgrad over 19 840 rows, where fp32 accumulation weighs most) to 50x; worst error / bound 0.10
# on random data, 0.34 on the adversarial sets (2^+-60 scales).
MEAN_RATIO_MIN = 4.0


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def planes_for(ops, ws):
    """The weights back to back in one buffer (as flat.py lays them out), with its bf16 planes registered."""
    flat = torch.cat([w.reshape(-1) for w in ws]).to(DEV).contiguous()
    views, o = [], 0
    for w in ws:
        views.append(flat[o:o + w.numel()].view(w.shape))
        o += w.numel()
    ops.register_planes(flat, ops.split_planes(flat))
    return flat, views


def counters(ops):
    return ops._L().gct_gemm_x6_kernel_launches(), ops.gemm_x3_launches(), ops.gemm_launch_counts()[1]


def run_three(ops, x, ws, bs, dy, fwd_ws=False):
    """fwd / dgrad / wgrad (+ bias grad) in F32, BF16X6 and BF16X3 mode.  Returns {mode: (outputs, per-call counter
    deltas (x6 kernels, x3 kernels, launch_counts[1]))}."""
    M, K = x.shape
    nper, nseg = ws[0].shape[0], len(ws)
    N = nper * nseg
    xg, dyg = x.to(DEV), dy.to(DEV)
    bg = [b.to(DEV) if b is not None else None for b in bs]
    dys = [dyg[:, s * nper:] for s in range(nseg)]
    flat, wg = planes_for(ops, ws)
    wsb = (torch.empty(int(ops._L().gct_linear_fwd_ws_bytes(M, K, N)) // 4 + 64, device=DEV) if fwd_ws else None)
    res = {}
    keep = ops.gemm_get_mode()
    try:
        for mode in (ops.GEMM_F32, ops.GEMM_BF16X6, ops.GEMM_BF16X3):
            ops.gemm_set_mode(mode)
            deltas = []
            c0 = counters(ops)
            y = torch.empty(M, N, device=DEV)
            ops.linear_fwd(xg, wg, bg, [y[:, s * nper:] for s in range(nseg)], N, ws=wsb)
            c1 = counters(ops)
            dx = torch.empty(M, K, device=DEV)
            ops.linear_dgrad(dys, N, M, wg, dx)
            c2 = counters(ops)
            dws = [torch.empty(nper, K, device=DEV) for _ in range(nseg)]
            dbs = [torch.empty(nper, device=DEV) for _ in range(nseg)]
            ops.linear_wgrad(dys, N, xg, dws, dbs)
            c3 = counters(ops)
            for a, b in ((c0, c1), (c1, c2), (c2, c3)):
                deltas.append(tuple(bb - aa for aa, bb in zip(a, b)))
            res[mode] = ([y.cpu().double(), dx.cpu().double(), torch.cat(dws).cpu().double(),
                          torch.cat(dbs).cpu().double()], deltas)
    finally:
        ops.gemm_set_mode(keep)
        ops.unregister_planes(flat)
    return res


def check_x3(ops, x, ws, bs, dy, res, what, ratio_min=None):
    """The per-element bound, the counters, and (ratio_min) the x3 / x6 mean-error ratio.  Returns the measured
    (worst error / bound, x3 / x6 mean-error ratios)."""
    X, W, DY = x.double(), torch.cat(ws).double(), dy.double()
    b = torch.cat([bb if bb is not None else torch.zeros(ws[0].shape[0]) for bb in bs]).double()
    refs = (X @ W.t() + b, DY @ W, DY.t() @ X)
    mags = (X.abs() @ W.abs().t() + b.abs(), DY.abs() @ W.abs(), DY.abs().t() @ X.abs())
    # pieces below bf16's normal range are flushed: < 2^-126 per piece and product partner
    floors = (3 * 2.0 ** -126 * W.abs().sum(1)[None, :], 3 * 2.0 ** -126 * W.abs().sum(0)[None, :],
              3 * 2.0 ** -126 * (DY.abs().sum(0)[:, None] + X.abs().sum(0)[None, :]))
    out32, _ = res[ops.GEMM_F32]
    out6, d6 = res[ops.GEMM_BF16X6]
    out3, d3 = res[ops.GEMM_BF16X3]
    # the 2-piece kernels ran exactly where bf16x6 mode ran the 3-piece ones, and nothing else moved
    for i, call in enumerate(("fwd", "dgrad", "wgrad")):
        assert d3[i][0] == 0 and d3[i][2] == 0, f"{what} {call}: bf16x6 counters moved in bf16x3 mode {d3[i]}"
        assert d6[i][1] == 0, f"{what} {call}: bf16x3 counter moved in bf16x6 mode"
        assert d3[i][1] == d6[i][0], f"{what} {call}: {d3[i][1]} bf16x3 launches, bf16x6 mode made {d6[i][0]}"
    worst, ratios = 0.0, []
    for i, call in enumerate(("fwd", "dgrad", "wgrad")):
        e3 = (out3[i] - refs[i]).abs()
        e32 = (out32[i] - refs[i]).abs()
        assert torch.isfinite(out3[i]).all(), f"{what} {call}"
        r32 = (e32 / mags[i].clamp_min(1e-300)).max().item()
        bound = (X3_REL + 1.5 * r32) * mags[i] + floors[i]
        w = (e3 / bound).max().item()
        worst = max(worst, w)
        assert w <= 1.0, f"{what} {call}: error {w:.3f} x the stated bf16x3 bound (r32 = {r32:.3e})"
        if ratio_min is not None and d3[i][1] > 0:
            e6 = (out6[i] - refs[i]).abs().mean().item()
            r = e3.mean().item() / max(e6, 1e-300)
            ratios.append(r)
            assert r >= ratio_min, f"{what} {call}: x3 mean error only {r:.2f} x the x6 one (x3 kernels in disguise?)"
    # bias gradients are fp32 sums of dY in every mode (no split)
    tb = 1e-4 * math.sqrt(X.shape[0] / 100 + 1)
    e = (out3[3] - DY.sum(0)).abs()
    assert (e <= tb + 1e-4 * DY.sum(0).abs()).all(), f"{what}: bias grad"
    return worst, ratios


# (M, K, nper, nseg, fwd workspace): the shapes of test_linear_bf16x6_vs_fp64 (segmented weights included), the
# small-tile shapes, split-K over the whole problem (workspace), a tail-balanced launch with a workspace, and the
# sampler's mu | log_var (two segments of 128 weight rows)
ROUTE_SHAPES = [(300, 512, 512, 3, False), (1000, 2048, 512, 1, False), (4099, 512, 2048, 1, False),
                (6400, 64, 520, 1, False), (2048, 512, 256, 2, False), (96, 128, 1000, 1, False),
                (3104, 512, 512, 3, False),
                (4096, 512, 512, 1, False), (2050, 1024, 520, 1, False), (3000, 512, 512, 2, False),
                (1500, 64, 1000, 1, False),
                (1024, 2048, 512, 1, True),
                (128 * 66 + 40, 512, 1024, 1, True), (155 * 128, 512, 512, 2, True),
                (6144, 512, 128, 2, False)]


def route_case(ops, M, K, nper, nseg, fwd_ws):
    x = rnd(M, K, seed=1)
    ws = [rnd(nper, K, seed=10 + s, scale=max(K, 64) ** -0.5) for s in range(nseg)]
    bs = [rnd(nper, seed=20 + s) for s in range(nseg)]
    dy = rnd(M, nper * nseg, seed=3)
    res = run_three(ops, x, ws, bs, dy, fwd_ws)
    worst, ratios = check_x3(ops, x, ws, bs, dy, res, f"M={M} K={K} N={nper}x{nseg}", MEAN_RATIO_MIN)
    return worst, ratios, [d[1] for d in res[ops.GEMM_BF16X3][1]]


@pytest.mark.parametrize("M,K,nper,nseg,fwd_ws", ROUTE_SHAPES)
def test_linear_bf16x3_every_route_vs_fp64(ops, M, K, nper, nseg, fwd_ws):
    _, _, launches = route_case(ops, M, K, nper, nseg, fwd_ws)
    if M * nper * nseg >= 1 << 20:
        assert sum(launches) > 0          # the large shapes engage the bf16 routes


def _adversarial(kind, M, K, N):
    """The operand sets of tests/test_kernels_gpu.py::test_linear_bf16x6_adversarial_vs_fp64."""
    x, w, dy = rnd(M, K, seed=31), rnd(N, K, seed=32, scale=K ** -0.5), rnd(M, N, seed=33)
    if kind == "cancel":
        x = torch.cat([x, x], 1)
        w = torch.cat([w, -w * (1 + 2.0 ** -12)], 1)
    elif kind == "scales":
        e = torch.randint(-60, 61, (K,), generator=torch.Generator().manual_seed(5)).float()
        x, w = x * torch.exp2(e), w * torch.exp2(-e)
        dy = dy * torch.exp2(torch.randint(-60, 61, (N,), generator=torch.Generator().manual_seed(6)).float())
    elif kind == "ones":
        full = 2.0 - 2.0 ** -23
        mk = lambda t, sd: torch.sign(t) * full * torch.exp2(                                     # noqa: E731
            torch.randint(-3, 4, t.shape, generator=torch.Generator().manual_seed(sd)).float())
        x, w, dy = mk(x, 7), mk(w, 8) * K ** -0.5, mk(dy, 9)
    elif kind == "tiny":
        dy = dy * 2.0 ** -112
    return x.float(), w.float(), dy.float()


def adversarial_case(ops, kind):
    M, K0, N = 6144, 512, 512
    x, w, dy = _adversarial(kind, M, K0, N)
    b = rnd(N, seed=34) * (0.0 if kind in ("cancel", "tiny") else 1.0)
    res = run_three(ops, x, [w], [b], dy)
    assert [d[1] for d in res[ops.GEMM_BF16X3][1]] == [1, 1, 1]        # all three calls on the bf16x3 kernels
    return check_x3(ops, x, [w], [b], dy, res, kind)[0]


@pytest.mark.parametrize("kind", ["cancel", "scales", "ones", "tiny"])
def test_linear_bf16x3_adversarial_vs_fp64(ops, kind):
    adversarial_case(ops, kind)


def epilogue_case(ops, M, N):
    """Fused epilogues in bf16x6 and bf16x3 mode (twice): returns {label: outputs}."""
    K, p, seed = 512, 0.1, 99
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    W2 = rnd(K, N, seed=5, scale=0.05)
    dy, base = rnd(M, K, seed=6), rnd(M, N, seed=7)
    xg, bg, rg, dyg = x.to(DEV), b.to(DEV), r.to(DEV), dy.to(DEV)
    flat, (wg, w2g) = planes_for(ops, [w, W2])
    out = {}
    keep = ops.gemm_get_mode()
    try:
        for label, mode in (("x6", ops.GEMM_BF16X6), ("x3", ops.GEMM_BF16X3), ("x3 again", ops.GEMM_BF16X3)):
            ops.gemm_set_mode(mode)
            k3 = ops.gemm_x3_launches()
            y0, y1, pre, y2, dpre = (torch.empty(M, N, device=DEV) for _ in range(5))
            acc = base.to(DEV).clone()
            ops.linear_fwd(xg, [wg], [bg], [y0], N)
            ops.linear_fwd(xg, [wg], [bg], [y1], N, epi=ops.EPI_GELU_DROP, pre=pre, p=p, seed=seed, site=3)
            ops.linear_fwd(xg, [wg], [bg], [y2], N, epi=ops.EPI_DROP_RESID, resid=rg, p=p, seed=seed, site=4)
            ops.linear_dgrad([dyg], K, M, [w2g], dpre, depi=ops.DEPI_GELU_BWD, pre=pre, p=p, seed=seed, site=3)
            ops.linear_dgrad([dyg], K, M, [w2g], acc, depi=ops.DEPI_ACCUM)
            if mode == ops.GEMM_BF16X3:
                assert ops.gemm_x3_launches() > k3
            out[label] = [t.cpu() for t in (y0, y1, pre, y2, dpre, acc)]
    finally:
        ops.gemm_set_mode(keep)
        ops.unregister_planes(flat)
    return out, (x, w, b, r, W2, dy, base, p)


@pytest.mark.parametrize("M,N", [(640, 2048), (128 * 66 + 40, 1024)])
def test_linear_bf16x3_epilogues_masks_and_determinism(ops, M, N):
    """Bias, GELU + dropout, dropout + residual, GELU backward (dgrad) and accumulate (dgrad) in bf16x3 mode: the dropout
    masks are those of bf16x6 mode bit for bit (a mask depends on (seed, site, row, col) only), two identical calls give
    bit-identical results, and the values stay inside the bf16x3 bound around the bf16x6 ones.  The second shape has
    268 tiles of 128 x 256: its tail rows run as a second launch."""
    out, (x, w, b, r, W2, dy, base, p) = epilogue_case(ops, M, N)
    c6, c3, c3b = out["x6"], out["x3"], out["x3 again"]
    for t, u in zip(c3, c3b):
        assert torch.equal(t, u), "two identical bf16x3 calls differ"
    assert torch.equal(c6[1] == 0, c3[1] == 0), "GELU + dropout mask"
    assert torch.equal(c6[4] == 0, c3[4] == 0), "GELU backward dropout mask"
    u = x.double() @ w.double().t() + b.double()
    # a kept element whose value is below the rounding of the residual it is added to cannot be told from a dropped one
    assert not (((c6[3] == r) != (c3[3] == r)) & (u.abs() > 1e-4)).any(), "dropout + residual mask"
    mag_f = x.double().abs() @ w.double().abs().t() + b.double().abs()
    mag_d = dy.double().abs() @ W2.double().abs()
    tol = lambda mag, s: 1.2 * X3_REL * s * mag + 5e-5 + 1e-4 * mag.abs().max() * 2.0 ** -20   # noqa: E731
    for i, mag, s in ((0, mag_f, 1.0), (1, mag_f, 1.0 / (1 - p)), (2, mag_f, 1.0), (3, mag_f, 1.0 / (1 - p)),
                      (4, mag_d, 1.13 / (1 - p)), (5, mag_d, 1.0)):
        err = (c3[i].double() - c6[i].double()).abs()
        assert (err <= tol(mag, s) + 1e-4 * c6[i].double().abs()).all(), \
            f"output {i}: max err {err.max().item():.3e} against bf16x6"
    assert ((c3[2].double() - u).abs() <= 1.2 * X3_REL * mag_f + 2e-5 + 2e-5 * u.abs()).all(), "pre vs fp64"
