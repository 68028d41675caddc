"""The FFN's saved-factor epilogue pair (GCT_EPI_GELU_DROP_SAVE forward, GCT_DEPI_MUL_SAVED dgrad) against the
recomputing pair it replaces in the model (GCT_EPI_GELU_DROP saving pre = acc + b, GCT_DEPI_GELU_BWD).  On the same
data, in every GEMM mode, with and without dropout:
  * the forward output y is bit-identical (same erf, same operations);
  * dpre is bit-identical: the saved factor d = keep ? gelu'(v) : 0 is the value the old backward recomputes from
    pre = v, and dx = d == 0 ? 0 : (acc * d) * keep_scale is the old keep ? (acc * gelu'(v)) * keep_scale : 0 in the
    same order (torch.equal: an exact zero may differ in sign only);
  * both agree with an fp64 restatement.
Shapes: the training FFN at 40 960 rows (tail-balanced bf16 launches), a ragged 77-row problem (fp32 / small-tile
routes), and the quad-compacted decoder: a compact forward with its compact saved factor, and a full-row forward
whose factor the compact backward reads through the quad map (pre_rows)."""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, DFF, SEED = 512, 2048, 4321
X3_REL = 3.02 * 2.0 ** -16            # bf16x3 per-product bound (include/gctplus_hip.h)


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def planes_for(ops, ws):
    flat = torch.cat([w.reshape(-1) for w in ws]).to(DEV).contiguous()
    views, o = [], 0
    for w in ws:
        views.append(flat[o:o + w.numel()].view(w.shape))
        o += w.numel()
    ops.register_planes(flat, ops.split_planes(flat))
    return flat, views


def quad_list(n_quads, n_live, seed):
    """Ascending live quads of n_quads, padded with -1 to a multiple of 32 (the gct_live_rows layout)."""
    g = torch.Generator().manual_seed(seed)
    live = torch.randperm(n_quads, generator=g)[:n_live].sort().values
    pad = (-n_live) % 32
    return torch.cat([live, torch.full((pad,), -1, dtype=torch.long)]).to(torch.int32)


def both_pairs(ops, x, w1, b1, w2, dy, p, site, fwd_map=None, bwd_map=None, pre_full=False):
    """(y, dpre) of the old and the new epilogue pair on the same operands, in the current GEMM mode.
    fwd_map / bwd_map: quad lists of the forward / the dgrad (None: plain rows)."""
    M, Mb = x.shape[0], dy.shape[0]
    fl = None if fwd_map is None else types.SimpleNamespace(quad_list=fwd_map)
    bl = None if bwd_map is None else types.SimpleNamespace(quad_list=bwd_map)
    out = {}
    for name, epi, depi in (("old", ops.EPI_GELU_DROP, ops.DEPI_GELU_BWD),
                            ("new", ops.EPI_GELU_DROP_SAVE, ops.DEPI_MUL_SAVED)):
        y, saved = torch.empty(M, DFF, device=DEV), torch.empty(M, DFF, device=DEV)
        ops.linear_fwd(x, [w1], [b1], [y], DFF, epi=epi, pre=saved, p=p, seed=SEED, site=site, live=fl)
        dpre = torch.empty(Mb, DFF, device=DEV)
        ops.linear_dgrad([dy], D, Mb, [w2], dpre, depi=depi, pre=saved, p=p, seed=SEED, site=site, live=bl,
                         pre_full=pre_full)
        out[name] = (y, dpre)
    torch.cuda.synchronize()
    return out


def assert_same(out, what):
    (y0, g0), (y1, g1) = out["old"], out["new"]
    assert torch.equal(y0, y1), f"{what}: y differs from the GELU_DROP forward"
    assert torch.equal(g0 == 0, g1 == 0), f"{what}: dpre zero patterns differ"
    assert torch.equal(g0, g1), f"{what}: dpre differs by up to {(g0 - g1).abs().max().item():.3e}"


def check_fp64(ops, mode, y, dpre, x, w1, b1, w2, dy, keep, p, what):
    """y / dpre (rows matching x / dy / keep) against fp64: u = x w1^T + b1, y = gelu(u) keep / (1-p),
    dpre = (dy w2) gelu'(u) keep / (1-p)."""
    X, W1, B1 = x.double().cpu(), w1.double().cpu(), b1.double().cpu()
    DY, W2 = dy.double().cpu(), w2.double().cpu()
    s = 1.0 / (1.0 - p)
    u = (X @ W1.t() + B1).requires_grad_()
    kf = keep.double().cpu()
    gw = DY @ W2
    (F.gelu(u) * kf * s * gw).sum().backward()
    ref_y, ref_d = (F.gelu(u) * kf * s).detach(), u.grad
    if mode == ops.GEMM_BF16X3:       # ~16 good bits per product: the bound of tests/test_gemm_x3_gpu.py, through gelu / gelu'
        mag_f = X.abs() @ W1.abs().t() + B1.abs()
        mag_d = DY.abs() @ W2.abs()
        tol_y = 1.2 * X3_REL * s * 1.13 * mag_f + 5e-5
        tol_d = 1.2 * X3_REL * s * (1.13 * mag_d + gw.abs() * mag_f) + 5e-5
    else:
        tol_y = tol_d = 3e-5
    for got, ref, tol, nm in ((y, ref_y, tol_y, "y"), (dpre, ref_d, tol_d, "dpre")):
        err = (got.double().cpu() - ref).abs()
        bad = err > tol + 1e-4 * ref.abs()
        assert not bad.any(), f"{what} {nm} vs fp64: max err {err.max().item():.3e}, {int(bad.sum())} bad"


MODES = ["f32", "bf16x6", "bf16x3"]


@pytest.fixture(scope="module")
def weights(ops):
    w1 = rnd(DFF, D, seed=11, scale=D ** -0.5)
    w2 = rnd(D, DFF, seed=12, scale=0.05)        # linear_2.weight [d, dff]: dgrad reduces over its d rows
    b1 = rnd(DFF, seed=13, scale=0.5)
    flat, (w1g, w2g) = planes_for(ops, [w1, w2])
    yield w1g, b1.to(DEV), w2g
    ops.unregister_planes(flat)


def _mode(ops, name):
    return {"f32": ops.GEMM_F32, "bf16x6": ops.GEMM_BF16X6, "bf16x3": ops.GEMM_BF16X3}[name]


def _keep(ops, M, p, site):
    return ops.dropout_bwd(torch.ones(M, DFF, device=DEV), p, SEED, site) != 0 if p > 0 else \
        torch.ones(M, DFF, dtype=torch.bool, device=DEV)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", [40960, 77])
def test_saved_factor_pair_matches_recomputing_pair(ops, weights, mode, p, M):
    w1, b1, w2 = weights
    x, dy = rnd(M, D, seed=1).to(DEV), rnd(M, D, seed=2).to(DEV)
    keep_mode = ops.gemm_get_mode()
    try:
        ops.gemm_set_mode(_mode(ops, mode))
        out = both_pairs(ops, x, w1, b1, w2, dy, p, site=5)
    finally:
        ops.gemm_set_mode(keep_mode)
    what = f"M={M} {mode} p={p}"
    assert_same(out, what)
    rows = (torch.arange(M) if M < 1024 else torch.randperm(M, generator=torch.Generator().manual_seed(3))[:384]).to(DEV)
    y, dpre = out["new"]
    check_fp64(ops, _mode(ops, mode), y[rows], dpre[rows], x[rows], w1, b1, w2, dy[rows], _keep(ops, M, p, 5)[rows],
               p, what)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pre_full", [False, True])
def test_saved_factor_pair_quad_compacted(ops, weights, mode, p, pre_full):
    """pre_full = False: a compact forward (dropout drawn through the quad map) saves a compact factor, the dgrad runs
    on the same compact rows.  pre_full = True: the forward ran on all rows, the compact dgrad reads the factor
    through the quad map (pre_rows > 0); the padding quads read no factor and their dy rows are zero."""
    w1, b1, w2 = weights
    M_full, n_quads, n_live = 6144, 1536, 701
    ql = quad_list(n_quads, n_live, seed=9)
    Mc = 4 * ql.numel()
    orig = (4 * ql.clamp_min(0).long()[:, None] + torch.arange(4)[None, :]).reshape(-1)   # padding quads: quad 0's mask
    pad = (ql < 0).repeat_interleave(4)
    xf = rnd(M_full, D, seed=21)
    xc = xf[orig].clone()
    xc[pad] = 0.0                                   # LiveRows.gather: padding rows are zero
    dy = rnd(Mc, D, seed=22)
    dy[pad] = 0.0
    qg, dyg = ql.to(DEV), dy.to(DEV)
    keep_mode = ops.gemm_get_mode()
    try:
        ops.gemm_set_mode(_mode(ops, mode))
        if pre_full:
            out = both_pairs(ops, xf.to(DEV), w1, b1, w2, dyg, p, site=6, bwd_map=qg, pre_full=True)
        else:
            out = both_pairs(ops, xc.to(DEV), w1, b1, w2, dyg, p, site=6, fwd_map=qg, bwd_map=qg)
    finally:
        ops.gemm_set_mode(keep_mode)
    what = f"compact {'pre_full' if pre_full else 'fwd'} {mode} p={p}"
    assert_same(out, what)
    y, dpre = out["new"]
    assert not dpre[pad.to(DEV)].any(), f"{what}: padding rows of dpre are not zero"
    live_rows = torch.nonzero(~pad).squeeze(1)
    rows = live_rows[torch.randperm(live_rows.numel(), generator=torch.Generator().manual_seed(4))[:384]]
    keep = _keep(ops, M_full, p, 6)[orig[rows].to(DEV)]
    # compact row r holds original row orig[r]: x is the same there, so the compact fp64 restatement serves both
    # forms; y of the full-row forward is indexed by original rows
    y_rows = y[orig[rows].to(DEV)] if pre_full else y[rows.to(DEV)]
    check_fp64(ops, _mode(ops, mode), y_rows, dpre[rows.to(DEV)], xc[rows], w1, b1, w2, dy[rows], keep, p, what)
