"""Every kernel that draws a dropout mask or N(0, 1) noise against tests/rng_ref.py, the host restatement of the
conventions documented in csrc/common.h, csrc/attention.hip (keep_bits_row) and csrc/vae.hip.  Masks are compared
exactly.  They are recovered so that a kept element cannot read as a dropped one: the inputs are ones (or one-hot), or
the run is repeated with another bias (tests/test_gemm_tile_end_gpu.py: an element that is zero in both runs was
dropped).  Outputs are filled with NaN before the call."""
import math

import numpy as np
import pytest
import torch

from tests import rng_ref as R
from tests.test_kernels_gpu import _planes_for, rnd
from tests.test_loss_optim_edges_gpu import embed_fwd, nans, ratio, reparam_fwd
from tests.test_rowwise_compact_gpu import PLANS, _plan

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = [(0x1234 << 32) | 99, 0xFEDCBA9876543210]          # both above 2^32: the high word is part of the key
SITES = [0, 7]
PS = [0.1, 0.5, 0.9]


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def _same_mask(got, want, what):
    got, want = torch.as_tensor(got).cpu(), torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} mask elements differ, first at {bad.nonzero()[0].tolist()}"


def _kept_values(y, keep, p, what):
    """Dropped elements are exactly 0; kept ones (the input was 1) are 1 / (1 - p) to one fp32 ulp."""
    y = y.cpu()
    assert torch.isfinite(y).all(), f"{what}: an element was not written"
    _same_mask(y != 0, keep, what)
    want = 1.0 / (1.0 - float(np.float32(p)))
    ulp = float(np.spacing(np.float32(want)))
    kept = y[torch.as_tensor(keep)].double()
    if kept.numel():
        assert float((kept - want).abs().max()) <= ulp, f"{what}: kept values off by more than 1 ulp of {want}"


# ------------------------------------------------------------------------------------------- dropout_bwd
# 1025 quads x 1030 columns = 1 055 750 threads: more than the 4096 x 256 of the grid, threads go round again
@pytest.mark.parametrize("rows,cols", [(13, 7), (4, 1), (1030, 512), (4100, 258), (4100, 1030)])
def test_dropout_bwd_dense(ops, rows, cols):
    ones = torch.ones(rows, cols, device=DEV)
    for seed in SEEDS:
        for site in SITES:
            lanes, _ = R.dropout_lanes(seed, site, rows, cols)
            for p in PS + [2.0 ** -17]:
                buf = nans(rows + 4, cols)
                ops.dropout_bwd(ones, p, seed, site, out=buf[:rows])
                keep = lanes >= np.uint64(R.drop_threshold(p) >> 16)
                _kept_values(buf[:rows], keep, p, f"dropout_bwd {rows}x{cols} p={p} seed={seed:#x} site={site}")
                assert torch.isnan(buf[rows:]).all(), "wrote behind the last row"
                if p == 2.0 ** -17:
                    assert keep.all()                # below one 16-bit step: everything is kept


def test_dropout_bwd_values_on_a_random_gradient(ops):
    """dy = dout / (1 - p) where kept (1e-6 relative, the existing bound), exactly 0 where dropped."""
    rows, cols, p = 1030, 258, 0.1
    dout = rnd(rows, cols, seed=3)
    dy = nans(rows, cols)
    ops.dropout_bwd(dout.to(DEV), p, SEEDS[0], 7, out=dy)
    keep = torch.as_tensor(R.dropout_keep(SEEDS[0], 7, p, rows, cols))
    ref = torch.where(keep, dout.double() / (1 - float(np.float32(p))), torch.zeros(rows, cols, dtype=torch.double))
    ratio(dy, ref, 1e-30, 1e-6, "dropout_bwd values")
    assert not dy.cpu()[~keep].any()


@pytest.mark.parametrize("d", [7, 258])
def test_dropout_bwd_under_a_quad_map_equals_the_reference(ops, d):
    """Compact quad i carries the mask of original quad quad_list[i]; the padding quads (-1) hold zeros."""
    p, seed, site = 0.2, SEEDS[1], 6
    for B, T, n in PLANS:
        L, ref, orig = _plan(ops, B, T, n)
        gc = (orig >= 0).to(torch.float32)[:, None].expand(L.Mc, d).contiguous().to(DEV)   # what gather(ones) holds:
        #                                              ones on the rows of the live quads, zeros on padding and past M
        buf = nans(L.Mc + 4, d)
        ops.dropout_bwd(gc, p, seed, site, out=buf[:L.Mc], live=L)
        quads = ref["quad_list"][:L.Mc // 4].numpy()
        keep = R.dropout_keep(seed, site, p, L.Mc, d, quad_of_row=quads) & (orig >= 0).numpy()[:, None]
        assert (quads < 0).any() or B == 1
        _kept_values(buf[:L.Mc], keep, p, f"dropout_bwd(live) d={d} plan={n}")
        assert torch.isnan(buf[L.Mc:]).all()


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("n_c,B,S", [(0, 3, 7), (0, 5, 3), (3, 3, 4), (3, 5, 4)])
@pytest.mark.parametrize("d", [64, 260])
def test_embedding_masks(ops, n_c, B, S, d):
    """B * (S + n_c) % 4 is 1 and 3: the last quad is ragged.  table = 0 and pe = 1: every kept output is 1 / (1 - p)."""
    V, p, seed, site = 30, 0.3, SEEDS[0], 11
    rows = B * (S + n_c)
    assert rows % 4 in (1, 3)
    tok = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(1))
    table, pe = torch.zeros(V, d, device=DEV), torch.ones(S + n_c, d, device=DEV)
    cond = torch.zeros(B, n_c, d, device=DEV) if n_c else None
    out = embed_fwd(ops, tok.to(DEV), table, cond, pe, n_c, math.sqrt(d), p, seed, site, d, V)
    keep = R.dropout_keep(seed, site, p, rows, d)
    _kept_values(out, keep, p, f"embed_pe_fwd B={B} S={S} n_c={n_c} d={d}")
    # backward of a gradient of ones: dtable = scale / (1 - p) * (kept rows added up per token id)
    scale = float(np.float32(math.sqrt(d)))
    kk = torch.as_tensor(keep).double().view(B, S + n_c, d) * scale / (1 - float(np.float32(p)))
    exp = torch.zeros(V, d, dtype=torch.double)
    exp.index_add_(0, tok.reshape(-1), kk[:, n_c:].reshape(-1, d))
    dtable = nans(V, d)
    dcond = nans(B, n_c, d) if n_c else None
    ops.embed_pe_bwd(torch.ones(rows, d, device=DEV), tok.to(DEV), dtable, dcond, n_c, math.sqrt(d), p, seed, site)
    ratio(dtable, exp, 1e-4, 1e-5, "embed_pe_bwd dtable under the reference mask")
    if n_c:
        ratio(dcond, kk[:, :n_c], 1e-5, 1e-5, "embed_pe_bwd dcond under the reference mask")
        _same_mask(dcond.cpu() != 0, torch.as_tensor(keep).view(B, S + n_c, d)[:, :n_c], "dcond mask")


# ------------------------------------------------------------------------------------------ GEMM epilogues
# (M, K, N, ldy): the wide bf16x6 tile with its tail launch (test_linear_bf16x6_epilogues_and_dropout_masks), the
# 64 x 128 bf16x6 tile (test_linear_bf16x6_small_tile_kernel), the panel kernel (test_linear_panel_kernel_small_problems)
# and a narrow output in a wider buffer (test_linear_narrow_output_panel_kernel; with a dropout epilogue the planner sends
# it to the 32 x 32 panel or the general kernel).  Each has a ragged last row tile.
@pytest.mark.parametrize("M,K,N,ldy", [(128 * 66 + 40, 512, 1024, 1024), (2050, 1024, 520, 520), (77, 512, 64, 64),
                                       (33, 512, 32, 36)])
def test_linear_epilogue_masks(ops, M, K, N, ldy):
    p, seed = 0.1, SEEDS[1]
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    xg = x.to(DEV)
    biases = [b.to(DEV), (b + 8.0).to(DEV)]            # x.w + b is N(0, 2): with b + 8 no GELU saturates to zero
    zero = torch.zeros(M, ldy, device=DEV)
    want = {site: ~torch.as_tensor(R.dropout_keep(seed, site, p, M, N)) for site in (3, 4)}
    flat, (wg,) = _planes_for(ops, [w])
    try:
        for mode in (ops.GEMM_F32, ops.GEMM_BF16X6):
            ops.gemm_set_mode(mode)
            for epi, site in ((ops.EPI_GELU_DROP, 3), (ops.EPI_DROP_RESID, 4)):
                dropped = torch.ones(M, N, dtype=torch.bool)
                for bias in biases:
                    y, pre = nans(M, ldy), nans(M, ldy)
                    if epi == ops.EPI_GELU_DROP:
                        ops.linear_fwd(xg, [wg], [bias], [y], ldy, epi=epi, pre=pre, p=p, seed=seed, site=site)
                    else:
                        ops.linear_fwd(xg, [wg], [bias], [y], ldy, epi=epi, resid=zero, p=p, seed=seed, site=site)
                    yh = y.cpu()
                    assert torch.isfinite(yh[:, :N]).all() and torch.isnan(yh[:, N:]).all()
                    dropped &= yh[:, :N] == 0
                _same_mask(dropped, want[site], f"linear_fwd M={M} K={K} N={N} mode={mode} epi={epi}: dropped elements")
    finally:
        ops.gemm_set_mode(ops.GEMM_BF16X6)
        ops.unregister_planes(flat)


# ----------------------------------------------------------------------------------------------- norm_bwd
@pytest.mark.parametrize("d", [12, 768])
def test_norm_bwd_drop_output(ops, d):
    """norm_bwd(drop=(buffer, p, seed, site)): buffer = dx * keep / (1 - p) with the reference mask.  Against the dx
    the same call returns: exactly 0 where dropped, and 2^-22 relative where kept (the scale 1 / (1 - p) carries two
    roundings, the product a third: 1.5 ulp)."""
    rows, p, seed, site = 9, 0.2, SEEDS[0], 6
    x, a, b, dy = rnd(rows, d, seed=1), rnd(d, seed=2) + 1, rnd(d, seed=3), rnd(rows, d, seed=4)
    xg, ag, bg = x.to(DEV), a.to(DEV), b.to(DEV)
    _, mean, rstd = ops.norm_fwd(xg, ag, bg)
    da, db = nans(d), nans(d)
    buf, out = nans(rows + 1, d), nans(rows + 1, d)
    dx = ops.norm_bwd(dy.to(DEV), xg, ag, mean, rstd, da, db, out=out[:rows], drop=(buf[:rows], p, seed, site)).cpu()
    keep = torch.as_tensor(R.dropout_keep(seed, site, p, rows, d))
    got = buf[:rows].cpu()
    assert torch.isfinite(dx).all() and torch.isfinite(got).all()
    assert torch.isnan(buf[rows:]).all() and torch.isnan(out[rows:]).all()
    nz = dx != 0
    _same_mask((got != 0)[nz], keep[nz], f"norm_bwd drop output d={d}")
    assert not got[~keep].any() and not got[~nz].any()
    ref = torch.where(keep, dx.double() / (1 - float(np.float32(p))), torch.zeros(rows, d, dtype=torch.double))
    ratio(got, ref, 1e-45, 2.0 ** -22, f"norm_bwd drop values d={d}")


# ---------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("L", [48, 170])
def test_attention_mask(ops, L):
    """The one-hot-V recovery of test_attention_dropout: the output columns are the dropped probabilities of 64 keys per
    run.  Wherever the probability before dropout is not zero, kept <=> the reference says so."""
    B, H, dk, p, seed, site = 2, 2, 64, 0.25, SEEDS[1], 3
    d = H * dk
    qg, kg = rnd(B * L, d, seed=1).to(DEV), rnd(B * L, d, seed=2).to(DEV)
    pd = torch.full((B, H, L, L), float("nan"))
    for k0 in range(0, L, dk):
        eye = torch.zeros(B, L, H, dk)
        for i in range(k0, min(L, k0 + dk)):
            eye[:, i, :, i - k0] = 1.0
        out = nans(B * L, d)
        o, _, probs = ops.attn_fwd(qg, kg, eye.view(B * L, d).to(DEV), d, d, d, None, B, H, L, L, dk, p, seed, site,
                                   out=out, want_probs=True)
        n = min(L, k0 + dk) - k0
        pd[..., k0:k0 + n] = o.view(B, L, H, dk).transpose(1, 2)[..., :n].cpu()
    pr = probs.cpu()
    assert torch.isfinite(pd).all()
    keep = torch.as_tensor(R.attn_keep(seed, site, p, B, H, L, L))
    seen = pr != 0
    assert seen.float().mean() > 0.99
    _same_mask((pd != 0)[seen], keep[seen], f"attn_fwd L={L}")
    assert not pd[~keep].any()
    ratio(pd, torch.where(keep, pr.double() / (1 - p), torch.zeros_like(pr, dtype=torch.double)), 1e-6, 1e-5, "dropped probs")


# ------------------------------------------------------------------------------------------ reparam noise
@pytest.mark.parametrize("n", [1, 6, 4099, (1 << 20) + 3])
def test_reparam_noise(ops, n):
    """eps_out against the reference within 1e-5, derived: u01 is exact in fp32; the angle 2 pi_f32 * u rounded to fp32 is
    off by at most 2.4e-7; the radius is at most sqrt(48 ln 2) = 5.77; with a few ulp for logf, sqrtf and sincosf the
    error is at most 3e-6, and the bound leaves a margin of 3."""
    mu, lv = rnd(n, seed=1), rnd(n, seed=2, scale=0.5)
    for seed, site in ((42, 1), (SEEDS[1], 7)):
        z, eo = reparam_fwd(ops, mu.to(DEV), lv.to(DEV), None, seed, site)
        ref = torch.as_tensor(R.reparam_eps(seed, site, n))
        r0 = ratio(eo, ref, 1e-5, 0.0, f"reparam noise n={n} seed={seed:#x} site={site}")
        r1 = ratio(z, eo.cpu().double() * torch.exp(0.5 * lv.double()) + mu.double(), 1e-6, 1e-6, f"z n={n}")
        print(f"reparam noise n={n}: worst error / tolerance eps {r0:.3f}, z {r1:.3f}")
        if n > (1 << 20):                                # the moment checks of test_reparam_kld_ce
            e2 = eo.double()
            assert abs(e2.mean().item()) < 5e-3 and abs(e2.std().item() - 1) < 5e-3
            assert abs((e2 ** 4).mean().item() - 3) < 0.05
    other = reparam_fwd(ops, mu.to(DEV), lv.to(DEV), None, 42, 2)[1]
    assert n < 4 or not torch.equal(other, reparam_fwd(ops, mu.to(DEV), lv.to(DEV), None, 42, 1)[1])
