"""tests/attention_ref.py held to independent restatements (F.softmax, torch.logsumexp, bit loops written the slow way),
the inputs of tests/test_attention_dense_gpu.py shown to discriminate -- a kernel that masks key tile 0, takes the
previous sample's mask or K rows, or draws the keep bits of another site moves the output and every gradient by at least
100 x the tolerance the GPU test applies -- and the attention planner's table through gct_attn_route with an explicit
number of compute units.  No GPU: gct_attn_route launches nothing."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as A

SHAPES_A = [(1, 1, 1), (3, 17, 31), (2, 16, 32), (2, 33, 33), (3, 5, 96), (2, 97, 97), (2, 208, 208), (1, 20, 256)]


# ------------------------------------------------------------------------------------------------ the references
def _bits_slow(row, Lk):
    words = [0] * 8
    for k in range(256):
        if k < Lk and k < len(row) and row[k] != 0:
            words[k >> 5] |= 1 << (k & 31)
    return words


@pytest.mark.parametrize("B,Lq,Lk", SHAPES_A)
def test_pack_bits_against_a_bit_loop(B, Lq, Lk):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    m = (torch.rand(B, Lq, Lk + 3, generator=g) < 0.5).to(torch.uint8) * 7     # keys beyond Lk must not show
    got = A.pack_bits(m.numpy(), Lk)
    assert got.dtype == np.uint32 and got.shape == (B, Lq, 8)
    for b in range(B):
        for q in range(Lq):
            assert got[b, q].tolist() == _bits_slow(m[b, q].tolist(), Lk)
    assert A.pack_bits(m[:, 0].numpy(), Lk).tolist() == got[:, 0].tolist()     # [B, Lk] form: the same rule per row


def _tiles_slow(m):
    """The rule of include/gctplus_hip.h, element by element."""
    if m.ndim == 2:
        m = m[:, None, :]
    B, Lq, Lk = m.shape
    out = []
    for b in range(B):
        row = []
        for u in range((Lq + 15) // 16):
            real = range(16 * u, min(Lq, 16 * u + 16))
            blind = any(all(m[b, q, k] == 0 for k in range(Lk)) for q in real)
            word = 0
            for t in range((Lk + 15) // 16):
                seen = any(m[b, q, k] != 0 for q in real for k in range(16 * t, min(Lk, 16 * t + 16)))
                if blind or seen:
                    word |= 1 << t
            row.append(word)
        out.append(row)
    return out


@pytest.mark.parametrize("B,Lq,Lk", [s for s in SHAPES_A if s[1] * s[2] <= 97 * 97])
def test_tile_words_against_the_rule_written_out(B, Lq, Lk):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk + 1)
    m = (torch.rand(B, Lq, Lk, generator=g) < 0.04).to(torch.uint8)
    m[:, Lq // 2] = 0                                              # a row that sees nothing
    m[0, :, 0] = 1
    assert A.tile_words(m.numpy()).tolist() == _tiles_slow(m.numpy())
    assert A.tile_words(m[:, 0].numpy()).tolist() == _tiles_slow(m[:, 0].numpy())
    assert A.tile_words(m[:, 0].numpy()).shape == (B, 1)


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("shape", list(A.CASES_B))
def test_tile_words_cover_the_visible_tiles(shape, family):
    """A superset of the tiles a real row sees; equal to `all tiles` exactly when a real row sees nothing; and the
    families give what they are for: an invisible tile 0, gaps, single-bit words, rows and a sample that see nothing."""
    B, H, Lq, Lk, dk = shape
    m = A.make_mask(family, B, Lq, Lk).numpy()
    words = A.tile_words(m)
    m3 = m[:, None, :] if m.ndim == 2 else m
    nkt, full = (Lk + 15) // 16, (1 << ((Lk + 15) // 16)) - 1
    for b in range(B):
        for u in range(words.shape[1]):
            rows = m3[b, 16 * u:16 * u + 16] != 0
            vis = sum(1 << t for t in range(nkt) if rows[:, 16 * t:16 * t + 16].any())
            w = int(words[b, u])
            assert w & vis == vis and w >> nkt == 0
            blind = not rows.any(1).all()
            assert (w == full and vis != full) == (blind and vis != full)
            assert blind or w == vis
    w0 = [int(x) for x in words[0]]
    if family == "left":
        assert w0[0] & 1 == 0 and w0[0] != 0                       # tile 0 invisible, later ones visible
        assert B == 1 or (not m[1].any() and int(words[1, 0]) == full)
    elif family == "band":
        blind_rows = (~(m != 0).any(2)).sum(1)
        assert (blind_rows == 2).all()
        inner = [int(w) for w in words.reshape(-1) if w != full]
        assert any(w & 1 == 0 for w in inner) and any(w >> (nkt - 1) == 0 for w in inner)
        blind_tiles = {int(r) // 16 for r in (~(m[0] != 0).any(1)).nonzero()[0]}
        assert len(blind_tiles) == 2 and all(w0[u] == full for u in blind_tiles)   # in different query tiles
    else:
        assert all(bin(w).count("1") == 1 for w in w0)
        assert [w.bit_length() - 1 for w in w0] == [(5 * u + 3) % nkt for u in range(len(w0))]


def test_attention_reference_against_softmax_and_logsumexp():
    B, H, Lq, Lk, dk = 2, 2, 35, 37, 16
    q, k, v, do = A.make_inputs(B, H, Lq, Lk, dk, seed=9)
    qd, kd, vd = A.heads(q, B, Lq, H, dk), A.heads(k, B, Lk, H, dk), A.heads(v, B, Lk, H, dk)
    m = A.make_mask("band", B, Lq, Lk)
    mf = A.full_mask(m, B, Lq, Lk)
    keep = A.attn_keep(1, 2, 0.2, B, H, Lq, Lk)
    scale = 1 / math.sqrt(dk)
    o, pr, lse = A.attention(qd, kd, vd, mf, scale, keep, 0.8)
    s = (torch.einsum("bhqd,bhkd->bhqk", qd, kd) * scale).masked_fill(~mf, -1e9)
    assert torch.allclose(pr, F.softmax(s, -1), rtol=1e-13, atol=1e-300)
    assert torch.allclose(o, (F.softmax(s, -1) * keep / 0.8) @ vd, rtol=1e-12, atol=1e-14)
    sees = mf.expand(B, H, Lq, Lk).any(-1)
    assert (~sees).sum() == 2 * B * H
    assert torch.allclose(lse[sees], torch.logsumexp(s, -1)[sees], rtol=1e-13, atol=1e-13)
    assert (lse[~sees] == math.log(Lk)).all()
    assert torch.allclose(pr[~sees], torch.full((1,), 1 / Lk, dtype=torch.float64))
    # the chunked form with gradients equals one autograd pass over everything
    ref = [t.clone().requires_grad_() for t in (qd, kd, vd)]
    dod = A.heads(do, B, Lq, H, dk)
    A.attention(*ref, mf, scale, keep, 0.8)[0].backward(dod)
    got = A.attention_with_grads(qd, kd, vd, mf, scale, dod, keep, 0.8, chunk=1, want_probs=True)
    for name, want in (("o", o), ("probs", pr), ("lse", lse), ("dq", ref[0].grad), ("dk", ref[1].grad), ("dv", ref[2].grad)):
        assert torch.equal(got[name], want), name
    # key-padding form and no mask at all
    ml = A.make_mask("left", B, Lq, Lk)
    o2, pr2, lse2 = A.attention(qd, kd, vd, A.full_mask(ml, B, Lq, Lk), scale)
    s2 = (torch.einsum("bhqd,bhkd->bhqk", qd, kd) * scale).masked_fill(ml[:, None, None, :] == 0, -1e9)
    assert torch.allclose(pr2, F.softmax(s2, -1), rtol=1e-13, atol=1e-300)
    assert (lse2[1] == math.log(Lk)).all() and torch.allclose(lse2[0], torch.logsumexp(s2, -1)[0], rtol=1e-13)
    o3, _, lse3 = A.attention(qd, kd, vd, None, scale)
    assert torch.allclose(lse3, torch.logsumexp(s.new_tensor(0) + torch.einsum("bhqd,bhkd->bhqk", qd, kd) * scale, -1))


def test_keep_bits_by_sample_range_equal_the_rng_reference():
    from tests import rng_ref
    for (B, H, Lq, Lk, p) in ((3, 2, 5, 37, 0.2), (2, 1, 17, 208, 0.1), (2, 2, 3, 96, 0.5)):
        want = torch.from_numpy(rng_ref.attn_keep(77, 5, p, B, H, Lq, Lk))
        assert torch.equal(A.attn_keep(77, 5, p, B, H, Lq, Lk), want)
        assert torch.equal(A.attn_keep(77, 5, p, B, H, Lq, Lk, 1, 2), want[1:2])
        assert torch.equal(A.attn_keep(77, 5, p, B, H, Lq, Lk, 1, 9), want[1:])
        assert 0.5 * (1 - p) < float(want.float().mean()) < min(1.0, 1.5 * (1 - p))


def test_lse_tolerance_is_the_measured_fp32_error():
    """A.LSE_FP32_ERR bounds what torch.logsumexp in fp32 loses against fp64 on the section B cases (rows that see a
    key); the larger section C cases, sized for 256 compute units, were measured the same way and set the constant."""
    worst = 0.0
    for (B, H, Lq, Lk, dk) in A.CASES_B:
        q, k, _, _ = A.make_inputs(B, H, Lq, Lk, dk)
        for family in A.FAMILIES:
            mf = A.full_mask(A.make_mask(family, B, Lq, Lk), B, Lq, Lk)
            s32 = (A.heads(q, B, Lq, H, dk).float() @ A.heads(k, B, Lk, H, dk).float().transpose(-1, -2)) / math.sqrt(dk)
            s64 = (A.heads(q, B, Lq, H, dk) @ A.heads(k, B, Lk, H, dk).transpose(-1, -2)) / math.sqrt(dk)
            l32 = torch.logsumexp(s32.masked_fill(~mf, -1e9), -1).double()
            l64 = torch.logsumexp(s64.masked_fill(~mf, -1e9), -1)
            sees = mf.expand(B, H, Lq, Lk).any(-1)
            worst = max(worst, float(((l32 - l64).abs() / (1 + l64.abs()))[sees].max()))
    print(f"fp32 logsumexp vs fp64, section B: {worst:.3e} (LSE_FP32_ERR {A.LSE_FP32_ERR:.3e})")
    assert A.LSE_FP32_ERR / 4 <= worst <= A.LSE_FP32_ERR
    assert A.TOL_LSE == 8 * A.LSE_FP32_ERR


# ------------------------------------------------------------------------------------------------ discrimination
def _first_tile_masked(mf):
    """Mistake (a): key tile 0 treated as masked -- in a sample whose rows all have tile 0 masked already (`left`), the
    first key tile one of its rows sees."""
    out = mf.clone()
    for b in range(mf.shape[0]):
        cols = mf[b].any(0).any(0).nonzero()
        if cols.numel():
            t0 = int(cols[0]) // 16
            out[b, :, :, 16 * t0:16 * t0 + 16] = False
    return out


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("shape", list(A.CASES_B))
def test_section_b_inputs_tell_kernel_mistakes_apart(shape, family):
    B, H, Lq, Lk, dk = shape
    q, k, v, do = A.make_inputs(B, H, Lq, Lk, dk)
    qd, kd, vd, dod = A.heads(q, B, Lq, H, dk), A.heads(k, B, Lk, H, dk), A.heads(v, B, Lk, H, dk), A.heads(do, B, Lq, H, dk)
    mf = A.full_mask(A.make_mask(family, B, Lq, Lk), B, Lq, Lk)
    scale = 1 / math.sqrt(dk)
    for p in (0.0, A.DROP_P):
        keep = A.attn_keep(A.DROP_SEED, A.DROP_SITE, p, B, H, Lq, Lk) if p else None
        right = A.attention_with_grads(qd, kd, vd, mf, scale, dod, keep, 1 - p)
        # with one sample "the previous sample" is the sample itself: its previous (batch, head) PAIR stands in for (c),
        # and there is no other mask for (b)
        prev_k = kd.roll(1, 0) if B > 1 else kd.roll(1, 1)
        wrong = {"a: key tile 0 masked": A.attention_with_grads(qd, kd, vd, _first_tile_masked(mf), scale, dod, keep, 1 - p),
                 "c: previous K rows": A.attention_with_grads(qd, prev_k, vd, mf, scale, dod, keep, 1 - p)}
        if B > 1:
            wrong["b: previous mask"] = A.attention_with_grads(qd, kd, vd, mf.roll(1, 0), scale, dod, keep, 1 - p)
        if p:
            k1 = A.attn_keep(A.DROP_SEED, A.DROP_SITE + 1, p, B, H, Lq, Lk)
            wrong["d: keep bits of site + 1"] = A.attention_with_grads(qd, kd, vd, mf, scale, dod, k1, 1 - p)
        gtol = A.TOL_GRAD_DROP if p else A.TOL_GRAD
        for name, w in wrong.items():
            for what, tol in (("o", A.TOL_O), ("dq", gtol), ("dk", gtol), ("dv", gtol)):
                moved = A.ratio(w[what], right[what], tol)
                assert moved >= 100, f"{shape} {family} p={p}: mistake ({name}) moves {what} by only {moved:.1f} x tol"


# ------------------------------------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def route():
    from gct_plus_amd import _lib
    lib = _lib.load()

    def call(bwd, Lq, Lk, dk, npairs, cus=256):
        out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
        _lib.check(lib.gct_attn_route(int(bwd), Lq, Lk, dk, npairs, cus, ctypes.addressof(out)), "gct_attn_route")
        return tuple(out)
    return call


DIRECT, LDS8, LDS13 = 0, 1, 2


def test_route_kinds_at_the_thresholds(route):
    for dk in (16, 32, 64):
        for bwd in (0, 1):
            assert route(bwd, 50, 96, dk, 64)[0] == DIRECT and route(bwd, 50, 97, dk, 64)[0] == LDS8
            assert route(bwd, 208, 96, dk, 64)[0] == DIRECT             # by the keys alone, forward and backward
            assert route(bwd, 128, 128, dk, 64)[0] == LDS8 and route(bwd, 129, 129, dk, 64)[0] == LDS13
            assert route(bwd, 100, 144, dk, 64)[0] == LDS13 and route(bwd, 100, 208, dk, 64)[0] == LDS13
        # padded lengths 128 / 144: the forward goes by Lk, the backward by max(Lq, Lk)
        assert route(0, 129, 128, dk, 64)[0] == LDS8 and route(1, 129, 128, dk, 64)[0] == LDS13
        assert route(0, 208, 97, dk, 64)[0] == LDS8 and route(1, 208, 97, dk, 64)[0] == LDS13
        assert route(0, 128, 113, dk, 64)[0] == LDS8 and route(1, 128, 113, dk, 64)[0] == LDS8
        assert route(0, 5, 129, dk, 64)[0] == LDS13 and route(1, 5, 129, dk, 64)[0] == LDS13
    for shape, kinds in A.CASES_B.items():
        B, H, Lq, Lk, dk = shape
        assert (route(0, Lq, Lk, dk, B * H)[0], route(1, Lq, Lk, dk, B * H)[0]) == kinds, shape


def test_route_grids(route):
    for npairs in (0, 1, 5, 511, 512, 513, 4000):
        for (Lq, Lk) in ((1, 1), (40, 37), (96, 96), (81, 90), (208, 96)):
            nqt, nkt = (Lq + 15) // 16, (Lk + 15) // 16
            assert route(0, Lq, Lk, 32, npairs) == (DIRECT, (npairs * nqt + 3) // 4, 0, 0)
            assert route(1, Lq, Lk, 32, npairs) == (DIRECT, (npairs * nqt + 3) // 4, (npairs * nkt + 3) // 4, 0)
        for (Lq, Lk) in ((100, 100), (20, 100), (130, 130), (208, 208), (208, 97)):
            for dk in (16, 32, 64):
                for bwd in (0, 1):
                    kind, grid, grid_kv, lds = route(bwd, Lq, Lk, dk, npairs)
                    assert grid <= npairs and grid_kv == 0 and (grid > 0 or npairs == 0)
                    assert grid == min(npairs, route(bwd, Lq, Lk, dk, 1 << 30)[1])
    # the persistent grids scale with the compute units and never exceed 6 workgroups per unit
    for cus in (1, 64, 256, 304):
        for dk in (16, 32, 64):
            for (Lq, Lk) in ((100, 100), (130, 130), (208, 208)):
                f, b = route(0, Lq, Lk, dk, 1 << 30, cus)[1], route(1, Lq, Lk, dk, 1 << 30, cus)[1]
                assert f % cus == 0 and b % cus == 0 and 1 <= f // cus <= 2 and 2 <= b // cus <= 6


def test_route_lds_bytes_over_every_admitted_shape(route):
    """Dynamic LDS <= 160 KB everywhere; above 64 KB only on the LDS kernels, whose launches opt in (launch_lds ->
    ensure_lds; the direct kernels use none); the bytes are those of the layout the kernels' comments state."""
    for dk in (16, 32, 64):
        for Lq in range(1, 209):
            for Lk in range(1, 209):
                for bwd in (0, 1):
                    kind, _, _, lds = route(bwd, Lq, Lk, dk, 1000)
                    if kind == DIRECT:
                        assert lds == 0 and Lk <= 96
                        continue
                    LQP, LKP = (Lq + 15) & ~15, (Lk + 15) & ~15
                    if bwd:
                        LMX, MW = max(LQP, LKP), (4 if kind == LDS8 else 7)
                        want = 2 * LMX * (dk + 4) * 4 + LQP * 8 + LQP * MW * 8 + LQP * 2
                        assert (kind == LDS8) == (LMX <= 128)
                    else:
                        want = 2 * LKP * (dk + 4) * 4
                        assert (kind == LDS8) == (LKP <= 128)
                    assert lds == want and lds <= 160 * 1024
                    assert lds > 64 * 1024 or dk < 64 or max(LQP, LKP) < 128 or not bwd


def test_route_refuses_bad_arguments(route):
    from gct_plus_amd import _lib
    for args in ((0, 0, 10, 16, 1), (0, 10, 209, 16, 1), (1, 209, 10, 16, 1), (0, 10, 10, 48, 1), (0, 10, 10, 16, -1)):
        with pytest.raises(_lib.GctError, match="attn_route"):
            route(*args)
    lib = _lib.load()
    assert lib.gct_attn_route(0, 10, 10, 16, 1, 256, None) != 0
    assert route(0, 100, 100, 16, 1 << 20, 0)[1] > 0                # cus <= 0: the device's own count (256 without one)
