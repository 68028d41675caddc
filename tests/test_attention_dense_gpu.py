"""The dense forms of gct_attn_mask_pack / gct_attn_fwd / gct_attn_bwd against tests/attention_ref.py (fp64, CPU) on
every route -- direct, LDS 8 tiles, LDS 13 tiles, forward 8 with backward 13 -- and head dim, through raw library calls
into buffers that start as NaN (o, lse, probs, dq, dk, dv, bits, tiles, the backward's workspace):

  A  mask packing: the packed bits and the tile words, exactly
  B  forward and backward under masks whose visible key tiles have gaps (`left`, `band`, `blocks`), with and
     without dropout (keep bits from the host Philox reference), rows and a whole sample that see no key, lse included
  C  more than two rounds of (batch, head) pairs per persistent workgroup of the LDS kernels, sized from
     gct_attn_route on the live device, every pair compared
  D  the direct kernels with the tile words given and with tbits = NULL: bit for bit the same

Tolerances (tests/attention_ref.py): probs 1e-6 + 1e-5 |ref|, o 1e-5 + 1e-5 |ref|, gradients 2e-5 + 1e-4 |ref| (3e-5
under dropout) -- those of test_attention / test_attention_dropout.  lse: |err| <= 3.624e-6 (1 + |ref|) = 8 x 4.53e-7,
the worst error of torch.logsumexp in fp32 against fp64 measured over all cases of B and C (rows that see no key must
give log(Lk) to the same bound).  A and D are exact.  tests/test_attention_ref_host.py shows that the inputs of B tell
a kernel's likely mistakes apart by >= 100 x these tolerances."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import attention_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}                       # worst error / tolerance per (section, family, quantity), printed at the end
SIZES_C = {}


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib
    yield _lib.load()
    for key in sorted(WORST):
        print(f"[attention dense] worst err / tol  {key}: {WORST[key]:.3f}")
    for key, val in SIZES_C.items():
        print(f"[attention dense] section C {key}: {val}")


def _check(rc, what):
    from gct_plus_amd import _lib
    _lib.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def nanf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def nani(*shape):
    """int32 words that hold the bits of a float NaN: a word the kernel does not write is no plausible mask word"""
    return nanf(*shape).view(torch.int32)


def route(lib, bwd, Lq, Lk, dk, npairs, cus=0):
    out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    _check(lib.gct_attn_route(int(bwd), Lq, Lk, dk, npairs, cus, ctypes.addressof(out)), "gct_attn_route")
    return tuple(out)


class Packed:
    """gct_attn_mask_pack of a uint8 mask [B, Lk] or [B, Lq, Lk] into NaN-filled words; `tiles=False`: no tile words."""

    def __init__(self, lib, mask_u8, B, Lq, Lk, tiles=True):
        self.mask = mask_u8.to(DEV).contiguous()
        pad = self.mask.dim() == 2
        rows, ntr = (1, 1) if pad else (Lq, (Lq + 15) // 16)
        self.bits, self.tiles = nani(B, rows, 8), nani(B, ntr)
        self.sb, self.sq = rows * 8, (0 if pad else 8)
        self.t_sb, self.t_su = ntr, (0 if pad else 1)
        self.use_tiles = tiles
        _check(lib.gct_attn_mask_pack(self.mask.data_ptr(), Lk if pad else Lq * Lk, 0 if pad else Lk, B, Lq, Lk,
                                      self.bits.data_ptr(), self.tiles.data_ptr(), _st()), "gct_attn_mask_pack")

    def margs(self):
        return self.bits.data_ptr(), self.sb, self.sq

    def targs(self):
        return (self.tiles.data_ptr(), self.t_sb, self.t_su) if self.use_tiles else (None, 0, 0)


def fwd(lib, q, k, v, ldq, ldkv, pk, o, ldo, B, H, Lq, Lk, dk, p, seed, site, probs=True):
    """raw gct_attn_fwd into NaN-filled lse / probs (o is the caller's, NaN-filled too); returns (lse, probs)"""
    lse = nanf(B, H, Lq)
    pr = nanf(B, H, Lq, Lk) if probs else None
    m = pk.margs() if pk is not None else (None, 0, 0)
    t = pk.targs() if pk is not None else (None, 0, 0)
    _check(lib.gct_attn_fwd(q.data_ptr(), ldq, k.data_ptr(), ldkv, v.data_ptr(), ldkv, *m, o.data_ptr(), ldo,
                            lse.data_ptr(), None if pr is None else pr.data_ptr(), B, H, Lq, Lk, dk, 1 / math.sqrt(dk),
                            p, seed, site, None, None, *t, None, None, _st()), "gct_attn_fwd")
    return lse, pr


def bwd(lib, q, k, v, ldq, ldkv, pk, o, do, ldo, lse, dq, dk_, dv, lddq, lddkv, B, H, Lq, Lk, dk, p, seed, site):
    """raw gct_attn_bwd; the direct kernels' workspace starts as 0xFF bytes (NaN as floats)"""
    need = int(lib.gct_attn_bwd_ws_bytes(B, H, Lq, Lk))
    ws = torch.full((max(need, 16),), 255, dtype=torch.uint8, device=DEV)
    m = pk.margs() if pk is not None else (None, 0, 0)
    t = pk.targs() if pk is not None else (None, 0, 0)
    _check(lib.gct_attn_bwd(q.data_ptr(), ldq, k.data_ptr(), ldkv, v.data_ptr(), ldkv, *m, o.data_ptr(), do.data_ptr(),
                            ldo, lse.data_ptr(), dq.data_ptr(), lddq, dk_.data_ptr(), lddkv, dv.data_ptr(), lddkv,
                            B, H, Lq, Lk, dk, 1 / math.sqrt(dk), p, seed, site, None, None, 0, None, None, *t,
                            ws.data_ptr() if need else None, need, _st()), "gct_attn_bwd")
    torch.cuda.synchronize()


def _worst(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


def check(key, what, got, ref, tol):
    r = A.ratio(got, ref, tol)
    print(f"  {key} {what}: err / tol {r:.3f}")
    _worst(f"{key} {what}", r)
    assert r <= 1.0, f"{key} {what}: worst error is {r:.2f} x the tolerance {tol}"


def check_lse(key, got, ref):
    r = A.lse_ratio(got, ref)
    print(f"  {key} lse: err / tol {r:.3f}")
    _worst(f"{key} lse", r)
    assert r <= 1.0, f"{key} lse: worst |err| / (1 + |ref|) is {r:.2f} x {A.TOL_LSE:.3e}"


# ------------------------------------------------------------------------------------------------ A: mask packing
SHAPES_A = [(1, 1, 1), (3, 17, 31), (2, 16, 32), (2, 33, 33), (3, 5, 96), (2, 97, 97), (2, 208, 208), (1, 20, 256)]


def _patterns(B, Lq, Lk):
    g = torch.Generator().manual_seed(1000 * Lq + Lk)
    k, q = torch.arange(Lk), torch.arange(Lq)
    out = {"ones": torch.ones(B, Lq, Lk, dtype=torch.uint8), "zeros": torch.zeros(B, Lq, Lk, dtype=torch.uint8)}
    for name, dens in (("half", 0.5), ("sparse", 0.05)):
        m = (torch.rand(B, Lq, Lk, generator=g) < dens).to(torch.uint8)
        m[:, ::3] = 0                                              # some all-zero rows (row 0 among them)
        out[name] = m
    centre = (q * Lk) // Lq
    out["band"] = ((k[None, :] - centre[:, None]).abs() <= 3).to(torch.uint8)[None].repeat(B, 1, 1)
    n = torch.tensor([(21 * (b + 1)) % (Lk + 1) for b in range(B)])
    out["left"] = (k[None, None, :] >= n[:, None, None]).to(torch.uint8).repeat(1, Lq, 1)
    vals = (torch.rand(B, Lq, Lk, generator=g) < 0.3).to(torch.uint8)
    out["values"] = vals * torch.where(torch.rand(B, Lq, Lk, generator=g) < 0.5, 2, 255).to(torch.uint8)
    return out


@pytest.mark.parametrize("B,Lq,Lk", SHAPES_A)
def test_mask_pack_bits_and_tile_words_exact(lib, B, Lq, Lk):
    for name, m in _patterns(B, Lq, Lk).items():
        for form in (m, m[:, Lq // 2].contiguous()):              # [B, Lq, Lk] and the key-padding form [B, Lk]
            pk = Packed(lib, form, B, Lq, Lk)
            torch.cuda.synchronize()
            bits = pk.bits.cpu().numpy().view(np.uint32)
            tiles = pk.tiles.cpu().numpy().view(np.uint32)
            want_bits = A.pack_bits(form.numpy(), Lk).reshape(bits.shape)
            assert np.array_equal(bits, want_bits), f"{name} {tuple(form.shape)}: packed bits"
            assert np.array_equal(tiles, A.tile_words(form.numpy())), f"{name} {tuple(form.shape)}: tile words"


def test_mask_pack_of_a_slice_of_a_wider_buffer_and_of_no_sample(lib):
    B, Lq, Lk = 3, 17, 31
    m = _patterns(B, Lq, Lk)["half"]
    wide = torch.full((B, Lq * Lk + 13), 1, dtype=torch.uint8)      # what lies between the samples is visible: it would show
    wide[:, :Lq * Lk] = m.reshape(B, -1)
    wg = wide.to(DEV)
    bits, tiles = nani(B, Lq, 8), nani(B, 2)
    _check(lib.gct_attn_mask_pack(wg.data_ptr(), Lq * Lk + 13, Lk, B, Lq, Lk, bits.data_ptr(), tiles.data_ptr(), _st()),
           "gct_attn_mask_pack")
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), A.pack_bits(m.numpy(), Lk))
    assert np.array_equal(tiles.cpu().numpy().view(np.uint32), A.tile_words(m.numpy()))
    # B = 0: OK, and nothing is written
    bits0, tiles0 = nani(2, Lq, 8), nani(2, 2)
    assert lib.gct_attn_mask_pack(wg.data_ptr(), Lq * Lk + 13, Lk, 0, Lq, Lk, bits0.data_ptr(), tiles0.data_ptr(), _st()) == 0
    assert lib.gct_attn_mask_pack(wg.data_ptr(), Lk, 0, 0, Lq, Lk, bits0.data_ptr(), tiles0.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits0, nani(2, Lq, 8)) and torch.equal(tiles0, nani(2, 2))


# ------------------------------------------------------------------------------------------------ B: every route
FUSED = {(2, 2, 96, 96, 32), (2, 2, 100, 100, 16), (1, 2, 208, 208, 32)}     # q | k | v in one [B L, 3d] buffer, dq | dk | dv too
WIDE_O = {(2, 3, 40, 37, 16), (2, 2, 120, 97, 64), (2, 2, 60, 203, 64)}      # o (and dO) rows of d + 8 columns


class Buffers:
    """The device operands of one case in its layout: fused (ld 3d in and out), or q alone and k | v interleaved
    (ld d and 2d, the cross-attention layout); o / dO rows of d columns, or d + 8 with NaN behind the d."""

    def __init__(self, shape, q, k, v, do, fused, wide):
        B, H, Lq, Lk, dk = shape
        d = self.d = H * dk
        if fused:
            assert Lq == Lk
            buf = torch.cat([q, k, v], 1).to(DEV)
            self.q, self.k, self.v, self.ldq, self.ldkv = buf, buf[:, d:], buf[:, 2 * d:], 3 * d, 3 * d
            g = nanf(B * Lq, 3 * d)
            self.dq, self.dk, self.dv, self.lddq, self.lddkv = g, g[:, d:], g[:, 2 * d:], 3 * d, 3 * d
        else:
            self.q, kv = q.to(DEV), torch.cat([k, v], 1).to(DEV)
            self.k, self.v, self.ldq, self.ldkv = kv, kv[:, d:], d, 2 * d
            self.dq, gkv = nanf(B * Lq, d), nanf(B * Lk, 2 * d)
            self.dk, self.dv, self.lddq, self.lddkv = gkv, gkv[:, d:], d, 2 * d
        self.ldo = d + 8 if wide else d
        self.o = nanf(B * Lq, self.ldo)
        self.do = nanf(B * Lq, self.ldo)
        self.do[:, :d] = do.to(DEV)

    def grads(self):
        d = self.d
        return self.dq[:, :d], self.dk[:, :d], self.dv[:, :d]


def _run_case(lib, key, shape, mask, p, do=None, fused=False, wide=False, seed=1, chunk=64, keep_fn=None):
    """forward (with probs where they fit) and backward of one case against the fp64 reference"""
    B, H, Lq, Lk, dk = shape
    d = H * dk
    q, k, v, do_ = A.make_inputs(B, H, Lq, Lk, dk, seed=seed)
    do = do_ if do is None else do
    mf = None if mask is None else A.full_mask(mask, B, Lq, Lk)
    keep = None
    if p:
        keep = keep_fn if keep_fn is not None else A.attn_keep(A.DROP_SEED, A.DROP_SITE, p, B, H, Lq, Lk)
    want_probs = B * H * Lq * Lk <= 1 << 22
    ref = A.attention_with_grads(A.heads(q, B, Lq, H, dk), A.heads(k, B, Lk, H, dk), A.heads(v, B, Lk, H, dk), mf,
                                 1 / math.sqrt(dk), A.heads(do, B, Lq, H, dk), keep, 1 - p, chunk=chunk,
                                 want_probs=want_probs)
    bf = Buffers(shape, q, k, v, do, fused, wide)
    pk = None if mask is None else Packed(lib, mask, B, Lq, Lk)
    lse, pr = fwd(lib, bf.q, bf.k, bf.v, bf.ldq, bf.ldkv, pk, bf.o, bf.ldo, B, H, Lq, Lk, dk, p, A.DROP_SEED, A.DROP_SITE,
                  probs=want_probs)
    torch.cuda.synchronize()
    if want_probs:
        check(key, "probs", pr, ref["probs"], A.TOL_PROBS)
    check(key, "o", bf.o[:, :d], A.unheads(ref["o"]), A.TOL_O)
    check_lse(key, lse, ref["lse"])
    if wide:
        assert torch.isnan(bf.o[:, d:]).all(), f"{key}: the forward wrote behind its {d} output columns"
    bwd(lib, bf.q, bf.k, bf.v, bf.ldq, bf.ldkv, pk, bf.o, bf.do, bf.ldo, lse, bf.dq, bf.dk, bf.dv, bf.lddq, bf.lddkv,
        B, H, Lq, Lk, dk, p, A.DROP_SEED, A.DROP_SITE)
    gtol = A.TOL_GRAD_DROP if p else A.TOL_GRAD
    for name, got in zip(("dq", "dk", "dv"), bf.grads()):
        check(key, name, got, A.unheads(ref[name]), gtol)


@pytest.mark.parametrize("p", [0.0, A.DROP_P])
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("shape", list(A.CASES_B))
def test_forward_backward_under_gapped_masks(lib, shape, family, p):
    B, H, Lq, Lk, dk = shape
    kinds = (route(lib, 0, Lq, Lk, dk, B * H)[0], route(lib, 1, Lq, Lk, dk, B * H)[0])
    assert kinds == A.CASES_B[shape], f"{shape}: routes {kinds}"
    names = {(0, 0): "direct", (1, 1): "lds8", (2, 2): "lds13", (1, 2): "lds8/13"}
    key = f"B {names[kinds]} {family} p={p}"
    print(f"{shape} {family} p={p}")
    _run_case(lib, key, shape, A.make_mask(family, B, Lq, Lk), p, fused=shape in FUSED, wide=shape in WIDE_O)


@pytest.mark.parametrize("pattern", ["tile", "row", "sample"])
@pytest.mark.parametrize("shape", [(2, 2, 100, 100, 16), (2, 2, 130, 129, 16), (2, 2, 150, 100, 64)])
def test_lds_backward_with_zero_gradient_tiles(lib, shape, pattern):
    """dO rows that are zero: a whole 16-row query tile (skipped by both phases), a tile with one non-zero row (not
    skipped), a whole sample; under the `band` mask and dropout."""
    B, H, Lq, Lk, dk = shape
    assert route(lib, 1, Lq, Lk, dk, B * H)[0] in (1, 2)
    _, _, _, do = A.make_inputs(B, H, Lq, Lk, dk)
    do = do.view(B, Lq, H * dk).clone()
    if pattern == "tile":
        do[0, 32:48] = 0
        do[1, 16 * ((Lq - 1) // 16):] = 0                          # the ragged last tile
    elif pattern == "row":
        do[0, 16:32] = 0
        do[0, 21, 5] = 0.75
        do[1, 0:16] = 0
        do[1, 15, H * dk - 1] = -1.5
    else:
        do[1] = 0
    _run_case(lib, f"B zero-dO {pattern}", shape, A.make_mask("band", B, Lq, Lk), A.DROP_P, do=do.view(B * Lq, H * dk))


# ------------------------------------------------------------------------------------------------ C: many pairs
@pytest.mark.parametrize("Lq,Lk,dk,p", A.CASES_C)
def test_lds_kernels_walk_several_pairs_per_workgroup(lib, Lq, Lk, dk, p):
    """More than two rounds of pairs on the persistent grids of forward and backward (proved by gct_attn_route on this
    device): the second and third pair of a workgroup run on prefetched K / V / Q / mask rows and re-staged LDS regions.
    Causal-and-ragged mask with a length per sample, independent inputs per sample, whole samples without gradient."""
    H = A.H_C
    f, b = route(lib, 0, Lq, Lk, dk, 1 << 30), route(lib, 1, Lq, Lk, dk, 1 << 30)
    assert f[0] in (1, 2) and b[0] in (1, 2)
    B = A.batch_c(f[1], b[1])
    npairs = B * H
    fg, bg = route(lib, 0, Lq, Lk, dk, npairs)[1], route(lib, 1, Lq, Lk, dk, npairs)[1]
    assert npairs > 2 * max(fg, bg), (npairs, fg, bg)
    nbytes = 4 * H * dk * B * (5 * Lq + 4 * Lk) + B * Lq * Lk + 8 * 64 * H * Lq * Lk * 8
    if nbytes > 2 << 30:
        pytest.skip(f"{npairs} pairs for grids {fg} / {bg} would need {nbytes >> 20} MB")
    SIZES_C[(Lq, Lk, dk, p)] = f"kinds {f[0]} / {b[0]}, grids {fg} / {bg}, B {B}, pairs {npairs}"
    print(SIZES_C[(Lq, Lk, dk, p)])
    shape = (B, H, Lq, Lk, dk)
    _, _, _, do = A.make_inputs(B, H, Lq, Lk, dk, seed=3)
    do = do.view(B, Lq, H * dk).clone()
    do[3::5] = 0                                                   # samples without gradient, among those with
    keep_fn = (lambda b0, b1: A.attn_keep(A.DROP_SEED, A.DROP_SITE, p, B, H, Lq, Lk, b0, b1)) if p else None
    _run_case(lib, f"C {Lq}x{Lk} dk={dk} p={p}", shape, A.causal_ragged_mask(B, Lq, Lk), p, do=do.view(B * Lq, H * dk),
              seed=3, keep_fn=keep_fn)


# ------------------------------------------------------------------------------------------------ D: tbits or none
@pytest.mark.parametrize("form", ["left", "left3", "band"])
@pytest.mark.parametrize("shape", [(3, 2, 40, 37, 16), (2, 2, 96, 96, 32), (4, 2, 81, 90, 64)])
def test_direct_kernels_with_and_without_tile_words(lib, shape, form):
    """tbits = NULL: every wave computes the word gct_attn_mask_pack would have given it; o, lse, dq, dk, dv bit for bit."""
    B, H, Lq, Lk, dk = shape
    d = H * dk
    assert route(lib, 0, Lq, Lk, dk, B * H)[0] == 0 and route(lib, 1, Lq, Lk, dk, B * H)[0] == 0
    mask = A.make_mask("band" if form == "band" else "left", B, Lq, Lk)
    if form == "left3":                                            # the same key padding, given per query row
        mask = mask[:, None, :].repeat(1, Lq, 1)
    q, k, v, do = A.make_inputs(B, H, Lq, Lk, dk, seed=5)
    got = []
    for tiles in (True, False):
        pk = Packed(lib, mask, B, Lq, Lk, tiles=tiles)
        bf = Buffers(shape, q, k, v, do, fused=False, wide=False)
        lse, _ = fwd(lib, bf.q, bf.k, bf.v, bf.ldq, bf.ldkv, pk, bf.o, bf.ldo, B, H, Lq, Lk, dk, A.DROP_P, 9, 2, probs=False)
        bwd(lib, bf.q, bf.k, bf.v, bf.ldq, bf.ldkv, pk, bf.o, bf.do, bf.ldo, lse, bf.dq, bf.dk, bf.dv, bf.lddq, bf.lddkv,
            B, H, Lq, Lk, dk, A.DROP_P, 9, 2)
        got.append((bf.o, lse) + bf.grads())
    for name, x, y in zip(("o", "lse", "dq", "dk", "dv"), *got):
        assert not torch.isnan(x).any(), f"{name}: not everything was written"
        assert torch.equal(x, y), f"{name} differs between tbits given and NULL"
