"""Host reference of the project's random streams: plain numpy, nothing from the GPU side.  Written from the comments
that state the conventions (csrc/common.h, keep_bits_row in csrc/attention.hip, csrc/vae.hip), not from the kernels;
the device masks and noise are compared with this bit for bit (tests/test_dropout_masks_gpu.py), and the reference
itself is held to the published Philox known answers and to its own statistics in tests/test_rng_ref_host.py.

The rules:
  Philox4x32-10       multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85 (Salmon et al., SC'11)
  key                 (seed_lo, seed_hi ^ (site * 9E3779B9 + 7F4A7C15))
  threshold           thr = floor(float32(p) * 2^32) clamped to [0, 2^32 - 1]; a 16-bit lane is kept iff >= thr >> 16
  16-bit lanes        lane j of a call = half (j & 1) of word (j >> 1): x low, x high, y low, ... w high
  [rows][cols] masks  element (row, col) takes lane (row & 3) * 2 + (col & 1) of the counter
                      (row >> 2, col >> 1, 243F6A88, 85A308D3); under a quad map, row >> 2 is the ORIGINAL quad
  attention           key k = 16 t + 4 g + r of row = (b * H + h) * Lq + q takes lane (t & 1) * 4 + r of the counter
                      (row, 4 * (t >> 1) + g, A4093822, 299F31D0)
  N(0, 1) noise       elements 4 i .. 4 i + 3 from the counter (i, i >> 32, 13198A2E, 03707344): Box-Muller on the pairs
                      (x, y) and (z, w) with u01(v) = ((v >> 8) + 1) / 2^24 in (0, 1]: radius sqrt(-2 ln u01(first)),
                      angle float32(2 pi) * u01(second), outputs (r cos, r sin)
  multinomial draw    (include/gctplus_hip.h, gct_select_token) site DEC0DE; x = word 0 of the counter
                      (key, pos, 452821E6, 38D01377), key = the row (or item_base + item), pos = the token position;
                      u = (float32(x >> 8) + 0.5f) * 2^-24 in float32: the addition rounds to even once
                      x >> 8 >= 2^23, so u lies in (0, 1] (x >> 8 = 2^24 - 1 gives 1.0); the pick is the first token of
                      nonzero weight whose normalised inclusive cumulative sum exceeds u, else the last of nonzero weight
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
DROP_C2, DROP_C3 = 0x243F6A88, 0x85A308D3
ATTN_C2, ATTN_C3 = 0xA4093822, 0x299F31D0
NOISE_C2, NOISE_C3 = 0x13198A2E, 0x03707344
DRAW_C2, DRAW_C3 = 0x452821E6, 0x38D01377
DRAW_SITE = 0xDEC0DE


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words; each an int or an integer array (broadcast together).  Returns the 4 output
    words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = (_u64(c) & _u64(MASK32) for c in counter)
    k0, k1 = (_u64(k) & _u64(MASK32) for k in key)
    m32 = _u64(MASK32)
    for _ in range(10):
        p0 = _u64(M0) * c0                  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = _u64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> _u64(32)) ^ c1 ^ k0) & m32, p1 & m32, ((p0 >> _u64(32)) ^ c3 ^ k1) & m32, p0 & m32
        k0, k1 = (k0 + _u64(W0)) & m32, (k1 + _u64(W1)) & m32
    return c0, c1, c2, c3


def site_word(site):
    return (int(site) * 0x9E3779B9 + 0x7F4A7C15) & MASK32


def rng_key(seed, site):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK32, (seed >> 32) ^ site_word(site)


def drop_threshold(p):
    t = float(np.float32(p)) * 4294967296.0          # exact: a float32 times a power of two
    if t <= 0.0:
        return 0
    if t >= 4294967295.0:
        return 4294967295
    return int(t)


def _lane16(words, lane):
    """The 16-bit lane `lane` (array, 0..7) of the four output words."""
    lane = np.asarray(lane)
    w = np.choose(lane >> 1, words)
    return (w >> _u64(16) * _u64(lane & 1)) & _u64(0xFFFF)


def dropout_lanes(seed, site, rows, cols, quad_of_row=None):
    """(lanes, dead): the 16-bit lane of every element, uint64 [rows, cols], and bool [rows] = the row belongs to a
    negative (padding) quad of quad_of_row.  One Philox call per patch of 4 rows x 2 columns."""
    nq, ncp = (rows + 3) // 4, (cols + 1) // 2
    quad = np.arange(nq, dtype=np.int64) if quad_of_row is None else np.asarray(quad_of_row, dtype=np.int64)[:nq]
    assert quad.shape == (nq,)
    dead = quad < 0
    quad = np.where(dead, 0, quad)[:, None]
    cp = np.arange(ncp, dtype=np.int64)[None, :]
    words = philox4x32_10((quad + 0 * cp, cp + 0 * quad, DROP_C2, DROP_C3), rng_key(seed, site))
    lanes = np.empty((nq, 4, ncp, 2), dtype=np.uint64)          # [quad, row & 3, col >> 1, col & 1]
    for e in range(4):                                          # lane (row & 3) * 2 + (col & 1): word e, low half first
        lanes[:, e, :, 0] = words[e] & _u64(0xFFFF)
        lanes[:, e, :, 1] = words[e] >> _u64(16)
    return lanes.reshape(nq * 4, ncp * 2)[:rows, :cols], np.repeat(dead, 4)[:rows]


def dropout_keep(seed, site, p, rows, cols, quad_of_row=None):
    """bool [rows, cols]: element kept.  quad_of_row (int array [ceil(rows / 4)], optional): the original quad whose
    coordinates the rows 4 i .. 4 i + 3 carry (a quad compaction); negative entries (padding quads) come out False."""
    lanes, dead = dropout_lanes(seed, site, rows, cols, quad_of_row)
    return (lanes >= _u64(drop_threshold(p) >> 16)) & ~dead[:, None]


def attn_keep(seed, site, p, B, H, Lq, Lk):
    """bool [B, H, Lq, Lk]: probability kept."""
    row = np.arange(B * H * Lq, dtype=np.int64)[:, None]
    k = np.arange(Lk, dtype=np.int64)[None, :]
    t, g, r = k >> 4, (k >> 2) & 3, k & 3
    words = philox4x32_10((row + 0 * k, 4 * (t >> 1) + g + 0 * row, ATTN_C2, ATTN_C3), rng_key(seed, site))
    keep = _lane16(words, (t & 1) * 4 + r + 0 * row) >= _u64(drop_threshold(p) >> 16)
    return keep.reshape(B, H, Lq, Lk)


def _u01(v):
    return ((v >> _u64(8)).astype(np.float64) + 1.0) / 16777216.0


def reparam_eps(seed, site, n):
    """float64 [n]: the N(0, 1) noise of reparam_fwd(eps=None)."""
    i = np.arange((n + 3) // 4, dtype=np.uint64)
    x, y, z, w = philox4x32_10((i & _u64(MASK32), i >> _u64(32), NOISE_C2, NOISE_C3), rng_key(seed, site))
    two_pi = float(np.float32(6.283185307179586))
    out = np.empty((len(i), 4), dtype=np.float64)
    for j, (a, b) in enumerate(((x, y), (z, w))):
        rad, ang = np.sqrt(-2.0 * np.log(_u01(a))), two_pi * _u01(b)
        out[:, 2 * j], out[:, 2 * j + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(-1)[:n]


def draw_uniform_of_word(x):
    """float32 array: u = (float32(x >> 8) + 0.5f) * 2^-24, every operation in float32 (the sum rounds to even once
    x >> 8 >= 2^23, so the largest words give exactly 1.0)."""
    hi = (_u64(x) >> _u64(8)).astype(np.float32)                # exact: at most 24 bits
    return (hi + np.float32(0.5)) * np.float32(2.0 ** -24)


def select_uniform(seed, key, pos, word=0):
    """float32 array: the uniform of the multinomial draw keyed (key, pos) under `seed` (ints or integer arrays).  word: the
    Philox output word to take -- the draw takes word 0 (x); the others exist for the tests that show a wrong word would
    be noticed."""
    words = philox4x32_10((np.asarray(key, dtype=np.int64), np.asarray(pos, dtype=np.int64), DRAW_C2, DRAW_C3),
                          rng_key(seed, DRAW_SITE))
    return draw_uniform_of_word(words[word])


def draw(weights, u):
    """weights float64 [n, V] (>= 0, not all 0 in a row), u [n] -> (pick, gap, lo, hi), int64 / float64 [n].
    pick: the first token c with w_c > 0 whose normalised inclusive cumulative sum exceeds u; when there is none, the last
    token of nonzero weight.  gap: the distance from u to the nearest cumulative boundary of a nonzero-weight token --
    lo is that token and hi the next token of nonzero weight behind it (lo itself when it is the last): an evaluation of
    the sums in another precision or order may move a row whose gap is small from one of the two to the other, and to no
    third token."""
    w = np.asarray(weights, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 1)
    n, V = w.shape
    nz = w > 0
    assert nz.any(1).all() and (w >= 0).all()
    cum = np.cumsum(w / w.sum(1, keepdims=True), axis=1)
    idx = np.arange(V)[None, :]
    last = np.where(nz, idx, -1).max(1)
    hit = nz & (cum > u)
    pick = np.where(hit.any(1), hit.argmax(1), last)
    dist = np.where(nz, np.abs(cum - u), np.inf)
    lo = dist.argmin(1)
    gap = dist[np.arange(n), lo]
    behind = nz & (idx > lo[:, None])
    hi = np.where(behind.any(1), behind.argmax(1), lo)
    return pick.astype(np.int64), gap, lo.astype(np.int64), hi.astype(np.int64)
