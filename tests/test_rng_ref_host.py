"""tests/rng_ref.py held to the published Philox4x32-10 known answers and to the statistics a dropout mask must have.
No GPU, no library: tests/test_dropout_masks_gpu.py holds the kernels to this reference bit for bit, after which these
statistics are the kernels' own."""
import math

import numpy as np
import pytest

from tests import rng_ref as R

# (counter, key, output): the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _philox_scalar(counter, key):
    """Plain Python integers, one call: the direct restatement the array version is checked against."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = R.M0 * c[0], R.M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & R.MASK32, (p0 >> 32) ^ c[3] ^ k[1], p0 & R.MASK32]
        k = [(k[0] + R.W0) & R.MASK32, (k[1] + R.W1) & R.MASK32]
    return tuple(c)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == want
    assert _philox_scalar(counter, key) == want


def test_philox_array_form_equals_the_scalar_form():
    g = np.random.default_rng(5)
    ctr = g.integers(0, 1 << 32, size=(4, 50), dtype=np.uint64)
    key = (0x12345678, 0x9ABCDEF0)
    got = R.philox4x32_10(tuple(ctr), key)
    for i in range(50):
        assert tuple(int(w[i]) for w in got) == _philox_scalar([int(c) for c in ctr[:, i]], key)


def test_rng_key():
    assert R.rng_key(0, 0) == (0, 0x7F4A7C15)
    assert R.rng_key((0xDEADBEEF << 32) | 0x01234567, 3) == (0x01234567, 0xDEADBEEF ^ ((3 * 0x9E3779B9 + 0x7F4A7C15) & R.MASK32))


def test_drop_threshold():
    assert R.drop_threshold(0.0) == 0
    assert R.drop_threshold(0.25) == 1 << 30 and R.drop_threshold(0.5) == 1 << 31
    assert R.drop_threshold(0.1) >> 16 == 6553                 # float32(0.1) = 0.100000001490116: floor(p * 2^16) = 6553
    assert R.drop_threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32) == 429496736
    assert R.drop_threshold(0.9) >> 16 == 58982                # float32(0.9) = 0.899999976158142
    assert R.drop_threshold(2.0 ** -17) == 1 << 15 and R.drop_threshold(2.0 ** -17) >> 16 == 0
    assert R.dropout_keep(77, 1, 2.0 ** -17, 64, 64).all()      # below one 16-bit step: nothing is dropped
    assert R.dropout_keep(77, 1, 0.0, 64, 64).all()
    assert R.drop_threshold(-1.0) == 0 and R.drop_threshold(1.0) == 4294967295


def _within(count, n, prob, what):
    sd = math.sqrt(n * prob * (1 - prob))
    assert abs(count - n * prob) <= 5 * sd, f"{what}: {count} of {n}, expected {n * prob:.0f} +- {5 * sd:.0f}"


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5, 0.9])
def test_keep_rate(p):
    rows, cols = 1024, 512
    keep = R.dropout_keep((5 << 32) | 1234, 7, p, rows, cols)
    _within(int(keep.sum()), rows * cols, 1 - (R.drop_threshold(p) >> 16) / 65536, f"keep rate at p = {p}")
    B, H, Lq, Lk = 4, 4, 128, 256
    keep = R.attn_keep((5 << 32) | 1234, 7, p, B, H, Lq, Lk)
    _within(int(keep.sum()), keep.size, 1 - (R.drop_threshold(p) >> 16) / 65536, f"attention keep rate at p = {p}")


def test_sites_are_uncorrelated():
    rows, cols, seed = 256, 256, (9 << 32) | 42
    masks = [R.dropout_keep(seed, s, 0.5, rows, cols) for s in range(16)]
    for i in range(16):
        for j in range(i + 1, 16):
            _within(int((masks[i] == masks[j]).sum()), rows * cols, 0.5, f"agreement of sites {i} and {j}")


@pytest.mark.parametrize("bit", [0, 31, 32, 47, 63])
def test_every_seed_bit_changes_the_stream(bit):
    """Seeds that differ in one bit -- bit 0, bit 31 (the top of the low word), and bits of the high word, which a
    32-bit truncation of the seed would ignore -- give masks that agree on half of the elements."""
    rows, cols, seed = 256, 256, (0x1234 << 32) | 0x89ABCDEF
    a = R.dropout_keep(seed, 3, 0.5, rows, cols)
    b = R.dropout_keep(seed ^ (1 << bit), 3, 0.5, rows, cols)
    _within(int((a == b).sum()), rows * cols, 0.5, f"agreement across seed bit {bit}")
    an, bn = R.reparam_eps(seed, 3, 4096), R.reparam_eps(seed ^ (1 << bit), 3, 4096)
    assert abs(float(np.corrcoef(an, bn)[0, 1])) < 5 / math.sqrt(4096)


def test_the_documented_collision():
    """key word 1 is seed_hi ^ f(site): (seed, site) and (seed ^ ((f(site) ^ f(site')) << 32), site') are one stream.
    Stated so that nobody takes seeds that differ only in the high word for independent across sites."""
    seed, s0, s1 = (0xCAFE << 32) | 17, 2, 9
    twin = seed ^ ((R.site_word(s0) ^ R.site_word(s1)) << 32)
    assert twin != seed and R.rng_key(seed, s0) == R.rng_key(twin, s1)
    assert np.array_equal(R.dropout_keep(seed, s0, 0.5, 64, 64), R.dropout_keep(twin, s1, 0.5, 64, 64))
    assert not np.array_equal(R.dropout_keep(seed, s0, 0.5, 64, 64), R.dropout_keep(seed, s1, 0.5, 64, 64))


def test_one_call_serves_a_patch_of_4_rows_by_2_columns():
    """The 8 lanes of the call at (quad, col >> 1) are the 8 elements of the patch, x low first; a quad map moves whole
    quads and drops the negative ones."""
    seed, site = (3 << 32) | 5, 4
    keep = R.dropout_keep(seed, site, 0.5, 8, 6)
    th = R.drop_threshold(0.5) >> 16
    for quad in range(2):
        for cp in range(3):
            w = _philox_scalar((quad, cp, R.DROP_C2, R.DROP_C3), R.rng_key(seed, site))
            for e in range(4):
                assert bool(keep[4 * quad + e, 2 * cp]) == ((w[e] & 0xFFFF) >= th)
                assert bool(keep[4 * quad + e, 2 * cp + 1]) == ((w[e] >> 16) >= th)
    full = R.dropout_keep(seed, site, 0.5, 40, 6)
    moved = R.dropout_keep(seed, site, 0.5, 12, 6, quad_of_row=[9, -1, 2])
    assert np.array_equal(moved[0:4], full[36:40]) and not moved[4:8].any() and np.array_equal(moved[8:12], full[8:12])


def test_attention_lanes():
    seed, site, B, H, Lq, Lk = (3 << 32) | 5, 4, 2, 2, 3, 40
    keep = R.attn_keep(seed, site, 0.5, B, H, Lq, Lk)
    th = R.drop_threshold(0.5) >> 16
    for row in (0, 7, B * H * Lq - 1):
        b, h, q = row // (H * Lq), (row // Lq) % H, row % Lq
        for k in range(Lk):
            t, g, r = k // 16, (k // 4) % 4, k % 4
            w = _philox_scalar((row, 4 * (t >> 1) + g, R.ATTN_C2, R.ATTN_C3), R.rng_key(seed, site))
            lane = (t & 1) * 4 + r
            assert bool(keep[b, h, q, k]) == (((w[lane >> 1] >> (16 * (lane & 1))) & 0xFFFF) >= th)


def test_reparam_noise_moments_and_layout():
    e = R.reparam_eps(42, 1, 1 << 18)
    n = e.size
    assert abs(e.mean()) < 5 / math.sqrt(n) and abs(e.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs((e ** 4).mean() - 3) < 5 * math.sqrt(96 / n)
    assert np.array_equal(R.reparam_eps(42, 1, 6), e[:6])          # a tail of 2 is the head of the next quad
    x, y, _, _ = _philox_scalar((1, 0, R.NOISE_C2, R.NOISE_C3), R.rng_key(42, 1))
    rad = math.sqrt(-2 * math.log(((x >> 8) + 1) / 2 ** 24))
    ang = float(np.float32(6.283185307179586)) * ((y >> 8) + 1) / 2 ** 24
    assert e[4] == pytest.approx(rad * math.cos(ang), abs=1e-14) and e[5] == pytest.approx(rad * math.sin(ang), abs=1e-14)
