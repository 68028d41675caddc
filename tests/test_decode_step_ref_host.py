"""tests/decode_step_ref.py and the draw reference of tests/rng_ref.py held to themselves, and the inputs of the exact-draw
tests of tests/test_decode_step_kernels_gpu.py shown to discriminate: a draw with a wrong Philox word, a wrong key or a
pick one token off would differ from the reference in most rows, and few rows sit too close to a cumulative boundary to
be decided.  No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from tests import decode_step_ref as D
from tests import rng_ref as R
from tests.test_rng_ref_host import KAT, _philox_scalar


# ------------------------------------------------------------------------------------------------ the uniform
def _u_scalar(x):
    """Plain Python: float32(x >> 8) + 0.5f rounded to float32 (ties to even), times 2^-24 (exact)."""
    return float(np.float32((x >> 8) + 0.5)) * 2.0 ** -24       # (x >> 8) + 0.5 is exact in a double: one rounding


@pytest.mark.parametrize("counter,key,want", KAT)
def test_uniform_of_the_known_answer_words(counter, key, want):
    """The uniform is a function of word x of a Philox call the known answers pin."""
    for w in want:
        assert float(R.draw_uniform_of_word(w)) == _u_scalar(w)
    assert float(R.draw_uniform_of_word(0x6627E8D5)) == (0x6627E8 + 0.5) / 2 ** 24      # below 2^23: exact
    assert float(R.draw_uniform_of_word(0xE169C58D)) == 0xE169C6 / 2 ** 24              # above: .5 rounds to even (up)
    assert float(R.draw_uniform_of_word(0xBC57AC4C)) == 0xBC57AC / 2 ** 24              # even: .5 rounds down


def test_select_uniform_is_word_x_of_the_stated_call():
    for seed in D.SEEDS:
        key = R.rng_key(seed, 0xDEC0DE)
        assert key == (seed & 0xFFFFFFFF, (seed >> 32) ^ ((0xDEC0DE * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF))
        rows = np.array([0, 1, 5, 4095, 1000 + 77])
        for pos in (0, 1, 7, 255):
            got = R.select_uniform(seed, rows, pos)
            assert got.dtype == np.float32
            for r, u in zip(rows, got):
                words = _philox_scalar((int(r), pos, 0x452821E6, 0x38D01377), key)
                assert float(u) == _u_scalar(words[0])
                assert float(R.select_uniform(seed, int(r), pos, word=1)) == _u_scalar(words[1])


def test_uniform_range():
    """u in (0, 1]: the smallest word gives 2^-25, and every x with x >> 8 = 2^24 - 1 gives exactly 1.0."""
    assert float(R.draw_uniform_of_word(0)) == 2.0 ** -25 and float(R.draw_uniform_of_word(255)) == 2.0 ** -25
    assert float(R.draw_uniform_of_word(0xFFFFFF00)) == 1.0 and float(R.draw_uniform_of_word(0xFFFFFFFF)) == 1.0
    assert float(R.draw_uniform_of_word(0xFFFFFE00)) == 1.0 - 2.0 ** -23     # 2^24 - 2 + .5 -> 2^24 - 2 (even)
    assert float(R.draw_uniform_of_word((1 << 31) - 1)) == (2 ** 23 - 0.5) / 2 ** 24    # the last exact one
    u = R.select_uniform(D.SEEDS[1], np.arange(1 << 16), 3)
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) <= 1.0
    n = u.size
    assert abs(float(u.mean()) - 0.5) < 5 / math.sqrt(12 * n)


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_rules():
    w = np.array([[0.0, 2.0, 0.0, 1.0, 1.0, 0.0]])                 # cumulative: 0, .5, .5, .75, 1, 1
    for u, want in [(2.0 ** -25, 1), (0.49, 1), (0.5, 3), (0.74, 3), (0.75, 4), (0.99, 4), (1.0, 4)]:
        pick, gap, lo, hi = R.draw(w, np.array([u]))
        assert int(pick[0]) == want, (u, pick)
    pick, gap, lo, hi = R.draw(w, np.array([0.51]))
    assert gap[0] == pytest.approx(0.01) and (int(lo[0]), int(hi[0])) == (1, 3)
    pick, gap, lo, hi = R.draw(w, np.array([0.98]))
    assert gap[0] == pytest.approx(0.02) and (int(lo[0]), int(hi[0])) == (4, 4)      # the last boundary: one token
    pick, gap, lo, hi = R.draw(np.array([[3.0]]), np.array([1.0]))
    assert int(pick[0]) == 0 and gap[0] == 0.0
    # rows are independent
    w3 = np.array([[1.0, 1.0, 2.0], [0.0, 0.0, 5.0], [1.0, 0.0, 0.0]])
    pick, *_ = R.draw(w3, np.array([0.3, 0.3, 0.3]))
    assert pick.tolist() == [1, 2, 0]


def test_draw_frequencies_match_the_weights():
    """2^16 uniforms of the stream: the pick frequencies equal the weights within 5 standard deviations, and a token of
    weight 0 -- in front, in the middle, at the end -- is never returned."""
    g = np.random.default_rng(3)
    w = g.random(12) ** 3
    w[[0, 5, 11]] = 0.0
    n = 1 << 16
    u = R.select_uniform(D.SEEDS[0], np.arange(n), 1).astype(np.float64)
    pick, *_ = R.draw(np.broadcast_to(w, (n, 12)), u)
    count = np.bincount(pick, minlength=12)
    assert count[[0, 5, 11]].sum() == 0
    p = w / w.sum()
    assert (np.abs(count - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all(), (count, n * p)


# ------------------------------------------------------------------------------------------------ the draw cases
@pytest.mark.parametrize("name", [c[0] for c in D.DRAW_CASES])
def test_draw_cases_discriminate_and_are_decidable(name):
    """For each case of the GPU test and each (seed, position) it runs at: the share of rows within delta(V) of a
    boundary stays within the cap, and the reference picks differ in at least half of the rows from those of a draw
    with (key, pos) swapped, with word y, with pos + 1, and from the picks shifted by one token.  V = 1 has one token
    to pick: no input can tell draws apart there, the case is in for the fallback and the bounds only."""
    _, V, _, filt = D.CASE[name]
    x, w = D.draw_inputs(name)
    assert x.shape == (D.DRAW_ROWS, V) and x.dtype == torch.float32 and w.dtype == np.float64
    n = D.DRAW_ROWS
    rows = np.arange(n)
    for seed, pos in D.combos(V):
        pick, gap, lo, hi = D.reference_draws(w, seed, rows, np.full(n, pos))
        und = int((gap <= D.delta(V)).sum())
        print(f"{name} seed {seed:#x} pos {pos}: {und} of {n} rows undecidable ({100 * und / n:.2f}%)")
        assert und <= D.UNDECIDABLE_CAP * n
        assert (w[rows, pick] > 0).all()
        if V == 1:
            assert (pick == 0).all()
            continue
        wrong = {
            "(key, pos) swapped": D.reference_draws(w, seed, np.full(n, pos), rows)[0],
            "word y": D.reference_draws(w, seed, rows, np.full(n, pos), word=1)[0],
            "pos + 1": D.reference_draws(w, seed, rows, np.full(n, pos + 1))[0],
            "pick shifted by one token": (pick + 1) % V,
        }
        for what, other in wrong.items():
            differ = int((other != pick).sum())
            print(f"    {what}: {differ} rows differ")
            assert differ >= n // 2, (name, what, differ)


def test_draw_cases_are_the_ones_stated():
    assert sorted(c[1] for c in D.PLAIN_CASES) == [1, 30, 64, 65, 257, 1024, 4099]
    assert D.CASE["plain-4099"][2] == 6.0 and all(c[2] == 2.0 for c in D.DRAW_CASES if c[1] != 4099)
    assert [(c[1],) + c[3] for c in D.FILTER_CASES] == [(30, 8, 0.9, 0.8), (65, 12, 0.95, 0.9), (1024, 50, 0.9, 1.2),
                                                        (1024, None, 0.7, 1.0), (200, 3, None, 1.0)]
    assert D.delta(1024) == 32 * 2.0 ** -23 and D.delta(64) == 17 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ attention, embedding
def test_cached_attention_against_a_loop():
    g = torch.Generator().manual_seed(1)
    n, H, dk, L = 3, 2, 4, 5
    q, k, v = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((n, H, dk), (n, L, H, dk), (n, L, H, dk)))
    valid = torch.tensor([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.uint8)
    got = D.cached_attention(q, k, v, valid, 0.5)
    for b in range(n):
        for h in range(H):
            s = [float(q[b, h] @ k[b, j, h]) * 0.5 if valid[b, j] else -1e9 for j in range(L)]
            m = max(s)
            e = [math.exp(t - m) for t in s]
            want = sum(e[j] / sum(e) * v[b, j, h] for j in range(L))
            assert torch.allclose(got[b, h], want, rtol=1e-13, atol=1e-13)
    assert torch.allclose(got[1], v[1].mean(0), rtol=1e-13, atol=1e-13)          # all masked: uniform weights
    assert torch.equal(D.cached_attention(q, k, v, None, 0.5)[2], got[2])


def test_decode_embed_reference_clamps():
    table = torch.arange(12, dtype=torch.float32).view(3, 4)
    pe = torch.arange(40, dtype=torch.float32).view(10, 4) / 8
    ys = torch.tensor([[0, -1], [1, 3], [2, 1 << 40], [1, 1]])
    x, bound = D.decode_embed(ys, torch.tensor([1, 1, 1, 0]), table, pe, 3, 2.0)
    assert torch.equal(x[0], table[0].double() * 2 + pe[4].double())           # -1 -> row 0
    assert torch.equal(x[1], table[2].double() * 2 + pe[4].double())           # vocab -> the last row
    assert torch.equal(x[2], table[2].double() * 2 + pe[4].double())           # 2^40 -> the last row
    assert torch.equal(x[3], table[1].double() * 2 + pe[3].double())
    assert torch.equal(bound, 2.0 ** -23 * ((x - pe.double()[[4, 4, 4, 3]]).abs() + pe.double()[[4, 4, 4, 3]].abs()))


def test_greedy_reference_takes_the_first_maximum():
    x = torch.tensor([[0.0, 3.0, 3.0, 1.0], [-math.inf, -math.inf, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0]])
    first, p = D.greedy(x)
    assert first.tolist() == [1, 2, 0]
    assert torch.allclose(p[2], torch.full((4,), 0.25, dtype=torch.float64)) and p[1, 0] == 0
