"""Host side of molecule interpolation (gct_plus_amd/Inference/mol_interpolation.py) and the statistics of the host
reference's normals (tests/latent_ref.py).  No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd.Inference import mol_interpolation as MI
from tests import latent_ref as LR


# ------------------------------------------------------------------------------------------------------- slerp
@pytest.mark.parametrize("as_torch", [False, True])
def test_slerp_closed_form_on_orthogonal_unit_vectors(as_torch):
    u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    for alpha in (0.1, 0.25, 0.5, 0.9):
        want = np.array([math.cos(alpha * math.pi / 2), math.sin(alpha * math.pi / 2), 0.0])
        got = MI.slerp(torch.tensor(u), torch.tensor(v), alpha).numpy() if as_torch else MI.slerp(u, v, alpha)
        assert np.allclose(got, want, rtol=0, atol=1e-15)


def test_slerp_endpoints_and_batches():
    g = np.random.default_rng(3)
    u, v = g.normal(size=(5, 7)), g.normal(size=(5, 7))
    assert np.allclose(MI.slerp(u, v, 0.0), u, rtol=1e-14, atol=0) and np.allclose(MI.slerp(u, v, 1.0), v, rtol=1e-14, atol=0)
    rows = np.stack([MI.slerp(u[i], v[i], 0.3) for i in range(5)])             # the last axis is the vector
    assert np.array_equal(MI.slerp(u, v, 0.3), rows)
    assert np.allclose(MI.slerp(torch.tensor(u), torch.tensor(v), 0.3).numpy(), rows, rtol=1e-14, atol=0)
    # not renormalised, as the reference: the norm of the midpoint of two vectors of different length lies between
    long = 3.0 * v
    mid = np.linalg.norm(MI.slerp(u, long, 0.5), axis=-1)
    assert np.all(mid > 0) and not np.allclose(mid, np.linalg.norm(u, axis=-1))


@pytest.mark.parametrize("as_torch", [False, True])
def test_slerp_guard_takes_the_lerp_and_is_finite(as_torch):
    u = np.array([0.3, -1.2, 2.0, 0.5])
    wrap = (lambda x: torch.tensor(x)) if as_torch else (lambda x: x)
    for v, alpha in ((u.copy(), 0.1), (-u, 0.25), (np.zeros(4), 0.7), (2.0 * u, 0.9)):
        got = np.asarray(MI.slerp(wrap(u), wrap(v), alpha))
        assert np.all(np.isfinite(got))
        assert np.allclose(got, MI.lerp(u, v, alpha), rtol=0, atol=1e-15)
    assert np.array_equal(np.asarray(MI.slerp(wrap(u), wrap(u.copy()), 0.1)), u)          # u == v: u exactly
    got = np.asarray(MI.slerp(wrap(np.zeros(4)), wrap(u), 0.4))
    assert np.allclose(got, 0.4 * u, rtol=0, atol=1e-15)
    # just inside the threshold the slerp branch runs: c = cos(0.01) < 1 - 2^-20
    v = np.array([math.cos(0.01), math.sin(0.01)])
    got = MI.slerp(np.array([1.0, 0.0]), v, 0.5)
    assert np.allclose(got, [math.cos(0.005), math.sin(0.005)], rtol=0, atol=1e-12)
    assert MI.SLERP_MAX_COS == LR.SLERP_MAX_COS == 1 - 2.0 ** -20


# -------------------------------------------------------------------------------------------------------- plan
def test_interp_plan_toklen_moves_from_the_first_length_to_the_second():
    alphas = MI.interior_alphas(3)
    assert np.allclose(alphas, [0.25, 0.5, 0.75])
    tl = MI.interp_plan([10, 30, 12], [30, 10, 12], alphas)
    assert tl.tolist() == [[15, 20, 25], [25, 20, 15], [12, 12, 12]]
    # the reference's interpolate_z_pair takes the first length twice: it would give 10, 10, 10 for the first pair
    assert tl[0].tolist() != [int(MI.lerp(10, 10, a)) for a in alphas]
    for p, (l0, l1) in enumerate(((10, 30), (30, 10), (12, 12))):
        assert tl[p].tolist() == [int(MI.lerp(l0, l1, a)) for a in alphas]
    assert MI.interp_plan([7], [8], [0.99]).tolist() == [[7]]                   # int() truncates


def test_interp_plan_scaffold_rows():
    alphas = MI.interior_alphas(2)
    assert MI.interp_plan([9, 20], [12, 20], alphas, extras=[8, 5]).shape == (2, 2)      # 9 rows >= 8 + 1
    with pytest.raises(ValueError, match="prefix"):
        MI.interp_plan([8, 20], [8, 20], alphas, extras=[8, 5])                 # 8 rows for a prefix of 8 and a molecule
    with pytest.raises(ValueError):
        MI.interp_plan([8, 20], [8], alphas)
    with pytest.raises(ValueError):
        MI.interp_plan([0], [4], alphas)
    with pytest.raises(ValueError):
        MI.interior_alphas(0)


# ------------------------------------------------------------------------------------------------------ ladder
def test_noise_ladder_is_the_reference_schedule():
    lad = MI.noise_ladder()
    # the reference's loop: two tries per standard deviation, +0.005 after every second one, exit at >= 1.0
    want, std, count = [], 0, 0
    while True:
        want.append(std)
        if (count + 1) % 2 == 0:
            std += 0.005
        if std >= 1.0:
            break
        count += 1
    assert lad.tolist() == want and len(lad) == 400
    assert lad[0] == lad[1] == 0 and lad[2] == lad[3] == 0.005 and lad[-1] < 1.0 and abs(lad[-1] - 0.995) < 1e-12
    assert np.all(np.diff(lad) >= 0)
    assert MI.noise_ladder(0.25, 1, 1.0).tolist() == [0.0, 0.25, 0.5, 0.75]
    assert MI.noise_ladder(0.5, 3, 1.0).tolist() == [0.0] * 3 + [0.5] * 3
    with pytest.raises(ValueError):
        MI.noise_ladder(0.0)


def test_first_accepted():
    flags = np.zeros((2, 3, 5), dtype=bool)
    flags[0, 1, [2, 4]] = True
    flags[1, 0, 0] = True
    flags[1, 2, 4] = True
    assert MI.first_accepted(flags).tolist() == [[-1, 2, -1], [0, -1, 4]]
    assert MI.first_accepted(np.zeros((1, 1, 0), dtype=bool)).tolist() == [[-1]]


# ------------------------------------------------------------------------------------------------- round loop
def _stub(threshold_of):
    """decode_round / accept stand-ins: a row's result is its (item, try); a cell accepts from its threshold on, and
    additionally skips odd tries -- the lowest accepted try is the first even one >= the threshold."""
    seen = []

    def decode_round(rnd):
        assert np.all(np.diff(rnd.pair * 1000 + rnd.alpha) >= 0)               # cells in (pair, alpha) order
        seen.append(rnd)
        return list(zip(rnd.item.tolist(), rnd.pair.tolist(), rnd.alpha.tolist(), rnd.tries.tolist()))

    def accept(o):
        _, p, i, k = o
        return k >= threshold_of(p, i) and k % 2 == 0
    return decode_round, accept, seen


def test_chunking_resolves_every_cell_to_the_same_try():
    P, A, K = 3, 4, 40
    thr = lambda p, i: (7 * p + 5 * i) % 23                                     # noqa: E731
    outs = {}
    for chunk in (4, 16, 1, 40):
        dr, acc, seen = _stub(thr)
        tries, results, n = MI.run_ladder(P, A, K, chunk, None, dr, acc)
        outs[chunk] = tries
        assert n == sum(len(r.pair) for r in seen)
        for p in range(P):
            for i in range(A):
                t = thr(p, i) + thr(p, i) % 2
                assert tries[p, i] == t and results[p][i] == ((p * A + i) * K + t, p, i, t)
    assert all(np.array_equal(outs[4], o) for o in outs.values())
    # a resolved cell sends no more rows: with chunk 4 the cell (0, 0) (threshold 0) appears in the first round only
    dr, acc, seen = _stub(thr)
    MI.run_ladder(P, A, K, 4, None, dr, acc)
    assert all(not np.any((r.pair == 0) & (r.alpha == 0)) for r in seen[1:])
    assert all(np.array_equal(r.tries.reshape(-1, 4), np.tile(np.arange(4 * j, 4 * j + 4), (len(r.pair) // 4, 1)))
               for j, r in enumerate(seen))


def test_exhausted_ladder_and_pair_ids():
    dr, acc, seen = _stub(lambda p, i: 99)
    tries, results, n = MI.run_ladder(2, 3, 10, 4, None, dr, acc)              # rounds of 4, 4, 2 rungs
    assert np.all(tries == -1) and all(o is None for row in results for o in row) and n == 2 * 3 * 10
    assert [len(r.pair) for r in seen] == [24, 24, 12]
    dr, acc, seen = _stub(lambda p, i: 0)
    MI.run_ladder(1, 3, 10, 4, [5], dr, acc)                                    # the pair id keys the items, not the index
    assert seen[0].item.reshape(3, 4).tolist() == [[(5 * 3 + i) * 10 + k for k in range(4)] for i in range(3)]
    assert seen[0].pair.tolist() == [0] * 12
    with pytest.raises(ValueError):
        MI.run_ladder(2, 3, 10, 4, [5], dr, acc)
    with pytest.raises(ValueError):
        MI.run_ladder(2, 3, 10, 0, None, dr, acc)


def test_item_key_overflow():
    A, K = 8, 400
    last = (2 ** 31) // (A * K) - 1                                             # the largest pair id whose keys fit
    keys = MI.item_keys([0, last], A, K)
    assert keys.shape == (2, A, K) and keys[1, -1, -1] == (last * A + A - 1) * K + K - 1 < 2 ** 31
    assert keys[0, 2, 3] == 2 * K + 3
    with pytest.raises(ValueError, match="int32"):
        MI.item_keys([last + 1], A, K)
    with pytest.raises(ValueError, match="int32"):
        MI.run_ladder(1, A, K, 16, [2 ** 40], lambda r: [], lambda o: True)
    with pytest.raises(ValueError):
        MI.item_keys([-1], A, K)


# -------------------------------------------------------------------------------------- the reference's normals
def test_interp_normals_moments_and_layout():
    D, tokens = 128, 400
    e = LR.token_normals(42, 7, tokens, D)                                      # [tokens, 5, D]: 256 000 values
    n = e.size
    assert abs(e.mean()) < 5 / math.sqrt(n) and abs(e.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs((e ** 4).mean() - 3) < 5 * math.sqrt(96 / n)
    for s in range(5):                                                          # and each of the five vectors on its own
        x = e[:, s].reshape(-1)
        assert abs(x.mean()) < 5 / math.sqrt(x.size) and abs(x.var() - 1) < 5 * math.sqrt(2 / x.size)
    # the five vectors, neighbouring tokens and two items are uncorrelated
    flat = e.transpose(1, 0, 2).reshape(5, -1)
    cc = np.corrcoef(flat)
    assert np.all(np.abs(cc[~np.eye(5, dtype=bool)]) < 5 / math.sqrt(flat.shape[1]))
    other = LR.token_normals(42, 8, tokens, D)
    assert abs(np.corrcoef(e.reshape(-1), other.reshape(-1))[0, 1]) < 5 / math.sqrt(n)
    # layout: nothing but (item, t, s, d) enters -- a shorter call and a narrower D are prefixes
    assert np.array_equal(LR.token_normals(42, 7, 3, D), e[:3])
    assert np.array_equal(LR.token_normals(42, 7, 3, 6), e[:3, :, :6])
    assert np.array_equal(LR.interp_normals(42, 7, 2, 4, 6), e[2, 4, :6])
    from tests import rng_ref as R
    x, y, _, _ = (int(w) for w in R.philox4x32_10((7, 8 * 2 + 4, 1, LR.LATENT_C3), R.rng_key(42, LR.LATENT_SITE)))
    rad = math.sqrt(-2 * math.log(((x >> 8) + 1) / 2 ** 24))
    ang = float(np.float32(6.283185307179586)) * ((y >> 8) + 1) / 2 ** 24
    assert e[2, 4, 4] == pytest.approx(rad * math.cos(ang), abs=1e-14)
    assert e[2, 4, 5] == pytest.approx(rad * math.sin(ang), abs=1e-14)


def test_reference_float32_evaluation_stays_near_the_float64_one():
    """The tolerance of the device test is built from this difference; it must be a rounding-sized number on
    well-conditioned inputs, and the guard must be reported."""
    g = np.random.default_rng(1)
    D, n = 16, 3
    stats = np.stack([g.normal(size=(n, D)) * 0.5, g.uniform(0.5, 1.5, (n, D)), g.normal(size=(n, D)) * 0.5,
                      g.uniform(0.5, 1.5, (n, D))], axis=1).astype(np.float32)
    stats[2, 1] = stats[2, 3] = 0                                               # molecule 2: one row, std 0
    a, b, lens = [0, 1, 2], [1, 0, 2], [5, 0, 4]
    z, tol, c, sl = LR.interp_tolerance(stats, a, b, [0.3] * 3, [0.2, 0.2, 0.0], lens, [1, 2, 3], 6, 9)
    assert z.shape == (3, 6, D) and np.all(z[0, 5:] == 0) and np.all(z[1] == 0) and np.all(z[2, 4:] == 0)
    assert not sl[2].any() and np.array_equal(z[2, :4], np.broadcast_to(stats[2, 0].astype(np.float64), (4, D)))
    assert sl[0, :5].all() and not sl[0, 5:].any() and np.isnan(c[2, :, 1]).all()
    assert tol.min() >= 1e-5 and tol.max() < 1e-3
