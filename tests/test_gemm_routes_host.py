"""gct_linear_fwd_route / gct_linear_dgrad_route tabulated over the case table of tests/test_gemm_routes_gpu.py in all
three GEMM modes (every GCT_GEMM_ROUTE_* kind is named by a row), a property sweep of the two queries against the
workspace queries over a few thousand shapes, their argument errors, tests/gemm_ref.py held to an explicit-loop
restatement, and the cases shown to discriminate: a tail that draws its dropout mask at row 0, a missing last K-split,
the bias once per slab, a fix-up that skips the last ragged patch, a weight-segment boundary one tile off, the output's
leading dimension taken for N and pre read in compact row space each leave the bound the GPU test applies by >= 100 x.
No GPU: the queries launch nothing.

gemm_f32_panel_kernel<64> is gone: its route asked for N % 64 == 0 and at most 768 tiles of 32 x 64 after the 32 x 32
panel route, whose conditions N % 64 == 0 implies, had been refused for more than 4096 tiles of 32 x 32, i.e. more than
2048 of 32 x 64 -- no shape reached it."""
import ctypes
import math

import pytest

from tests import gemm_ref as G

@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_every_case_reports_the_route_it_names(lib, c):
    for mode in (G.BF16X6, G.BF16X3):
        r = G.query(lib, c, mode)
        assert r[:5] == (c.route, c.splits, c.tail, c.m1, c.tsplits), (G.KIND_NAMES[r[0]], r)
        assert r[5] == G.launches_of(r) and r[7] == 0
        assert r[6] <= (G.ws_bytes_of(lib, c) if c.ws == "full" else 0)
        assert (r[6] > 0) == (r[1] > 1 or r[2] == G.TAIL_SLABS)
    r = G.query(lib, c, G.F32)
    assert r[0] == c.f32_route, (G.KIND_NAMES[r[0]], r)
    assert r[0] not in G.BF16_KINDS and r[2] == 0


def test_every_route_kind_is_named_by_a_case():
    for side_kinds, side in (((G.X6S, G.X6_SPLITK_ALL, G.X6, G.F32_FAST, G.F32_VEC, G.F32_SCALAR), "dgrad"), (G.KINDS, "fwd")):
        have = {c.route for c in G.CASES if c.side == side}
        assert have == set(side_kinds), (side, sorted(have))
    tails = {(c.side, c.tail) for c in G.CASES}
    assert tails == {(s, t) for s in ("fwd", "dgrad") for t in (0, 1, 2)}
    # the tail rows have their own rows with dropout epilogues: row_base carries the head's coordinates on
    for t in (1, 2):
        for s in ("fwd", "dgrad"):
            assert any(c.tail == t and c.p > 0 and c.side == s for c in G.CASES), (t, s)
    assert any(c.route == G.F32_SMALL and c.splits > 1 and (c.K // 32) % c.splits for c in G.CASES)   # ragged last K range


def test_k1024_takes_the_split_only_from_2048_rows():
    assert G.case("fwd", "splitk-all-not-at-K1024").route == G.PANEL32
    assert G.case("fwd", "splitk-all-4").route == G.X6_SPLITK_ALL


# ------------------------------------------------------------------------------------------------ property sweep
SWEEP_M = sorted({m + d for m in (4, 32, 64, 128, 256, 1024, 2048, 4096, 16384, 32768) for d in (-1, 0, 1)} |
                 {1, 77, 300, 5184, 33000, 40960, 41472, 45000})
SWEEP_N = (1, 28, 31, 32, 64, 96, 128, 256, 260, 512, 516, 1024, 1536, 2048)     # the model's widths and their neighbours
SWEEP_K = (30, 36, 64, 256, 260, 384, 416, 512, 1024, 1280, 2048)


def _sweep_cases():
    for side in ("fwd", "dgrad"):
        for M in SWEEP_M:
            for N in SWEEP_N:
                for K in SWEEP_K:
                    i = (M * 31 + N * 7 + K) % 8                 # planes and epilogue vary with the shape: every
                    for planes, epi in ((True, i % 4), (i >= 4, (i + 1) % 4)):   # combination occurs, two per shape
                        if side == "fwd":
                            yield G._case(side, "sweep", 0, 0, M, K, 1, N, epi=epi, planes=planes)
                        else:
                            yield G._case(side, "sweep", 0, 0, M, N, 1, K, epi=epi, planes=planes)


def test_route_properties_over_a_sweep_of_shapes(lib):
    n, seen, combos = 0, set(), set()
    for c in _sweep_cases():
        full = G.ws_bytes_of(lib, c)
        for mode in (G.BF16X6, G.F32):
            r = G.query(lib, c, mode, full)
            what = (G.case_id(c), c.M, c.K, c.nper, c.epi, c.planes, mode, r)
            seen.add((c.side, r[0], r[2]))
            combos.add((c.side, c.planes, c.epi))
            assert r[0] in G.KINDS and r[7] == 0, what
            assert r[6] <= full, what                            # the workspace query is an upper bound over every route
            assert r[5] == G.launches_of(r), what
            assert (r[6] > 0) == (r[1] > 1 or r[2] == G.TAIL_SLABS), what
            assert r[1] == 1 or r[0] in (G.X6_SPLITK_ALL, G.F32_SMALL), what
            if r[2]:
                assert r[0] == G.X6 and 0 < r[3] < c.M and r[3] % 128 == 0, what     # head rows + tail rows = M
                assert (r[4] > 1) == (r[2] == G.TAIL_SLABS), what
            else:
                assert r[3] == 0 and r[4] == 1, what
            r0 = G.query(lib, c, mode, 0)                        # no workspace: no slab route, one launch
            assert r0[0] != G.X6_SPLITK_ALL and r0[1:7] == (1, 0, 0, 1, 1, 0), (what, r0)
            if r[6] > 0:                                         # one byte short of the route's need: fewer splits or none
                r1 = G.query(lib, c, mode, r[6] - 1)
                assert r1[6] < r[6] and (r1[1], r1[4]) < (r[1], r[4]) or r1[0] != r[0], (what, r1)
                assert r1[5] == G.launches_of(r1), (what, r1)
            n += 1
    assert n > 4000
    assert combos == {(s, pl, e) for s in ("fwd", "dgrad") for pl in (True, False) for e in range(4)}
    for side in ("fwd", "dgrad"):                               # the sweep met every slab route and both tails
        assert {(side, G.X6_SPLITK_ALL, 0), (side, G.X6, 1), (side, G.X6, 2), (side, G.X6S, 0)} <= seen, seen
    assert ("fwd", G.F32_SMALL, 0) in seen and ("fwd", G.PANEL32, 0) in seen and ("fwd", G.PANEL_THIN, 0) in seen


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_leave_out8_alone(lib):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    a = ctypes.addressof(out)
    fwd_ok = [300, 64, 1, 128, 64, 64, 128, 0, 1, 1, 1, G.BF16X6, 0]
    dg_ok = [300, 1, 128, 64, 128, 64, 64, 0, 1, 1, G.BF16X6, 0]
    assert lib.gct_linear_fwd_route(*fwd_ok, a) == 0 and out[0] in G.KINDS
    assert lib.gct_linear_dgrad_route(*dg_ok, a) == 0 and out[0] in G.KINDS
    assert lib.gct_linear_fwd_route(0, *fwd_ok[1:], a) == 0 and tuple(out)[:6] == (G.NONE, 1, 0, 0, 1, 0)    # M = 0: no launch
    bad_fwd = {0: -1, 1: 0, 2: 0, 3: 0, 4: -1, 5: -1, 6: -1, 7: 4, 11: 3, 12: -1}
    bad_dg = {0: -1, 1: 4, 2: 0, 3: 0, 4: -1, 5: -1, 6: -1, 7: -1, 10: 7, 11: -1}
    for fn, ok, bad in ((lib.gct_linear_fwd_route, fwd_ok, bad_fwd), (lib.gct_linear_dgrad_route, dg_ok, bad_dg)):
        for i, v in bad.items():
            for k in range(8):
                out[k] = -7
            args = list(ok)
            args[i] = v
            assert fn(*args, a) != 0, (fn.__name__, i, v)
            assert list(out) == [-7] * 8, (fn.__name__, i, v, list(out))
        assert fn(*ok, None) != 0
    args = list(fwd_ok)
    args[2], args[7] = 2, G.EPI_DROP_RESID                       # fused epilogues take one segment
    assert lib.gct_linear_fwd_route(*args, a) != 0
    assert lib.gct_gemm_last_route(None) != 0
    assert lib.gct_gemm_last_route(a) == 0


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("side", ["fwd", "dgrad"])
def test_reference_against_explicit_loops(side):
    c = G._case(side, "tiny", 0, 0, 6, 5, 2, 3, lda=8, ldw=7, ldc=9)
    inp = G.Inputs(c)
    ref = G.reference(inp)
    n = 6
    for m in range(c.M):
        for j in range(G.widths(c)[1]):
            if side == "fwd":
                terms = [float(inp.a[m, k]) * float(inp.w[j, k]) for k in range(c.K)] + [float(inp.bias[j])]
            else:
                terms = [float(inp.a[m, i]) * float(inp.w[i, j]) for i in range(n)]
            assert math.isclose(float(ref.acc[m, j]), math.fsum(terms), rel_tol=1e-13, abs_tol=1e-15)
            assert math.isclose(float(ref.S[m, j]), math.fsum(abs(t) for t in terms), rel_tol=1e-13)
    assert ref.terms == (c.K + 1 if side == "fwd" else n)


def test_bound_counts_the_slabs_of_the_rows_that_have_them():
    assert G.slabs_of_rows(5, (G.X6, 1, G.TAIL_SLABS, 3, 8, 3, 0, 0)).tolist() == [0, 0, 0, 8, 8]
    assert G.slabs_of_rows(3, (G.F32_SMALL, 3, 0, 0, 1, 2, 0, 0)).tolist() == [3, 3, 3]
    assert G.slabs_of_rows(3, (G.X6, 1, G.TAIL_SMALL, 128, 1, 2, 0, 0)).tolist() == [0, 0, 0]
    assert G.DROP is __import__("tests.wgrad_ref", fromlist=["DROP"]).DROP      # imported, not copied


# ------------------------------------------------------------------------------------------------ mistake simulators
def _setup(lib, side, name, mode=G.BF16X6):
    c = G.case(side, name)
    inp = G.Inputs(c)
    ref = G.reference(inp)
    out8 = G.query(lib, c, mode)
    return c, inp, ref, out8, G.bound(ref, mode, out8)


def _caught(inp, ref, B, outs, what):
    assert G.judge(inp, ref, B, G.expected(inp, ref)) == 0.0     # the reference itself passes
    r = G.judge(inp, ref, B, outs)
    assert r >= 100, f"{what}: only {r:.1f} x the bound"


def test_a_tail_mask_drawn_at_row_0_is_caught(lib):
    for side, name in (("fwd", "x6-small-tail-gelu-drop"), ("dgrad", "x6-small-tail-quad-gelubwd")):
        c, inp, ref, out8, B = _setup(lib, side, name)
        assert out8[2] and c.p > 0
        _caught(inp, ref, B, G.mistake_tail_mask_at_row_0(inp, ref, out8), name)


def test_a_missing_last_k_split_is_caught(lib):
    for side, name in (("fwd", "splitk-all-8"), ("fwd", "f32-small-split-ragged-K-range-resid"), ("dgrad", "splitk-all-accum")):
        c, inp, ref, out8, B = _setup(lib, side, name)
        _caught(inp, ref, B, G.mistake_last_split_missing(inp, ref, out8), name)


def test_the_bias_once_per_slab_is_caught(lib):
    for name in ("splitk-all-8", "f32-small-split"):
        c, inp, ref, out8, B = _setup(lib, "fwd", name)
        _caught(inp, ref, B, G.mistake_bias_per_slab(inp, ref, out8), name)


def test_a_fixup_that_skips_the_ragged_patch_is_caught(lib):
    for name in ("f32-small-split", "splitk-all-3seg-raggedM-ld"):
        c, inp, ref, out8, B = _setup(lib, "fwd", name)
        assert c.M % 4 and out8[1] > 1
        _caught(inp, ref, B, G.mistake_fixup_skips_ragged_patch(inp, ref, out8), name)


def test_a_segment_boundary_one_tile_off_is_caught(lib):
    for name in ("x6s-3seg-raggedM-ld", "splitk-all-3seg-raggedM-ld"):
        c, inp, ref, out8, B = _setup(lib, "fwd", name)
        _caught(inp, ref, B, G.mistake_segment_boundary_one_tile_off(inp, ref, tile=64 if c.nper < 256 else 128), name)


def test_ldc_taken_for_n_is_caught(lib):
    for name in ("f32-small-split", "splitk-all-3seg-raggedM-ld"):
        c, inp, ref, out8, B = _setup(lib, "fwd", name)
        assert out8[1] > 1
        _caught(inp, ref, B, G.mistake_ldc_for_n(inp, ref, out8), name)


def test_pre_read_in_compact_row_space_is_caught(lib):
    for name in ("x6s-3seg-raggedN-ld-quad-gelubwd", "x6-slab-tail-3seg-quad-mulsaved"):
        c, inp, ref, out8, B = _setup(lib, "dgrad", name)
        assert G.pre_rows(c) > c.M
        _caught(inp, ref, B, G.mistake_pre_in_compact_space(inp, ref), name)
