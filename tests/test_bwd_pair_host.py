"""The planner of gct_linear_bwd through its reporter, gct_linear_bwd_route (no launch, no device access: runs on the CPU).

A call is paired -- weight gradient and dgrad of one dY as one bf16 tile launch -- only when both problems take the 128 x
256 bf16 tile kernel on their own and the list-scheduling model of the shared grid (csrc/gemm.hip) beats the model of the
two separate calls by at least two dgrad K-tile times, i.e. fills a partial round instead of merely dropping a launch."""
import ctypes
import itertools

import pytest

F32, BF16X6, BF16X3 = 0, 1, 2
STORE, ACCUM, GELU_BWD, MUL_SAVED = 0, 1, 2, 3
MIN_GAIN = 2.0                                                  # PAIR_MIN_GAIN of csrc/gemm.hip


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib
    return _lib.load()


def route(lib, M, nseg, nper, K, depi=STORE, *, lddy=None, ldx=None, ldw=None, lddx=None, aligned16=1, planes=1, bias=1,
          mode=BF16X6, ws_bytes=None):
    from gct_plus_amd import _lib
    out = (ctypes.c_int64 * 8)(*([-1] * 8))
    if ws_bytes is None:
        ws_bytes = int(lib.gct_linear_bwd_ws_bytes(M, nseg * nper, K))
    _lib.check(lib.gct_linear_bwd_route(M, nseg, nper, K, lddy or nseg * nper, ldx or K, ldw or K, lddx or K, depi,
                                        aligned16, planes, bias, mode, ws_bytes, ctypes.addressof(out)),
               "gct_linear_bwd_route")
    return tuple(out)


# the Linear shapes of a layer (d = 512, dff = 2048): name -> (nseg, nper, K, dgrad epilogue of the training step)
LAYER = {"out": (1, 512, 512, STORE), "qkv": (3, 512, 512, ACCUM), "q": (1, 512, 512, ACCUM), "kv": (2, 512, 512, STORE),
         "ffn2": (1, 512, 2048, MUL_SAVED), "ffn1": (1, 2048, 512, ACCUM)}
ROWS = [32 * n for n in (1, 5, 100, 163, 326, 417, 526, 563, 700, 1000, 1280, 2000)] + [10420, 40962]
GRID = [(M, *LAYER[n]) for M in ROWS for n in LAYER] + [(13344, 1, 256, 512, MUL_SAVED), (8224, 1, 128, 512, STORE),
                                                       (10464, 3, 128, 512, ACCUM), (16832, 2, 256, 512, STORE)]


def test_planner_is_pure(lib):
    """the same answer whatever was asked before, in any order"""
    first = [route(lib, *g) for g in GRID]
    again = [route(lib, *g) for g in reversed(GRID)]
    assert first == list(reversed(again))
    assert any(r[0] for r in first) and not all(r[0] for r in first)


@pytest.mark.parametrize("bias", [0, 1])
def test_paired_plan_fits_the_workspace_and_covers_the_rows(lib, bias):
    for g in GRID:
        M, nseg, nper, K, depi = g
        have = int(lib.gct_linear_bwd_ws_bytes(M, nseg * nper, K))
        for ws_bytes in (have, have // 2, have // 5):
            paired, ns, ks, fused, wb, db, pair_t, sep_t = route(lib, *g, bias=bias, ws_bytes=ws_bytes)
            if not paired:
                assert (wb, db) == (0, 0)
                continue
            Ntot = nseg * nper
            need = 4 * ((ns * Ntot * K + 3) // 4 * 4 + (ns * Ntot if bias else 0))   # slabs, then the bias slabs
            assert need <= ws_bytes <= have, (g, ns, need, ws_bytes)
            assert fused == bias
            assert ks % 32 == 0 and M % 32 == 0 and ks // 32 >= 4          # whole tiles, at least four per split
            assert (ns - 1) * ks < M <= ns * ks                             # the splits cover M exactly, none is empty
            assert wb == -(-Ntot // 128) * -(-K // 256) * ns and db == -(-M // 128) * -(-K // 256)
            assert sep_t - pair_t >= MIN_GAIN * 1000 - 1


def test_nothing_is_paired_off_the_bf16_tile_route(lib):
    M, nseg, nper, K = 18016, 1, 512, 512
    assert route(lib, M, nseg, nper, K)[0] == 1
    refused = {
        "fp32 mode": dict(mode=F32),
        "no weight planes: the dgrad runs on the fp32 kernels": dict(planes=0),
        "a buffer off 16 bytes": dict(aligned16=0),
        "dY rows not whole float4s": dict(lddy=nper + 2),
        "X rows not whole float4s: the weight gradient loads scalars": dict(ldx=K + 1),
    }
    for why, kw in refused.items():
        r = route(lib, M, nseg, nper, K, **kw)
        assert r[0] == 0 and r[4:] == (0, 0, 0, 0), (why, r)
    # rows that are no whole 32-row tiles: the weight gradient is on the fp32 kernels
    assert route(lib, M + 4, nseg, nper, K)[0] == 0
    # few rows: the dgrad is on the small-tile kernel (<= 160 large tiles) or on the K-split-everything route (K' = 2048)
    assert route(lib, 4096, nseg, nper, K)[0] == 0
    assert route(lib, 4096, 1, 2048, 512)[0] == 0
    # not a multiple of 8 columns: no transposed bf16 reads of W for the dgrad
    assert route(lib, M, 1, 512, 516, ldw=516, lddx=516, ldx=516)[0] == 0


# The headline's shapes (B = 512: 40 960 dense rows, about 18 000 compact decoder rows).  Not paired, with the lab's reason
# (profiles/r08_bwd_pair_lab.log): the model finds no partial round to fill --
NOT_PAIRED = {
    ("qkv", 40960): "the 2.5 rounds of the dgrad are already balanced by its own K-split tail (K' = 1 536: 48 K-tiles per "
                    "tile), and ten weight-gradient splits of 128 K-tiles leave nothing shorter to fill the rest with",
    ("ffn2", 40960): "2 560 dgrad tiles are exactly ten rounds and the weight gradient exactly one",
}


@pytest.mark.parametrize("M", [40960, 18016])
@pytest.mark.parametrize("name", sorted(LAYER))
def test_headline_shapes(lib, name, M):
    r = route(lib, M, *LAYER[name])
    gain = (r[7] - r[6]) / 1000.0
    if (name, M) in NOT_PAIRED:
        assert r[0] == 0 and 0 < r[6] and gain < MIN_GAIN, (name, M, r)
    else:
        assert r[0] == 1 and gain >= MIN_GAIN, (name, M, r)


def test_same_plan_in_bf16x6_and_bf16x3(lib):
    for g, bias in itertools.product(GRID, (0, 1)):
        assert route(lib, *g, bias=bias, mode=BF16X6) == route(lib, *g, bias=bias, mode=BF16X3)
