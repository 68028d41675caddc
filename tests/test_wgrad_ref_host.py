"""tests/wgrad_ref.py held to an independent restatement (explicit loops over 32-row tiles), gct_wgrad_route tabulated
over the case table of tests/test_wgrad_gpu.py in all three GEMM modes -- every kernel kind, both bias paths, list shares
of 0, 1, 2, 3, more than 3 and more than 1024 tiles, a last split of one tile, fewer splits than asked for, the workspace
query against what each route touches -- and the cases shown to discriminate: a kernel that skips a listed tile, counts
a share's last tile twice in the bias, loses the tile at a split boundary, leaves an empty share's slab at a stale 1.0 or
reads segment 1's dY for segment 2 moves the result by >= 100 x the bound the GPU test applies; bf16x3 arithmetic in
place of bf16x6 by >= 3 x (the most the two bounds allow).  No GPU: gct_wgrad_route launches nothing."""
import ctypes
import math

import pytest
import torch

from tests import wgrad_ref as W

MODES = (W.F32, W.BF16X6, W.BF16X3)


@pytest.fixture(scope="module")
def route():
    from gct_plus_amd import _lib
    lib = _lib.load()

    def call(c, mode, want_bias=None, aligned16=None):
        out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
        wb = c.want_bias if want_bias is None else want_bias
        al = c.aligned16 if aligned16 is None else aligned16
        _lib.check(lib.gct_wgrad_route(c.M, c.nseg, c.nper, c.K, c.lddy, c.ldx, int(al), int(wb), mode,
                                       ctypes.addressof(out)), "gct_wgrad_route")
        return tuple(out)
    return call


# ------------------------------------------------------------------------------------------------ the reference
def _slow(dys, x, tiles):
    """dW, db, S, Sb, t with explicit loops: tile by tile, row by row, element by element"""
    M, K = x.shape
    nper = dys[0].shape[1]
    N = nper * len(dys)
    dw = [[0.0] * K for _ in range(N)]
    S = [[0.0] * K for _ in range(N)]
    db, Sb, t = [0.0] * N, [0.0] * N, 0
    for tile in (range((M + 31) // 32) if tiles is None else tiles):
        for m in range(32 * tile, min(M, 32 * tile + 32)):
            row = [float(dys[n // nper][m, n % nper]) for n in range(N)]
            t += any(v != 0 for v in row)
            for n in range(N):
                db[n] += row[n]
                Sb[n] += abs(row[n])
                for k in range(K):
                    dw[n][k] += row[n] * float(x[m, k])
                    S[n][k] += abs(row[n]) * abs(float(x[m, k]))
    return torch.tensor(dw, dtype=torch.float64), torch.tensor(db, dtype=torch.float64), \
        torch.tensor(S, dtype=torch.float64), torch.tensor(Sb, dtype=torch.float64), t


@pytest.mark.parametrize("M,nseg,nper,K,tiles", [(70, 2, 3, 5, None), (96, 1, 4, 6, [0, 2]), (100, 3, 2, 3, [1, 3])])
def test_reference_against_explicit_tile_loops(M, nseg, nper, K, tiles):
    buf = W.rnd(M, nseg * nper + 1, seed=M)
    buf[5:9] = 0                                               # zero rows do not count in t
    buf[40] = 0
    x = W.rnd(M, K + 2, seed=M + 1)[:, 2:]
    dys = [buf[:, s * nper:(s + 1) * nper] for s in range(nseg)]
    r = W.reference(dys, x, tiles)
    dw, db, S, Sb, t = _slow(dys, x, tiles)
    assert r.t == t and r.nper == nper
    for got, want in ((r.dw, dw), (r.db, db), (r.S, S), (r.Sb, Sb)):
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert (got - want).abs().max() <= 1e-13 * want.abs().max()
    # the bound formulas, spelled out once
    ns, u = 3, 2.0 ** -24
    xs = W.x_abs_colsum(x, tiles)
    for mode, drop in ((W.F32, 0.0), (W.BF16X6, 2.0 ** -23), (W.BF16X3, 3.02 * 2.0 ** -16)):
        want_b = (drop + (t + ns) * u * 1.01) * S + 3 * 2.0 ** -126 * (Sb[:, None] + xs[None, :])
        assert torch.equal(W.bound_w(r, mode, ns, xs), want_b)
    assert torch.equal(W.bound_b(r, ns), (t + ns + 16) * u * 1.01 * Sb)


def test_ratio_demands_exact_zeros_where_the_bound_is_zero():
    z = torch.zeros(3, dtype=torch.float64)
    assert W.ratio(torch.zeros(3), z, z) == 0.0
    assert W.ratio(torch.tensor([0.0, 1e-30, 0.0]), z, z) == math.inf
    assert W.ratio(torch.tensor([0.0, float("nan"), 0.0]), z, z + 1) == math.inf
    assert W.ratio(torch.tensor([0.5, 2.0, 0.0]), z, z + 1) == 2.0


def test_case_inputs_are_what_the_table_says():
    for c in W.CASES:
        if c.group.startswith("2"):
            rows, dy, x = W.long_live_inputs(c)
            assert len(rows) == c.M // 32 == 1056 and [r // 32 for r in rows] == list(range(1056))
            assert len({r % 32 for r in rows}) == 32 and dy.shape == (1056, c.nper) and x.shape == (1056, c.K)
            lst = W.tile_list(c)
            assert len(lst) == c.cnt and lst == sorted(set(lst)) and lst[-1] < 1056
            continue
        inp = W.Inputs(c)
        dys, x = inp.views()
        assert len(dys) == c.nseg and all(d.shape == (c.M, c.nper) and d.stride(0) == c.lddy for d in dys)
        assert x.shape == (c.M, c.K) and x.stride(0) == c.ldx
        D = torch.cat(list(dys), 1)
        nz = (D != 0).any(1)
        if inp.list is not None:
            assert len(inp.list) == c.cnt and inp.list == sorted(set(inp.list)) and all(0 <= t < c.M // 32 for t in inp.list)
            listed = torch.zeros(c.M, dtype=torch.bool)
            listed[W.rows_of_tiles(inp.list, c.M)] = True
            if c.how in ("first", "last", "scattered"):
                assert not nz[~listed].any() and (c.rows_per_tile < 32 or torch.equal(nz, listed))   # zero off the list
                assert inp.reference().t == c.rows_per_tile * c.cnt
                assert all(int(nz[32 * t:32 * t + 32].sum()) == c.rows_per_tile for t in inp.list)
            elif c.how == "sparse":
                assert not nz[~listed].any() and inp.reference().t == c.cnt
            else:
                assert c.how == "outside" and nz.all()
        elif c.how == "onerow":
            assert int(nz.sum()) == c.M // 32
        else:
            assert nz.all()
        if c.how == "misaligned":
            assert dys[0].data_ptr() % 16 == 4 and c.lddy % 4 == 0
    names = [(c.group, c.name) for c in W.CASES]
    assert len(names) == len(set(names))


# ------------------------------------------------------------------------------------------------ the route
def _shares(c, r):
    kind, ns, ks, _ = r
    if c.cnt is not None and kind == W.BF16_TILES:
        return W.shares(c.cnt, ns)
    return W.range_tiles(c.M, ks, ns) if c.M % 32 == 0 else None


def test_route_over_the_case_table(route):
    kinds, bias_paths, share_lengths = set(), set(), set()
    last_one_tile = fewer_than_asked = long_share = False
    for c in W.CASES:
        for mode in MODES:
            kind, ns, ks, fused = r = route(c, mode)
            assert ns >= 1 and ks >= 32 and ks % 32 == 0
            assert c.M == 0 or (ns - 1) * ks < c.M <= ns * ks           # every split has rows, together they cover M
            if mode not in c.modes:
                continue
            kinds.add(kind)
            if c.want_bias:
                bias_paths.add(fused)
                assert fused == (kind in (W.FAST, W.BF16_TILES))
            else:
                assert fused == 0
            sh = _shares(c, r)
            if c.cnt is not None:
                assert kind == W.BF16_TILES, "a list is honoured on the bf16 route only"
                share_lengths.update(sh)
                long_share |= max(sh) > W.KLIST_MAX
            elif sh is not None and ns > 1:
                last_one_tile |= sh[-1] == 1
            asked = W.wgrad_splits_asked(c.M, c.nseg * c.nper, c.K, kind == W.BF16_TILES)
            assert ns <= asked
            fewer_than_asked |= ns < asked
    assert kinds == {W.SCALAR, W.VEC, W.FAST, W.BF16_TILES}
    assert bias_paths == {0, 1}
    assert {0, 1, 2, 3} <= share_lengths and any(3 < s <= W.KLIST_MAX for s in share_lengths)
    assert long_share and last_one_tile and fewer_than_asked


def test_route_of_each_group_is_the_one_its_cases_are_written_for(route):
    for c in W.cases("1 shares") + [c for c in W.cases("6 bf16x3") if c.cnt is not None]:
        assert route(c, W.BF16X6) == route(c, W.BF16X3) == (W.BF16_TILES, 8, 128, 1)
        assert route(c, W.F32) == (W.FAST, 8, 128, 1)
    got = {cnt: sorted(W.shares(cnt, 8), reverse=True) for cnt in W.SHARE_COUNTS}
    assert got == {0: [0] * 8, 1: [1] + [0] * 7, 3: [1] * 3 + [0] * 5, 9: [2] * 4 + [1] + [0] * 3,
                   17: [3] * 5 + [2] + [0] * 2, 31: [4] * 7 + [3], 32: [4] * 8}
    for c in W.cases("2 long share"):
        assert route(c, W.BF16X6) == (W.BF16_TILES, 1, 32 * 1056, 1)
    assert W.shares(1056, 1) == [1056] and W.shares(1024, 1) == [1024]      # uncached, and the last cached length
    geom = {c.name: c for c in W.cases("3 geometry")}
    for n in W.GEOM_NPER:
        for K in W.GEOM_K:
            tail = f"-n{n}-K{K}"
            for mode, kind in ((W.BF16X6, W.BF16_TILES), (W.F32, W.FAST)):
                assert route(geom["M32" + tail], mode) == (kind, 1, 32, 1)
                assert route(geom["M64" + tail], mode) == (kind, 1, 64, 1)
                assert route(geom["M160" + tail], mode) == (kind, 2, 96, 1)            # 3 + 2 tiles
                assert route(geom["M1056" + tail], mode) == (kind, 9, 128, 1)          # 8 x 4 tiles + 1
                assert route(geom["M9600" + tail], mode) == (kind, 60, 160, 1)         # 64 asked
                assert route(geom["M0" + tail], mode) == (W.FAST, 1, 32, 1)            # no row: never the bf16 kernel
    seg = {c.name: c for c in W.cases("4 segments")}
    assert route(seg["3seg-slices"], W.BF16X6) == (W.BF16_TILES, 9, 128, 1)
    assert route(seg["3seg-slices"], W.F32) == (W.FAST, 9, 128, 1)
    assert route(seg["3seg-nobias"], W.BF16X6) == (W.BF16_TILES, 9, 128, 0)
    for mode in MODES:
        assert route(seg["2seg-96"], mode) == (W.VEC, 9, 128, 0)               # segments are not whole tiles
    rag = {c.name: c for c in W.cases("5 ragged")}
    for mode in MODES:
        assert route(rag["M37"], mode) == (W.VEC, 1, 64, 0)
        assert route(rag["M1000"], mode) == (W.VEC, 8, 128, 0)
        assert route(rag["vocab-head"], mode) == (W.SCALAR, 8, 128, 0)
        assert route(rag["K30"], mode) == (W.SCALAR, 8, 128, 0)
        assert route(rag["dy-plus-4-bytes"], mode) == (W.SCALAR, 8, 128, 0)
        assert route(rag["dy-plus-4-bytes"], mode, aligned16=True)[0] != W.SCALAR


def test_workspace_query_covers_what_every_route_touches(route):
    from gct_plus_amd import _lib
    lib = _lib.load()
    for c in W.CASES:
        have = lib.gct_wgrad_ws_bytes(c.M, c.nseg * c.nper, c.K)
        for mode in MODES:
            for wb in (0, 1):
                for al in (0, 1):
                    _, ns, _, fused = route(c, mode, want_bias=wb, aligned16=al)
                    need = 4 * W.ws_floats_needed(c.M, c.nseg * c.nper, c.K, ns, fused, wb)
                    assert have >= need, (c, mode, wb, al, have, need)


def test_route_refuses_bad_arguments():
    from gct_plus_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 4)()
    ok = (64, 1, 8, 8, 8, 8, 1, 1, 1)
    assert lib.gct_wgrad_route(*ok, ctypes.addressof(out)) == 0
    for i, bad in ((0, -1), (1, 0), (1, 4), (2, 0), (3, 0), (8, 3), (8, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.gct_wgrad_route(*args, ctypes.addressof(out)) != 0
        assert b"wgrad_route" in lib.gct_last_error()
    assert lib.gct_wgrad_route(*ok, None) != 0


# ------------------------------------------------------------------------------------------------ the cases discriminate
def _small_cases():
    return [c for c in W.CASES if not c.group.startswith("2")]


def _tiles_of_shares(c, r):
    """per split: the tiles it reduces (list entries on the bf16 route with a list, else its rows' tiles)"""
    kind, ns, ks, _ = r
    if c.cnt is not None:
        lst, per = W.tile_list(c), (c.cnt + ns - 1) // ns
        return [lst[z * per:z * per + per] for z in range(ns)]
    nt = (c.M + 31) // 32
    return [list(range(z * ks // 32, min(nt, (z + 1) * ks // 32))) for z in range(ns)]


def test_cases_tell_the_likely_mistakes_apart(route):
    seen = {k: 0 for k in ("skip", "twice", "boundary", "stale", "swap")}
    weakest = {k: math.inf for k in seen}
    for c in _small_cases():
        inp = W.Inputs(c)
        ref = inp.reference()
        xs = W.x_abs_colsum(inp.views()[1], W.reduced_tiles(c))
        for mode in c.modes:
            r = route(c, mode)
            ns = r[1]
            bw, bb = W.bound_w(ref, mode, ns, xs), W.bound_b(ref, ns)
            parts = _tiles_of_shares(c, r)
            wrong = {}
            if parts[0]:
                mid = parts[len(parts) // 2] or parts[0]
                wrong["skip"] = W.mistake_skip_tile(inp, mid[len(mid) // 2])
                if c.want_bias:
                    wrong["twice"] = W.mistake_bias_twice(inp, ref, parts[0][-1])
            if len(parts) > 1 and parts[1]:
                wrong["boundary"] = W.mistake_skip_tile(inp, parts[1][0])
            if any(len(p) == 0 for p in parts):
                wrong["stale"] = W.mistake_stale_slab(ref)
            if c.nseg == 3:
                wrong["swap"] = W.mistake_segment_swap(inp)
            for name, (dw, db) in wrong.items():
                moved = W.ratio(dw, ref.dw, bw) if name != "twice" else 0.0
                if c.want_bias:
                    moved = max(moved, W.ratio(db, ref.db, bb))
                seen[name] += 1
                weakest[name] = min(weakest[name], moved)
                assert moved >= 100, f"{W.case_id(c)} mode {mode}: mistake `{name}` moves the result by only {moved:.1f} x the bound"
    print("weakest separation (x bound):", {k: round(v, 1) for k, v in weakest.items()}, "cases:", seen)
    assert all(n > 0 for n in seen.values())


def test_long_share_cases_tell_a_skipped_tile_apart():
    """Case 2 without its 17 GFLOP reference: S <= |dY col|_2 |X col|_2 (Cauchy-Schwarz) gives an upper bound of the
    bound; a skipped tile removes one rank-1 term dY[r] x X[r], a tile counted twice in the bias adds dY[r]."""
    for c in W.cases("2 long share"):
        rows, dy, x = W.long_live_inputs(c)
        lst = W.tile_list(c)
        D, X = dy.double()[lst], x.double()[lst]
        t, ns = len(lst), 1
        S_ub = D.norm(dim=0)[:, None] * X.norm(dim=0)[None, :]
        floor = 3 * 2.0 ** -126 * (D.abs().sum(0)[:, None] + X.abs().sum(0)[None, :])
        bw_ub = (W.DROP[W.BF16X6] + (t + ns) * W.U * 1.01) * S_ub + floor
        bb = (t + ns + 16) * W.U * 1.01 * D.abs().sum(0)
        for i in (0, t // 2, t - 1):
            moved = float(((D[i].abs()[:, None] * X[i].abs()[None, :]) / bw_ub).max())
            print(f"{W.case_id(c)} tile {lst[i]}: skipped moves dw by >= {moved:.0f} x bound")
            assert moved >= 100
        twice = float((D[-1].abs() / bb).max())                # the share's last tile counted twice
        print(f"{W.case_id(c)} tile {lst[-1]}: counted twice moves db by {twice:.0f} x bound")
        assert lst[-1] == 1055 and twice >= 100


def test_bf16x3_in_place_of_bf16x6_is_told_apart():
    """The two bounds are 2^-23 and 3.02 * 2^-16 apart only where few terms are accumulated: measured factor per case."""
    best = {}
    for c in W.cases("1 shares"):
        if c.cnt == 0:
            continue
        inp = W.Inputs(c)
        ref = inp.reference()
        dw3, _ = W.mistake_bf16x3(inp)
        bw = W.bound_w(ref, W.BF16X6, 8, W.x_abs_colsum(inp.views()[1], W.reduced_tiles(c)))
        best[c.name] = W.ratio(dw3, ref.dw, bw)
        assert W.ratio(dw3, ref.dw, W.bound_w(ref, W.BF16X3, 8, W.x_abs_colsum(inp.views()[1], W.reduced_tiles(c)))) <= 1.0
    print("bf16x3 error / bf16x6 bound:", {k: round(v, 2) for k, v in best.items()})
    assert best["cnt3-sparse"] >= 3.0
