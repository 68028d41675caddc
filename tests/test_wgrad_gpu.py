"""gct_linear_wgrad against tests/wgrad_ref.py (fp64 on the CPU, derived bound) on every route gct_wgrad_route reports --
bf16 tiles, fast fp32 with the fused bias slab, vector and scalar fp32 with gct_colsum -- through raw library calls:

  1  shares of a tile list: 0, 1, 2, 3, 4 listed tiles per split (0 .. 32 listed of 32, first / last / scattered), the
     same dY without the list, dY non-zero outside the list
  2  a share of 1056 tiles (longer than the kernel's cached list) and of 1024 (the longest cached one)
  3  split geometry: M = 32, 64, 160, 1056 (a last split of one tile), 9600 (fewer splits than asked), 0
  4  three / two dY segments cut out of one buffer, X a column slice, separate dw allocations, no bias
  5  rows that are no multiple of 32, the vocabulary head, K = 30, a dY pointer 4 bytes off
  6  cases of 1 and 4 in bf16x3 mode
  7  ops.linear_wgrad(kt = ops.nonzero_row_tiles(dy)) = the raw call, bit for bit, with and without the side stream

Every call: dw and db start as NaN; ws is exactly gct_wgrad_ws_bytes long plus a 4 KiB guard that must stay untouched,
once NaN-filled and once zero-filled (bit-equal results); the call repeated (bit-equal: deterministic).  The kernel and
bias path are asserted from gct_wgrad_route and the matching launch counter.  tests/test_wgrad_ref_host.py shows that
these inputs tell a kernel's likely mistakes apart by >= 100 x the bound.

Measured on MI355X, worst error / bound (dw, db) per group, printed at the end of the module with -s:
  1 shares 0.214 (cnt3-sparse, three terms per output), 0.049   2 long share 0.013, 0.0004   3 geometry 0.141, 0.027
  4 segments 0.0009, 0.0003   5 ragged 0.096, 0.013   6 bf16x3 0.160, 0.019.  No case is above 0.5; the 55 tests take 4 s."""
import ctypes

import pytest
import torch

from tests import wgrad_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
WORST = {}                       # worst error / bound per (group, quantity)
ROUTES = {}                      # case -> (kind, nsplit, shares)


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib
    yield _lib.load()
    for key, val in ROUTES.items():
        print(f"[wgrad] {key}: {val}")
    for key in sorted(WORST):
        print(f"[wgrad] worst err / bound  {key}: {WORST[key]:.4f}")


def _check(rc, what):
    from gct_plus_amd import _lib
    _lib.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def nanf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def route(lib, c, mode):
    out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    _check(lib.gct_wgrad_route(c.M, c.nseg, c.nper, c.K, c.lddy, c.ldx, int(c.aligned16), int(c.want_bias), mode,
                               ctypes.addressof(out)), "gct_wgrad_route")
    return tuple(out)


def counters(lib):
    out = (ctypes.c_int64 * 2)()
    _check(lib.gct_gemm_launch_counts(ctypes.addressof(out)), "gct_gemm_launch_counts")
    return {"fp32": int(out[0]), "x6": int(out[1]), "x6k": int(lib.gct_gemm_x6_kernel_launches()),
            "x3": int(lib.gct_gemm_x3_launches())}


class Operands:
    """device copies of a case's buffers and the addresses of the operands inside them"""

    def __init__(self, c, dy_buf, x_buf, tiles):
        self.c, self.dy_buf, self.x_buf = c, dy_buf, x_buf
        base = dy_buf.data_ptr() + (4 if c.how == "misaligned" else 0)
        self.dy = [base + 4 * s * c.nper if s < c.nseg else None for s in range(3)]
        self.x = x_buf.data_ptr() + 4 * (c.ldx - c.K)
        self.tiles = self.count = None
        if tiles is not None:
            self.tiles = torch.tensor(tiles + [0] * 8, dtype=torch.int32, device=DEV)   # never empty; entries past the count are valid tiles
            self.count = torch.tensor([len(tiles)], dtype=torch.int32, device=DEV)

    @classmethod
    def of(cls, inp, with_list=True):
        return cls(inp.c, inp.dy_buf.to(DEV), inp.x_buf.to(DEV), inp.list if with_list else None)


def raw_wgrad(lib, op, fill):
    """one gct_linear_wgrad into NaN-filled dw / db with ws = `fill` over exactly gct_wgrad_ws_bytes + a guard"""
    c = op.c
    need = int(lib.gct_wgrad_ws_bytes(c.M, c.nseg * c.nper, c.K))
    assert need % 4 == 0
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=DEV)
    ws[:need].view(torch.float32).fill_(fill)
    ws[need:] = 0xA5
    dws = [nanf(c.nper, c.K) for _ in range(c.nseg)]
    dbs = [nanf(c.nper) for _ in range(c.nseg)] if c.want_bias else []
    pw = [d.data_ptr() for d in dws] + [None] * (3 - c.nseg)
    pb = [d.data_ptr() for d in dbs] + [None] * (3 - len(dbs))
    _check(lib.gct_linear_wgrad(op.dy[0], op.dy[1], op.dy[2], c.lddy, c.M, c.nseg, c.nper, op.x, c.ldx, c.K,
                                pw[0], pw[1], pw[2], c.K, pb[0], pb[1], pb[2], ws.data_ptr(),
                                None if op.tiles is None else op.tiles.data_ptr(),
                                None if op.count is None else op.count.data_ptr(), _st()), "gct_linear_wgrad")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), f"{W.case_id(c)}: the call wrote past gct_wgrad_ws_bytes = {need}"
    dw = torch.cat(dws).cpu()
    db = torch.cat(dbs).cpu() if dbs else None
    return dw, db


def run_lengths(v):
    """[4, 4, 4, 1] -> '3 x 4, 1 x 1'"""
    out = []
    for x in v:
        if out and out[-1][1] == x:
            out[-1][0] += 1
        else:
            out.append([1, x])
    return ", ".join(f"{n} x {x}" for n, x in out)


def bits_equal(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def hold(key, what, got, want, bound):
    r = W.ratio(got, want, bound)
    print(f"  {key} {what}: err / bound {r:.4f}")
    g = key.split(":")[0] + " " + what
    WORST[g] = max(WORST.get(g, 0.0), r)
    assert r <= 1.0, f"{key} {what}: worst error is {r:.3f} x the bound"


def run(lib, c, mode, op, ref, xs, tag=""):
    """the three calls of a case (ws NaN, ws zero, ws NaN again), the counters, and the comparison with `ref`"""
    from gct_plus_amd import ops
    ops.gemm_set_mode(mode)
    kind, ns, ks, fused = r = route(lib, c, mode)
    listed = op.tiles is not None and kind == W.BF16_TILES
    key = f"{c.group}: {c.name}{tag} mode {mode}"
    ROUTES[key] = (W.KIND_NAMES[kind], f"nsplit {ns}", "bias fused" if fused else "bias colsum" if c.want_bias else "no bias",
                   "tiles per split: " + (run_lengths(W.shares(len(W.tile_list(c)), ns)) if listed else
                                          run_lengths(W.range_tiles(c.M, ks, ns)) if c.M % 32 == 0 else f"{ns} x {ks} rows"))
    c0 = counters(lib)
    dw, db = raw_wgrad(lib, op, float("nan"))
    c1 = counters(lib)
    moved = {k: c1[k] - c0[k] for k in c0}
    if kind != W.BF16_TILES:
        assert moved == {"fp32": 1, "x6": 0, "x6k": 0, "x3": 0}, (key, moved)
    elif mode == W.BF16X3:
        assert moved == {"fp32": 0, "x6": 0, "x6k": 0, "x3": 1}, (key, moved)
    else:
        assert moved == {"fp32": 0, "x6": 1, "x6k": 1, "x3": 0}, (key, moved)
    dw0, db0 = raw_wgrad(lib, op, 0.0)
    assert bits_equal(dw, dw0) and bits_equal(db, db0), f"{key}: the result depends on what ws held"
    dw2, db2 = raw_wgrad(lib, op, float("nan"))
    assert bits_equal(dw, dw2) and bits_equal(db, db2), f"{key}: two identical calls differ"
    hold(key, "dw", dw, ref.dw, W.bound_w(ref, mode, ns, xs))
    if c.want_bias:
        hold(key, "db", db, ref.db, W.bound_b(ref, ns))
    else:
        assert db is None
    return r, dw, db


def run_case(lib, c, mode, with_list=True, tag=""):
    inp = W.Inputs(c)
    tiles = W.reduced_tiles(c) if with_list else None
    ref = inp.reference(tiles)
    xs = W.x_abs_colsum(inp.views()[1], tiles)
    return run(lib, c, mode, Operands.of(inp, with_list), ref, xs, tag)


# ------------------------------------------------------------------------------------------------ 1: shares of a list
@pytest.mark.parametrize("c", W.cases("1 shares"), ids=W.case_id)
def test_shares_of_a_tile_list(lib, c):
    (kind, ns, ks, fused), dw, db = run_case(lib, c, W.BF16X6)
    assert (kind, ns, ks, fused) == (W.BF16_TILES, 8, 128, 1)
    if c.cnt == 0:
        assert not dw.any() and not db.any()                   # every share empty: exact zeros over NaN slabs
    if c.how != "outside":                                     # dY is zero off the list: the same problem without it
        run_case(lib, c, W.BF16X6, with_list=False, tag=" (no list)")


# ------------------------------------------------------------------------------------------------ 2: a long share
def test_a_share_longer_than_the_cached_list(lib):
    """1056 listed tiles in one split (the list is read from memory, not from its LDS copy) and 1024 (the longest share
    that is cached), one non-zero dY row per tile; the reference multiplies the 1056 live rows only"""
    long_, cached = W.cases("2 long share")
    c = long_
    rows, dy_live, x_live = W.long_live_inputs(c)
    g = torch.Generator(device=DEV).manual_seed(5)
    x_buf = torch.randn(c.M, c.K, device=DEV, generator=g)     # rows beside the live ones: dense, they meet zeros only
    dy_buf = torch.zeros(c.M, c.nper, device=DEV)
    ridx = torch.tensor(rows, device=DEV)
    x_buf[ridx] = x_live.to(DEV)
    dy_buf[ridx] = dy_live.to(DEV)
    D, X = dy_live.double(), x_live.double()
    full = W.Ref(D.t() @ X, D.sum(0), D.abs().t() @ X.abs(), D.abs().sum(0), len(rows), c.nper)
    out = sorted(set(range(len(rows))) - set(W.tile_list(cached)))                 # the 32 tiles `cached` leaves out
    Do, Xo = D[out], X[out]
    part = W.Ref(full.dw - Do.t() @ Xo, full.db - Do.sum(0), full.S - Do.abs().t() @ Xo.abs(), full.Sb - Do.abs().sum(0),
                 len(rows) - len(out), c.nper)
    for case, ref, xs in ((long_, full, X.abs().sum(0)), (cached, part, X.abs().sum(0) - Xo.abs().sum(0))):
        op = Operands(case, dy_buf, x_buf, W.tile_list(case))
        (kind, ns, ks, fused), _, _ = run(lib, case, W.BF16X6, op, ref, xs)
        assert (kind, ns, fused) == (W.BF16_TILES, 1, 1)
        assert (W.shares(case.cnt, ns)[0] > W.KLIST_MAX) == (case is long_)


# ------------------------------------------------------------------------------------------------ 3: split geometry
@pytest.mark.parametrize("mode", [W.BF16X6, W.F32], ids=["bf16x6", "f32"])
@pytest.mark.parametrize("M", W.GEOM_M)
def test_split_geometry(lib, M, mode):
    want = {32: (1, 32), 64: (1, 64), 160: (2, 96), 1056: (9, 128), 0: (1, 32), 9600: (60, 160)}[M]
    for c in W.cases("3 geometry"):
        if c.M != M:
            continue
        (kind, ns, ks, fused), dw, db = run_case(lib, c, mode)
        assert (ns, ks, fused) == want + (1,)
        assert kind == (W.BF16_TILES if mode == W.BF16X6 and M else W.FAST)
        if M == 0:
            assert not dw.any() and not db.any()               # exact zeros, not NaN and not what ws held


# ------------------------------------------------------------------------------------------------ 4: segments, strides
@pytest.mark.parametrize("mode", [W.BF16X6, W.F32], ids=["bf16x6", "f32"])
@pytest.mark.parametrize("c", W.cases("4 segments"), ids=W.case_id)
def test_segments_and_strides(lib, c, mode):
    (kind, ns, ks, fused), dw, db = run_case(lib, c, mode)
    if c.nper == 96:
        assert (kind, fused) == (W.VEC, 0)                     # segments are not whole tiles: colsum bias
    else:
        assert (kind, fused) == (W.BF16_TILES if mode == W.BF16X6 else W.FAST, int(c.want_bias))


# ------------------------------------------------------------------------------------------------ 5: ragged and scalar
@pytest.mark.parametrize("c", W.cases("5 ragged"), ids=W.case_id)
def test_ragged_and_scalar_routes(lib, c):
    want = {"M37": W.VEC, "M1000": W.VEC, "vocab-head": W.SCALAR, "K30": W.SCALAR, "dy-plus-4-bytes": W.SCALAR}[c.name]
    for mode in (W.BF16X6, W.F32):
        (kind, ns, ks, fused), dw, db = run_case(lib, c, mode)
        assert (kind, fused) == (want, 0)                      # fp32 kernels in either mode, bias through gct_colsum


# ------------------------------------------------------------------------------------------------ 6: bf16x3
@pytest.mark.parametrize("c", W.cases("6 bf16x3"), ids=W.case_id)
def test_bf16x3_mode(lib, c):
    (kind, ns, ks, fused), dw, db = run_case(lib, c, W.BF16X3)
    if c.nper == 96:
        assert (kind, fused) == (W.VEC, 0)
    else:
        assert (kind, fused) == (W.BF16_TILES, int(c.want_bias))
    if c.cnt == 0:
        assert not dw.any() and not db.any()


# ------------------------------------------------------------------------------------------------ 7: the wrapper
@pytest.mark.parametrize("side", [False, True], ids=["main-stream", "side-stream"])
def test_wrapper_equals_the_raw_call(lib, side, monkeypatch):
    from gct_plus_amd import ops
    c = next(k for k in W.cases("1 shares") if k.name == "cnt17-scattered")
    inp = W.Inputs(c)
    ops.gemm_set_mode(W.BF16X6)
    op = Operands.of(inp)
    dw_raw, db_raw = raw_wgrad(lib, op, float("nan"))
    dys, x = inp.views(op.dy_buf, op.x_buf)
    lst, cnt = ops.nonzero_row_tiles(dys[0])
    assert int(cnt.item()) == c.cnt and lst[:c.cnt].tolist() == inp.list
    monkeypatch.setattr(ops, "SIDE_ENABLED", side)
    dw, db = nanf(c.nper, c.K), nanf(c.nper)
    ops.linear_wgrad(dys, c.lddy, x, [dw], [db], kt=(lst, cnt))
    ops.join_side()
    torch.cuda.synchronize()
    assert bits_equal(dw.cpu(), dw_raw) and bits_equal(db.cpu(), db_raw)
