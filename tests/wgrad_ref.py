"""fp64 reference, derived error bound, case table and mistake simulators for gct_linear_wgrad
(tests/test_wgrad_ref_host.py runs them on the CPU, tests/test_wgrad_gpu.py holds the kernels to them).

Reference, per segment s:  dW_s = dY_s^T X,  db_s = sum_m dY_s,  S_s = |dY_s|^T |X|,  Sb_s = sum_m |dY_s|, all in fp64
over the rows reduced (every row, or the rows of the listed 32-row tiles).

Bound (derived, not measured on the kernels).  t = rows among those reduced whose dY row is not all zero (adding an
exact zero rounds nothing), ns = the route's nsplit, u = 2^-24:

    |dW - ref| <= (drop + (t + ns) * u * 1.01) * S + floor        drop = 0 (fp32), 2^-23 (bf16x6), 3.02 * 2^-16 (bf16x3)
    |db - ref| <= (t + ns + 16) * u * 1.01 * Sb

drop: what the bf16 piece products leave out (the head of csrc/gemm_x6.inc); (t + ns) u: one fp32 rounding per non-zero
term of the accumulation chain and one per slab of the deterministic slab sum (1.01 covers the second-order terms);
floor: bf16 pieces below the normal range are flushed (tests/test_gemm_x3_gpu.py); the bias is summed in fp32 in every
mode, 16 = the row groups a workgroup combines before it writes its bias slab row."""
import math
from collections import namedtuple

import torch

F32, BF16X6, BF16X3 = 0, 1, 2                                  # GCT_GEMM_*
SCALAR, VEC, FAST, BF16_TILES = 0, 1, 2, 3                     # GCT_WGRAD_* (gct_wgrad_route out4[0])
KIND_NAMES = {SCALAR: "scalar fp32", VEC: "vector fp32", FAST: "fast fp32", BF16_TILES: "bf16 tiles"}
U = 2.0 ** -24
DROP = {F32: 0.0, BF16X6: 2.0 ** -23, BF16X3: 3.02 * 2.0 ** -16}
T = 32                                                         # rows of one tile
KLIST_MAX = 1024                                               # X_KLIST_MAX of csrc/gemm_x6.inc: list entries cached per workgroup


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ reference and bound
Ref = namedtuple("Ref", "dw db S Sb t nper")                   # dw, S: [nseg * nper][K]; db, Sb: [nseg * nper]; fp64


def rows_of_tiles(tiles, M):
    """row indices of the listed 32-row tiles (clipped to M), in list order"""
    if len(tiles) == 0:
        return torch.zeros(0, dtype=torch.int64)
    r = (torch.as_tensor(tiles, dtype=torch.int64)[:, None] * T + torch.arange(T)[None, :]).reshape(-1)
    return r[r < M]


def reference(dys, x, tiles=None):
    """dys: the segments' dY [M][nper] (any strides), x [M][K]; tiles: reduce over these 32-row tiles only (None: all)"""
    D = torch.cat([d.double() for d in dys], 1)
    X = x.double()
    if tiles is not None:
        r = rows_of_tiles(tiles, D.shape[0])
        D, X = D[r], X[r]
    live = (D != 0).any(1)                                     # zero rows add exact zeros: dropping them changes nothing
    D, X = D[live], X[live]
    return Ref(D.t() @ X, D.sum(0), D.abs().t() @ X.abs(), D.abs().sum(0), int(live.sum()), dys[0].shape[1])


def bound_w(ref, mode, ns, X_abs_colsum):
    floor = 3 * 2.0 ** -126 * (ref.Sb[:, None] + X_abs_colsum[None, :])
    return (DROP[mode] + (ref.t + ns) * U * 1.01) * ref.S + floor


def bound_b(ref, ns):
    return (ref.t + ns + 16) * U * 1.01 * ref.Sb


def x_abs_colsum(x, tiles=None):
    X = x.double().abs()
    return X.sum(0) if tiles is None else X[rows_of_tiles(tiles, X.shape[0])].sum(0)


def ratio(got, want, bound):
    """worst |got - want| / bound; where the bound is 0 the result must be exact (inf otherwise)"""
    err = (got.double() - want).abs()
    if not torch.isfinite(err).all():
        return math.inf
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ shares of a tile list
def shares(cnt, nsplit):
    """listed tiles per split: split z takes entries [z * per, z * per + per), per = ceil(cnt / nsplit)"""
    per = (cnt + nsplit - 1) // nsplit
    return [max(0, min(per, cnt - z * per)) for z in range(nsplit)]


def range_tiles(M, ksplit, nsplit):
    """32-row tiles per split when the rows themselves are split (no list)"""
    return [(min(M, (z + 1) * ksplit) - min(M, z * ksplit)) // T for z in range(nsplit)]


def wgrad_splits_asked(M, Ntot, K, bf16):
    """restatement of the launcher's split wish: one resident round of workgroups, >= 4 tiles of rows per split, <= 64"""
    cdiv = lambda a, b: (a + b - 1) // b                                              # noqa: E731
    tiles = cdiv(Ntot, 128) * cdiv(K, 256) if bf16 else cdiv(Ntot, 128) * cdiv(K, 128)
    return max(1, min((256 if bf16 else 512) // tiles, cdiv(M, 128), 64))


def ws_floats_needed(M, Ntot, K, nsplit, fused, want_bias):
    """floats of ws a call touches: the slabs, the bias slabs behind them (4-float aligned), or gct_colsum's partials"""
    slabs = nsplit * Ntot * K
    if fused:
        return (slabs + 3) // 4 * 4 + nsplit * Ntot
    colsum = min(256, max(1, (M + 127) // 128)) * Ntot if want_bias else 0
    return max(slabs, colsum)


# ------------------------------------------------------------------------------------------------ the case table
# One Case = one gct_linear_wgrad problem.  how: contents of dY and of the tile list (cnt = None: no list)
#   dense     dY dense everywhere                      onerow   one non-zero dY row per 32-row tile, at a varying offset
#   first / last / scattered   the first cnt, last cnt, a scattered ascending draw of cnt tiles; dY dense on them, zero off
#              (rows_per_tile < 32: only that many rows of each listed tile are non-zero -- the bf16x3 cases, whose bound
#              is 2^7 looser per term: with 8 rows per tile a stale 1.0 still stands >= 100 x above it)
#   outside   scattered list, dY dense everywhere: the reference reduces over the listed tiles only
#   sparse    scattered list, one non-zero row per listed tile (t = cnt: the bound is tight enough to tell bf16x3 apart)
#   misaligned   dense, dY's base pointer 4 bytes off a 16-byte boundary
Case = namedtuple("Case", "group name M nseg nper K lddy ldx cnt how modes want_bias aligned16 scales rows_per_tile")


def _case(group, name, M, nseg, nper, K, *, lddy=None, ldx=None, cnt=None, how="dense", modes=(BF16X6,), want_bias=True,
          aligned16=True, scales=(1.0, 1.0, 1.0), rows_per_tile=T):
    return Case(group, name, M, nseg, nper, K, lddy or nseg * nper, ldx or K, cnt, how, modes, want_bias, aligned16, scales,
                rows_per_tile)


SHARE_SHAPE = dict(M=1024, nseg=1, nper=128, K=256)            # the route reports 8 splits of 4 tiles
SHARE_COUNTS = (0, 1, 3, 9, 17, 31, 32)
LONG_SHAPE = dict(M=T * 1056, nseg=1, nper=2048, K=4096)       # one split: a share of 1056 > KLIST_MAX tiles
GEOM_M = (32, 64, 128 + 32, 1056, 0, 9600)                     # 9600: 64 splits asked, 60 made
GEOM_NPER = (8, 128, 132)
GEOM_K = (8, 256, 260)
SEG_SCALES = (1.0, 3.0, 0.25)


def _share_cases(group, counts, modes, rows_per_tile=T):
    out = []
    for cnt in counts:
        for how in ("first", "last", "scattered"):
            if how != "first" and cnt in (0, 32):
                continue                                       # one way to list none or all of the 32 tiles
            out.append(_case(group, f"cnt{cnt}-{how}", cnt=cnt, how=how, modes=modes, rows_per_tile=rows_per_tile,
                             **SHARE_SHAPE))
    return out


def _seg_cases(group, modes):
    return [
        _case(group, "3seg-slices", 1056, 3, 128, 256, lddy=3 * 128 + 8, ldx=256 + 4, modes=modes, scales=SEG_SCALES),
        _case(group, "2seg-96", 1056, 2, 96, 256, lddy=2 * 96 + 8, ldx=256 + 4, modes=modes, scales=SEG_SCALES),
        _case(group, "3seg-nobias", 1056, 3, 128, 256, lddy=3 * 128 + 8, ldx=256 + 4, modes=modes, scales=SEG_SCALES,
              want_bias=False),
    ]


CASES = (
    _share_cases("1 shares", SHARE_COUNTS, (BF16X6,))
    + [_case("1 shares", "cnt9-outside", cnt=9, how="outside", **SHARE_SHAPE),
       _case("1 shares", "cnt3-sparse", cnt=3, how="sparse", **SHARE_SHAPE)]
    + [_case("2 long share", "cnt1056", cnt=1056, how="onerow", **LONG_SHAPE),
       _case("2 long share", "cnt1024", cnt=1024, how="outside-onerow", **LONG_SHAPE)]
    + [_case("3 geometry", f"M{M}-n{n}-K{K}", M, 1, n, K, how="onerow" if M > 2000 else "dense", modes=(BF16X6, F32))
       for M in GEOM_M for n in GEOM_NPER for K in GEOM_K]
    + _seg_cases("4 segments", (BF16X6, F32))
    + [_case("5 ragged", "M37", 37, 1, 128, 256),
       _case("5 ragged", "M1000", 1000, 1, 128, 256),
       _case("5 ragged", "vocab-head", 1000, 1, 30, 512),
       _case("5 ragged", "K30", 1024, 1, 128, 30),
       _case("5 ragged", "dy-plus-4-bytes", 1024, 1, 128, 256, how="misaligned", aligned16=False)]
    + _share_cases("6 bf16x3", (0, 3, 17), (BF16X3,), rows_per_tile=8) + _seg_cases("6 bf16x3", (BF16X3,))
)


def cases(group):
    return [c for c in CASES if c.group == group]


def case_id(c):
    return f"{c.group.split()[0]}-{c.name}"


def tile_list(c):
    """the case's list of 32-row tile indices (ascending), or None"""
    if c.cnt is None:
        return None
    nt = c.M // T
    if c.how == "first" or c.cnt == nt:
        return list(range(c.cnt))
    if c.how == "last":
        return list(range(nt - c.cnt, nt))
    if c.how == "outside-onerow":                              # every 33rd tile left out, the last tile kept
        out = set(range(16, nt, 33))
        assert len(out) == nt - c.cnt
        return [t for t in range(nt) if t not in out]
    g = torch.Generator().manual_seed(1000 + c.cnt)
    return sorted(torch.randperm(nt, generator=g)[:c.cnt].tolist())


def onerow_offsets(ntiles):
    """the offset of the one non-zero row inside each tile: every offset 0..31 occurs, in no regular order"""
    return [(7 * i + 3 * (i // T)) % T for i in range(ntiles)]


def live_rows(c):
    """rows whose dY is non-zero (ascending); None: all"""
    lst = tile_list(c)
    nt = (c.M + T - 1) // T
    if c.how in ("dense", "outside", "misaligned"):
        return None
    if c.how in ("onerow", "outside-onerow"):                  # one row in EVERY tile (outside-onerow: the list leaves some out)
        off = onerow_offsets(nt)
        return [t * T + off[t] for t in range(nt)]
    if c.how == "sparse":
        off = onerow_offsets(nt)
        return [t * T + off[t] for t in lst]
    step = T // c.rows_per_tile                                # first / last / scattered: dense on the listed tiles, or
    return [t * T + (step * j + t) % T for t in lst for j in range(c.rows_per_tile)]     # rows_per_tile rows of each


def reduced_tiles(c):
    """the tiles the reference reduces over: the list on the bf16 route, None (every row) otherwise"""
    return tile_list(c)


class Inputs:
    """CPU inputs of a case.  dy_buf [rows][lddy] (flat with one leading float when misaligned) and x_buf [rows][ldx]
    are the allocations; views() cuts the operands out of them (or out of device copies of them)."""

    def __init__(self, c, seed=0):
        assert c.M * c.nper * c.nseg <= 1 << 24, "large cases build their operands on the device (long_live_inputs)"
        self.c = c
        rows = max(c.M, 1)                                     # M == 0: one row, so that the pointers are not null
        dy = rnd(rows, c.lddy, seed=seed + 1)
        for s in range(c.nseg):
            dy[:, s * c.nper:(s + 1) * c.nper] *= c.scales[s]
        live = live_rows(c)
        if live is not None:
            keep = torch.zeros(rows, dtype=torch.bool)
            keep[torch.as_tensor(live, dtype=torch.int64)] = True
            dy[~keep] = 0
        self.x_buf = rnd(rows, c.ldx, seed=seed + 2)
        if c.how == "misaligned":
            self.dy_buf = torch.cat([torch.full((1,), 7.0), dy.reshape(-1), torch.full((3,), 7.0)])
        else:
            self.dy_buf = dy
        self.list = tile_list(c)

    def views(self, dy_buf=None, x_buf=None):
        c = self.c
        dy_buf = self.dy_buf if dy_buf is None else dy_buf
        x_buf = self.x_buf if x_buf is None else x_buf
        rows = max(c.M, 1)
        dy = dy_buf[1:1 + rows * c.lddy].view(rows, c.lddy) if c.how == "misaligned" else dy_buf
        dys = [dy[:c.M, s * c.nper:(s + 1) * c.nper] for s in range(c.nseg)]
        x = x_buf[:c.M, c.ldx - c.K:]                          # a column slice that ends where the buffer's rows end
        return dys, x

    def reference(self, tiles="case"):
        dys, x = self.views()
        return reference(dys, x, reduced_tiles(self.c) if tiles == "case" else tiles)


def long_live_inputs(c):
    """Case 2: the live rows only (one per tile of M) -- (rows, dY[rows] [nt][nper], X[rows] [nt][K]); every other dY row
    is zero, the other X rows are whatever the device test fills in (they multiply zeros).  The same for both cases."""
    rows = live_rows(c)
    dy = rnd(len(rows), c.nper, seed=21)
    dy[-1] *= 2            # the share's last tile, the one a clamped prefetch would count twice: 2 x, so that it shows in db
    return rows, dy, rnd(len(rows), c.K, seed=22)


# ------------------------------------------------------------------------------------------------ mistake simulators
# Each returns the (dw, db) a kernel with that mistake would produce, computed from the reference alone.
def all_tiles(c):
    return list(range((c.M + T - 1) // T))


def mistake_skip_tile(inp, tile):
    """one reduced tile skipped"""
    base = reduced_tiles(inp.c)
    base = all_tiles(inp.c) if base is None else base
    r = inp.reference([t for t in base if t != tile])
    return r.dw, r.db


def mistake_bias_twice(inp, ref, tile):
    """the bias sum counts `tile` twice (the clamped prefetch of a share's last tile not masked out)"""
    dys, _ = inp.views()
    D = torch.cat([d.double() for d in dys], 1)
    return ref.dw, ref.db + D[rows_of_tiles([tile], inp.c.M)].sum(0)


def mistake_stale_slab(ref, value=1.0):
    """an empty share's weight and bias slab rows keep a finite stale value"""
    return ref.dw + value, ref.db + value


def mistake_segment_swap(inp):
    """segment 2's result computed from segment 1's dY"""
    dys, x = inp.views()
    dys = list(dys)
    dys[2] = dys[1]
    r = reference(dys, x, reduced_tiles(inp.c))
    return r.dw, r.db


def _pieces2(a):
    h = a.float().bfloat16().float()
    m = (a.float() - h).bfloat16().float()
    return h.double(), m.double()


def mistake_bf16x3(inp):
    """bf16x3 arithmetic: two pieces per element, the products ah*bh + ah*bm + am*bh, exact accumulation"""
    dys, x = inp.views()
    tiles = reduced_tiles(inp.c)
    D, X = torch.cat(list(dys), 1), x
    if tiles is not None:
        r = rows_of_tiles(tiles, inp.c.M)
        D, X = D[r], X[r]
    dh, dm = _pieces2(D)
    xh, xm = _pieces2(X)
    return dh.t() @ xh + dh.t() @ xm + dm.t() @ xh, D.double().sum(0)
