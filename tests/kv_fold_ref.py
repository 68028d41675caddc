"""fp64 references, derived error bounds, case tables and mistake simulators for the K | V fold (gct_kv_fold_fwd,
gct_kv_fold_wgrad, gct_kv_fold_dbz), each entry point taken in isolation with its inputs exact
(tests/test_kv_fold_ref_host.py runs them on the CPU, tests/test_kv_fold_edges_gpu.py holds the kernels to them).

References, all in fp64 (segment i of the stack: k_linear (i even) / v_linear (i odd) weight of layer i / 2, [d][dm]):
    fwd     wstack [layers * 2d][dm] = the weights stacked,  c = wstack b_z + biases,  a = wstack W_z  (W_z [dm][lat])
    wgrad   dW [2d][dm] = P W_z^T + s (x) b_z   (rows < d: dw0, the others: dw1),  db0 | db1 = s       (P [2d][lat])
    dbz     db_z [dm] = wstack^T s over rows rows

Bounds (derived, not measured on the kernels), u = 2^-24, 1.01 for the second-order terms as in tests/wgrad_ref.py:
    wstack  a copy: bit-exact.
    c       every element is a sum of dm products and the bias.  Whatever the order (fma chains per lane, a butterfly
            over the lanes, the bias last), no term passes through more than dm + 1 roundings: one per fma it takes part
            in or per addition of partial sums above it -- at most dm, each joins at least one new term -- and one for
            the bias addition.  Adding an exact zero (no bias, lanes without a column) rounds nothing.
                |c - ref| <= (dm + 1) u 1.01 (|W| |b_z| + |b|)
    a       the dgrad problem rows = layers * 2d, N = dm, K' = lat of gct_linear_dgrad under the route the library
            reports for the call: gemm_ref.bound with terms = dm -- drop = DROP[mode] on the bf16 routes (with the planes
            of W_z, in the bf16 modes), 0 on the fp32 routes.
    planes  hi + mid + lo of a_planes reproduces a bit for bit; elements beyond numel of each plane are not written.
    dW      one fma per latent column in a fixed order (products with the zero fill of a ragged K chunk add exact
            zeros), then one fma for s b_z:   |dW - ref| <= (lat + 1) u 1.01 (|P| |W_z|^T + |s| |b_z|^T);   db = s exactly.
    db_z    32-row fma chains, their partial sums dealt to 8 lanes, the 8 sums added in a fixed order: no term passes
            through more than min(rows, 32) + (ceil(parts / 8) - 1) + (min(parts, 8) - 1) roundings (the sums of lanes
            without a part are exact zeros), which is rows with one part and <= 32 (parts - 1) + 1 <= rows with more:
                |db_z - ref| <= rows u 1.01 |wstack|^T |s|;   bit-identical between two calls.
Where a bound is 0 the result must be exact (wgrad_ref.ratio)."""
from collections import namedtuple

import torch

from tests import gemm_ref as G
from tests.wgrad_ref import BF16X3, BF16X6, DROP, F32, U, ratio, rnd   # noqa: F401  (one statement of DROP and u)

MODES = (F32, BF16X6, BF16X3)
MODE_NAMES = {F32: "f32", BF16X6: "bf16x6", BF16X3: "bf16x3"}
KVF_T, KVF_K, KVF_ROWS, MAX_LAYERS = 64, 32, 32, 16        # csrc/gemm.hip: wgrad tile, its K chunk, rows of a dbz part

# ------------------------------------------------------------------------------------------------ the case tables
FwdCase = namedtuple("FwdCase", "layers d dm lat")
WgradCase = namedtuple("WgradCase", "d dm lat")
DbzCase = namedtuple("DbzCase", "rows dm")

FWD_CASES = [FwdCase(1, 4, 4, 4),            # the smallest legal call: one lane, one float4
             FwdCase(2, 40, 72, 36),         # d != dm, nothing a multiple of 32
             FwdCase(3, 64, 260, 128),       # a second, ragged pass of the copy loop
             FwdCase(16, 8, 516, 20),        # the table's limit; three passes of the copy loop, the last ragged
             FwdCase(2, 64, 64, 32)]         # the geometry of tests/test_kv_fold_gpu.py
WGRAD_CASES = [WgradCase(2, 4, 4),           # one thread's rows straddle dw0 | dw1; d % 4 != 0
               WgradCase(40, 72, 36),        # ragged tiles both ways, a ragged second K chunk, the boundary inside a tile
               WgradCase(37, 68, 68),        # d % 4 != 0: the boundary inside one thread's four rows; three K chunks
               WgradCase(64, 64, 128),       # full tiles, four full K chunks (the prefetch alone)
               WgradCase(96, 132, 32)]       # three row tiles, three column tiles (the last ragged), one K chunk
DBZ_CASES = [DbzCase(1, 1), DbzCase(31, 7), DbzCase(33, 257), DbzCase(257, 260), DbzCase(2048, 36)]


def case_id(c):
    return type(c).__name__[:-4].lower() + "-" + "x".join(str(v) for v in c)


def dbz_parts(c):
    return (c.rows + KVF_ROWS - 1) // KVF_ROWS


# ------------------------------------------------------------------------------------------------ inputs (CPU, fp32)
class FwdInputs:
    """2 * layers separately allocated weights [d][dm] and biases [d] (segment i scaled by 1 + i / 2, so that a segment
    mix-up shows), W_z [dm][lat], b_z [dm]"""

    def __init__(self, c, seed=0):
        self.c = c
        n = 2 * c.layers
        self.scales = [1.0 + 0.5 * i for i in range(n)]
        self.w = [rnd(c.d, c.dm, seed=seed + 100 + i) * (self.scales[i] * c.dm ** -0.5) for i in range(n)]
        self.b = [rnd(c.d, seed=seed + 200 + i) * (0.5 * self.scales[i]) for i in range(n)]
        self.wz = rnd(c.dm, c.lat, seed=seed + 1) * c.lat ** -0.5
        self.bz = rnd(c.dm, seed=seed + 2)


class WgradInputs:
    def __init__(self, c, seed=0):
        self.c = c
        self.p = rnd(2 * c.d, c.lat, seed=seed + 11)
        self.s = rnd(2 * c.d, seed=seed + 12)
        self.wz = rnd(c.dm, c.lat, seed=seed + 13) * c.lat ** -0.5
        self.bz = rnd(c.dm, seed=seed + 14)


class DbzInputs:
    def __init__(self, c, seed=0):
        self.c = c
        self.wstack = rnd(c.rows, c.dm, seed=seed + 21)
        self.s = rnd(c.rows, seed=seed + 22)


def inputs(c):
    return {FwdCase: FwdInputs, WgradCase: WgradInputs, DbzCase: DbzInputs}[type(c)](c)


# ------------------------------------------------------------------------------------------------ references and bounds
FwdRef = namedtuple("FwdRef", "wstack c Sc a gemm")          # wstack fp32 (exact); gemm: gemm_ref.Ref of a = wstack W_z
WgradRef = namedtuple("WgradRef", "dw S db")                 # dw, S [2d][dm] fp64; db [2d] fp32 (exact)
DbzRef = namedtuple("DbzRef", "dbz S")


def reference_fwd(inp, bias=True, w=None):
    """bias False: the call without b_addrs; w: other stacked weights than the inputs' (the mistake simulators)"""
    c = inp.c
    wstack = torch.cat(inp.w) if w is None else w
    W, bz, wz = wstack.double(), inp.bz.double(), inp.wz.double()
    b = torch.cat(inp.b).double() if bias else torch.zeros(W.shape[0], dtype=torch.float64)
    a, Sa = W @ wz, W.abs() @ wz.abs()
    floor = 3 * 2.0 ** -126 * (W.abs().sum(1)[:, None] + wz.abs().sum(0)[None, :])
    return FwdRef(wstack, W @ bz + b, W.abs() @ bz.abs() + b.abs(), a, G.Ref(a, Sa, floor, c.dm))


def bound_c(ref, c):
    return (c.dm + 1) * U * 1.01 * ref.Sc


def bound_a(ref, mode, out8):
    """gemm_ref.bound of the dgrad problem under the route out8 (gct_gemm_last_route / gct_linear_dgrad_route)"""
    return G.bound(ref.gemm, mode, out8)


def reference_wgrad(inp):
    P, s, wz, bz = inp.p.double(), inp.s.double(), inp.wz.double(), inp.bz.double()
    return WgradRef(P @ wz.t() + s[:, None] * bz[None, :], P.abs() @ wz.abs().t() + s.abs()[:, None] * bz.abs()[None, :],
                    inp.s.clone())


def bound_w(ref, c):
    return (c.lat + 1) * U * 1.01 * ref.S


def reference_dbz(inp):
    W, s = inp.wstack.double(), inp.s.double()
    return DbzRef(W.t() @ s, W.abs().t() @ s.abs())


def bound_dbz(ref, c):
    return c.rows * U * 1.01 * ref.S


def planes_sum(planes, numel):
    """fp32 [numel]: hi + mid + lo of int16 planes [3][>= numel] (exact in fp64, exactly an fp32 value when they split one)"""
    p = planes[:, :numel].to(torch.int32) << 16
    return p.view(torch.float32).double().sum(0).float()


# ------------------------------------------------------------------------------------------------ the fold's algebra
def unfolded(z, wz, bz, wkv, bkv, dkv):
    """the formulas of the model as written: e = z W_z^T + b_z feeds every layer's K | V projection (all fp64)"""
    e = z @ wz.t() + bz
    de = sum(dy @ w for dy, w in zip(dkv, wkv))
    return dict(kvb=[e @ w.t() + b for w, b in zip(wkv, bkv)], dW_kv=[dy.t() @ e for dy in dkv],
                db_kv=[dy.sum(0) for dy in dkv], dW_z=de.t() @ z, db_z=de.sum(0), dz=de @ wz)


def folded(z, wz, bz, wkv, bkv, dkv):
    """the same through A_l = W_kv,l W_z, c_l = W_kv,l b_z + b_kv,l, P_l = dkv_l^T z, s_l = colsum(dkv_l): the header's
    formulas (include/gctplus_hip.h)"""
    A = [w @ wz for w in wkv]
    cc = [w @ bz + b for w, b in zip(wkv, bkv)]
    P = [dy.t() @ z for dy in dkv]
    s = [dy.sum(0) for dy in dkv]
    return dict(kvb=[z @ a.t() + c for a, c in zip(A, cc)],
                dW_kv=[p @ wz.t() + sl[:, None] * bz[None, :] for p, sl in zip(P, s)], db_kv=s,
                dW_z=sum(w.t() @ p for w, p in zip(wkv, P)), db_z=sum(w.t() @ sl for w, sl in zip(wkv, s)),
                dz=sum(dy @ a for dy, a in zip(dkv, A)))


# ------------------------------------------------------------------------------------------------ mistake simulators
# Each returns what a kernel with that mistake would leave, computed from the inputs and the reference alone.
def mistake_first_k_chunk_only(inp):
    """wgrad: only the first 32-wide K chunk accumulated"""
    P, wz = inp.p.double()[:, :KVF_K], inp.wz.double()[:, :KVF_K]
    return P @ wz.t() + inp.s.double()[:, None] * inp.bz.double()[None, :]


def _reads_on(t):
    """[rows][ceil32(lat)]: row r holds the flat elements r * lat ... r * lat + ceil32(lat) - 1 (zeros beyond the end)"""
    rows, lat = t.shape
    wide = (lat + KVF_K - 1) // KVF_K * KVF_K
    flat = torch.cat([t.double().reshape(-1), torch.zeros(wide, dtype=torch.float64)])
    return flat[torch.arange(rows)[:, None] * lat + torch.arange(wide)[None, :]]


def mistake_ragged_chunk_reads_on(inp):
    """wgrad: the ragged last K chunk reads on into the next row of P and of W_z instead of zeros"""
    return _reads_on(inp.p) @ _reads_on(inp.wz).t() + inp.s.double()[:, None] * inp.bz.double()[None, :]


def mistake_no_s_bz(inp):
    """wgrad: the s (x) b_z term left out"""
    return inp.p.double() @ inp.wz.double().t()


def mistake_dw1_rows_into_dw0(inp, ref):
    """wgrad: rows >= d written behind dw0 (m * dm from dw0) instead of into dw1, which keeps its NaN fill"""
    dw = ref.dw.clone()
    dw[inp.c.d:] = float("nan")
    return dw


def mistake_stack_row_stride_d(inp):
    """stack: row i of a segment read at i * d instead of i * dm (zeros beyond the weight's end) -> stacked weights"""
    c = inp.c
    out = []
    for w in inp.w:
        flat = torch.cat([w.reshape(-1), torch.zeros(c.d * c.dm)])
        out.append(flat[torch.arange(c.d)[:, None] * c.d + torch.arange(c.dm)[None, :]])
    return torch.cat(out)


def mistake_segment_one_off(inp):
    """stack: the first workgroup (4 rows) of every segment but the first takes the segment before it
    -> (stacked weights, stacked biases)"""
    c = inp.c
    w, b = [t.clone() for t in inp.w], [t.clone() for t in inp.b]
    for i in range(1, len(w)):
        w[i][:4], b[i][:4] = inp.w[i - 1][:4], inp.b[i - 1][:4]
    return torch.cat(w), torch.cat(b)


def mistake_no_b_kv(inp, ref):
    """stack: b_kv left out of c"""
    return ref.c - torch.cat(inp.b).double()


def mistake_last_ragged_part_dropped(inp):
    """dbz: the last part, of fewer than 32 rows, is not summed"""
    full = inp.c.rows // KVF_ROWS * KVF_ROWS
    return inp.wstack.double()[:full].t() @ inp.s.double()[:full]


def mistake_first_8_parts_only(inp):
    """dbz: each of the 8 lanes sums its first part only"""
    n = 8 * KVF_ROWS
    return inp.wstack.double()[:n].t() @ inp.s.double()[:n]


def mistake_cols_from_256_unwritten(ref):
    """dbz: only the first column block (blockIdx.y == 0) written; the others keep their NaN fill"""
    out = ref.dbz.clone()
    out[256:] = float("nan")
    return out
