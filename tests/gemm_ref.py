"""fp64 reference, derived error bound, case table and mistake simulators for gct_linear_fwd / gct_linear_dgrad
(tests/test_gemm_routes_host.py runs them on the CPU, tests/test_gemm_routes_gpu.py holds the kernels to them).

Both sides multiply by one weight matrix W [nseg * nper][K] (segments stacked, leading dimension ldw):
    forward   acc = x W^T + b     x [M][K]            S = |x| |W|^T + |b|     terms = K (+ 1 with a bias)
    dgrad     acc = dY W          dY [M][nseg * nper] S = |dY| |W|            terms = nseg * nper
all in fp64, per output element.

Bound on the accumulator (derived, not measured on the kernels).  u = 2^-24, ns = slabs summed for the row (0 where the
row's kernel applies its own epilogue):

    |out - acc| <= (drop + (terms + ns) * u * 1.01) * S + floor

drop: what the bf16 piece products leave out (wgrad_ref.DROP; 0 on the routes that run fp32 MFMA whatever the mode);
(terms + ns) u: one fp32 rounding per term of the accumulation chain -- a K-split chain is shorter, the slab sum then
adds one rounding per slab (1.01 covers the second-order terms); floor: bf16 pieces below the normal range are flushed,
as in wgrad_ref.bound_w.

Epilogues (s = float32(1) / (float32(1) - float32(p)), computed here exactly as the library computes it):
    EPI_BIAS, pre of EPI_GELU_DROP, DEPI_STORE     the bound
    DEPI_ACCUM        dx = base + acc              the bound + 1.01 u |result|            (the final addition rounds once)
    EPI_DROP_RESID    y = resid + s acc (kept)     s * bound + 1.01 u (s |acc| + |result|)   (product and sum round once
                      y = resid exactly (dropped)                                             each)
    GELU-shaped outputs follow the fp64 function of the reference at the suite's elementwise tolerances
    (test_linear_epilogues_no_dropout) plus the bound times the function's Lipschitz constant L:
    y of EPI_GELU_DROP(_SAVE) = s gelu(acc):  s (2e-5 + 2e-5 |gelu(acc)| + L bound)
    saved gelu'(acc), DEPI_GELU_BWD and DEPI_MUL_SAVED = s acc f, f = gelu'(pre) or the saved factor:
                                              s (2e-5 + 1e-4 |acc f| + L bound)
    L = 1.13: gelu'(x) = Phi(x) + x phi(x) has gelu''(x) = phi(x) (2 - x^2) = 0 at x = +-sqrt(2), where gelu' takes its
    extremes Phi(sqrt 2) + sqrt(2) phi(sqrt 2) = 0.9214 + 0.2076 = 1.129 and -0.129: |gelu'| <= 1.13 bounds the slope of
    gelu and the factor |f| that multiplies the accumulator's error (pre and the saved factor are inputs, exact);
    gelu' itself has slope |gelu''| <= 2 phi(0) = 0.80 < L.
Dropout masks are tests/rng_ref.py's, compared exactly: a dropped element is exactly 0 (or exactly resid), a kept one
whose reference magnitude exceeds its allowance must not be.  Rows of padding quads (quad map entry < 0) carry zero
operands; forward outputs on them (functions of the bias alone under an unspecified mask) are not compared."""
import math
from collections import namedtuple

import numpy as np
import torch

from tests import rng_ref as R
from tests.wgrad_ref import BF16X3, BF16X6, DROP, F32, U, ratio, rnd   # noqa: F401  (one statement of DROP and u)

# GCT_GEMM_ROUTE_* (include/gctplus_hip.h)
NONE, X6S, X6_SPLITK_ALL, PANEL_THIN, PANEL32, F32_SMALL, X6, F32_FAST, F32_VEC, F32_SCALAR = -1, 0, 1, 2, 3, 4, 5, 6, 7, 8
KINDS = (X6S, X6_SPLITK_ALL, PANEL_THIN, PANEL32, F32_SMALL, X6, F32_FAST, F32_VEC, F32_SCALAR)
KIND_NAMES = {NONE: "none", X6S: "X6S", X6_SPLITK_ALL: "X6_SPLITK_ALL", PANEL_THIN: "PANEL_THIN", PANEL32: "PANEL32",
              F32_SMALL: "F32_SMALL", X6: "X6", F32_FAST: "F32_FAST", F32_VEC: "F32_VEC", F32_SCALAR: "F32"}
BF16_KINDS = (X6S, X6_SPLITK_ALL, X6)
TAIL_NONE, TAIL_SMALL, TAIL_SLABS = 0, 1, 2
EPI_BIAS, EPI_GELU_DROP, EPI_DROP_RESID, EPI_GELU_DROP_SAVE = 0, 1, 2, 3        # GCT_EPI_*
DEPI_STORE, DEPI_ACCUM, DEPI_GELU_BWD, DEPI_MUL_SAVED = 0, 1, 2, 3              # GCT_DEPI_*
EPI_NAMES = {"fwd": ("bias", "gelu_drop", "drop_resid", "gelu_drop_save"), "dgrad": ("store", "accum", "gelu_bwd", "mul_saved")}
LIP = 1.13
SEED, SITE = (0x1234 << 32) | 99, 7                    # above 2^32: the high word is part of the key


# ------------------------------------------------------------------------------------------------ the case table
# One Case = one gct_linear_fwd / gct_linear_dgrad problem on W [nseg * nper][K].  lda: leading dimension of x (fwd) / of
# dY (dgrad); ldc: of y (fwd) / dx (dgrad).  route: the kind the planner must report in bf16x6 and bf16x3 mode, f32_route:
# in fp32 mode; f32: run the fp32 mode on the GPU too.  splits / tail / m1 / tsplits: out8[1..4] in the bf16 modes.
# ws: "full" = a workspace of the *_ws_bytes query, "none" = no workspace.  aligned: False = the A operand starts 4 bytes off
# a 16-byte boundary.  quad: the rows are a quad compaction (two padding quads at the end); pre_full: pre keeps the
# forward's row space and is read through the quad map.
Case = namedtuple("Case", "side name route f32_route M K nseg nper lda ldw ldc epi p planes bias ws aligned quad pre_full "
                          "f32 splits tail m1 tsplits")


def _case(side, name, route, f32_route, M, K, nseg, nper, *, lda=None, ldw=None, ldc=None, epi=0, p=0.0, planes=True,
          bias=True, ws="full", aligned=True, quad=False, pre_full=False, f32=False, splits=1, tail=TAIL_NONE, m1=0, tsplits=1):
    n = nseg * nper
    wa, wc = (K, n) if side == "fwd" else (n, K)
    return Case(side, name, route, f32_route, M, K, nseg, nper, lda or wa, ldw or K, ldc or wc, epi, p, planes,
                bias and side == "fwd", ws, aligned, quad, pre_full, f32, splits, tail, m1, tsplits)


_T = dict(m1=32768)
CASES = [
    # --- X6S: 64 x 128 bf16 tiles over the whole problem
    _case("fwd", "x6s-shape", X6S, F32_SMALL, 3072, 64, 1, 256, f32=True),
    _case("fwd", "x6s-shape-raggedN-ld-quad-gelu", X6S, F32_SMALL, 3000, 64, 1, 264, lda=72, ldc=272, epi=EPI_GELU_DROP, p=0.1,
          quad=True),
    _case("fwd", "x6s-3seg-raggedM-ld", X6S, F32_SMALL, 3001, 64, 3, 128, lda=72, ldw=72, ldc=392),
    _case("fwd", "x6s-seg128", X6S, F32_SMALL, 3072, 1056, 2, 128),
    _case("dgrad", "x6s-shape", X6S, F32_FAST, 3072, 256, 1, 64, f32=True),
    _case("dgrad", "x6s-3seg-raggedN-ld-quad-gelubwd", X6S, F32_FAST, 3000, 264, 3, 64, lda=200, ldc=272, epi=DEPI_GELU_BWD,
          p=0.1, quad=True, pre_full=True),
    # --- X6, no tail
    _case("fwd", "x6-plain", X6, F32_FAST, 4224, 64, 1, 1024, f32=True),
    _case("fwd", "x6-plain-3seg-raggedM-ld", X6, F32_FAST, 4201, 64, 3, 512, lda=72, ldc=1544),
    _case("fwd", "x6-plain-raggedN-quad-resid", X6, F32_FAST, 4200, 64, 1, 1032, epi=EPI_DROP_RESID, p=0.1, quad=True),
    _case("fwd", "x6-no-ws-no-tail", X6, F32_FAST, 33000, 256, 1, 256, ws="none"),
    _case("dgrad", "x6-plain-accum", X6, F32_FAST, 4224, 1024, 1, 64, epi=DEPI_ACCUM, f32=True),
    _case("dgrad", "x6-plain-3seg-raggedN-ld-quad-gelubwd", X6, F32_FAST, 4200, 1032, 3, 64, lda=200, ldc=1040,
          epi=DEPI_GELU_BWD, p=0.1, quad=True, pre_full=True),
    # --- X6 + the tail rows on 64 x 128 tiles
    _case("fwd", "x6-small-tail", X6, F32_FAST, 33000, 256, 1, 256, tail=TAIL_SMALL, **_T),
    _case("fwd", "x6-small-tail-gelu-drop", X6, F32_FAST, 33000, 256, 1, 256, epi=EPI_GELU_DROP, p=0.1, tail=TAIL_SMALL, **_T),
    _case("fwd", "x6-small-tail-raggedN-ld-quad-resid", X6, F32_FAST, 33000, 256, 1, 264, lda=264, ldc=272, epi=EPI_DROP_RESID,
          p=0.1, quad=True, tail=TAIL_SMALL, **_T),
    _case("fwd", "x6-small-tail-3seg", X6, F32_FAST, 32816, 256, 3, 256, tail=TAIL_SMALL, **_T),
    _case("dgrad", "x6-small-tail-quad-gelubwd", X6, F32_FAST, 33000, 256, 1, 256, epi=DEPI_GELU_BWD, p=0.1, quad=True,
          pre_full=True, tail=TAIL_SMALL, **_T),
    _case("dgrad", "x6-small-tail-3seg-mulsaved", X6, F32_FAST, 33000, 256, 3, 64, lda=200, ldc=260, epi=DEPI_MUL_SAVED, p=0.1,
          tail=TAIL_SMALL, **_T),
    # --- X6 + the tail rows K-split into slabs + fix-up
    _case("fwd", "x6-slab-tail", X6, F32_FAST, 33000, 1280, 1, 256, tail=TAIL_SLABS, tsplits=8, **_T),
    _case("fwd", "x6-slab-tail-resid-drop", X6, F32_FAST, 33000, 1280, 1, 256, epi=EPI_DROP_RESID, p=0.1, tail=TAIL_SLABS,
          tsplits=8, **_T),
    _case("fwd", "x6-slab-tail-raggedN-ld-quad-gelusave", X6, F32_FAST, 33000, 1280, 1, 264, lda=1288, ldc=272,
          epi=EPI_GELU_DROP_SAVE, p=0.1, quad=True, tail=TAIL_SLABS, tsplits=8, **_T),
    _case("dgrad", "x6-slab-tail", X6, F32_FAST, 33000, 256, 1, 1280, tail=TAIL_SLABS, tsplits=8, **_T),
    _case("dgrad", "x6-slab-tail-3seg-quad-mulsaved", X6, F32_FAST, 33000, 256, 3, 384, ldc=260, epi=DEPI_MUL_SAVED, p=0.1,
          quad=True, pre_full=True, tail=TAIL_SLABS, tsplits=8, **_T),
    # --- X6_SPLITK_ALL
    _case("fwd", "splitk-all-8", X6_SPLITK_ALL, PANEL32, 1024, 2048, 1, 256, splits=8, f32=True),
    _case("fwd", "splitk-all-4", X6_SPLITK_ALL, PANEL32, 2048, 1024, 1, 256, splits=4),
    _case("fwd", "splitk-all-not-at-K1024", PANEL32, PANEL32, 1024, 1024, 1, 256),
    _case("fwd", "splitk-all-3seg-raggedM-ld", X6_SPLITK_ALL, PANEL32, 1101, 2048, 3, 256, lda=2056, ldc=776, splits=8),
    _case("fwd", "splitk-all-raggedN-quad-resid", X6_SPLITK_ALL, F32_SMALL, 1100, 2048, 1, 264, epi=EPI_DROP_RESID, p=0.1,
          quad=True, splits=8),
    _case("dgrad", "splitk-all-accum", X6_SPLITK_ALL, F32_FAST, 1024, 256, 1, 2048, epi=DEPI_ACCUM, splits=8, f32=True),
    _case("dgrad", "splitk-all-3seg-raggedN-ld-quad-mulsaved", X6_SPLITK_ALL, F32_FAST, 1100, 264, 3, 704, ldc=272,
          epi=DEPI_MUL_SAVED, p=0.1, quad=True, pre_full=True, splits=8),
    # --- the fp32 routes (the same in every mode)
    _case("fwd", "panel-thin-N1", PANEL_THIN, PANEL_THIN, 77, 256, 1, 1, ldc=4, f32=True),
    _case("fwd", "panel-thin-N31", PANEL_THIN, PANEL_THIN, 77, 256, 1, 31, ldc=40),
    _case("fwd", "panel32", PANEL32, PANEL32, 77, 256, 1, 96, f32=True),
    _case("fwd", "f32-small-1", F32_SMALL, F32_SMALL, 77, 64, 1, 128, f32=True),
    _case("fwd", "f32-small-split", F32_SMALL, F32_SMALL, 77, 384, 1, 128, ldc=136, splits=3, f32=True),
    _case("fwd", "f32-small-split-ragged-K-range-resid", F32_SMALL, F32_SMALL, 77, 416, 1, 128, epi=EPI_DROP_RESID, p=0.1,
          splits=3),
    _case("fwd", "f32-fast-no-planes", F32_FAST, F32_FAST, 4224, 64, 1, 1024, planes=False),
    _case("dgrad", "f32-fast-no-planes", F32_FAST, F32_FAST, 4224, 1024, 1, 64, planes=False),
    _case("fwd", "f32-vec-K36", F32_VEC, F32_VEC, 300, 36, 1, 128, f32=True),
    _case("dgrad", "f32-vec-nseg36", F32_VEC, F32_VEC, 300, 128, 1, 36),
    _case("fwd", "f32-scalar-K30", F32_SCALAR, F32_SCALAR, 300, 30, 1, 128, f32=True),
    _case("dgrad", "f32-scalar-nper30", F32_SCALAR, F32_SCALAR, 300, 128, 1, 30),
    _case("fwd", "f32-scalar-x-plus-4-bytes", F32_SCALAR, F32_SCALAR, 300, 64, 1, 128, aligned=False),
]


def case_id(c):
    return f"{c.side}-{c.name}"


def case(side, name):
    return next(c for c in CASES if c.side == side and c.name == name)


def widths(c):
    """(columns of the A operand, columns of the output)"""
    n = c.nseg * c.nper
    return (c.K, n) if c.side == "fwd" else (n, c.K)


def reads_pre(c):
    return c.side == "dgrad" and c.epi in (DEPI_GELU_BWD, DEPI_MUL_SAVED)


def quad_map(c):
    """int32 [M / 4]: the original quad of every compact quad (ascending draw out of 5/4 as many), the last two padding"""
    if not c.quad:
        return None
    assert c.M % 4 == 0
    nq = c.M // 4
    g = torch.Generator().manual_seed(4242)
    q = torch.sort(torch.randperm(nq + nq // 4, generator=g)[:nq])[0].to(torch.int32)
    q[-2:] = -1
    return q


def pre_rows(c):
    return 4 * (c.M // 4 + c.M // 16) if (c.quad and c.pre_full) else 0


def scale_of(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def gelu(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))


def gelu_grad(v):
    return 0.5 * (1 + torch.erf(v / math.sqrt(2))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


class Inputs:
    """CPU operands of a case: a [M][lda], w [nseg * nper][ldw], bias, resid / base [M][ldc], pre, the quad map and the
    dropout mask of the output."""

    def __init__(self, c):
        self.c = c
        wa, wc = widths(c)
        n = c.nseg * c.nper
        self.a = rnd(c.M, c.lda, seed=1)
        self.w = rnd(n, c.ldw, seed=2) * c.K ** -0.5 if c.side == "fwd" else rnd(n, c.ldw, seed=2) * n ** -0.5
        self.bias = rnd(n, seed=3) if c.bias else None
        self.quads = quad_map(c)
        self.dead = None
        if self.quads is not None:
            self.dead = (self.quads < 0).repeat_interleave(4)
            self.a[self.dead] = 0
        self.extra = None                                        # resid (EPI_DROP_RESID) or the base of DEPI_ACCUM
        if (c.side == "fwd" and c.epi == EPI_DROP_RESID) or (c.side == "dgrad" and c.epi == DEPI_ACCUM):
            self.extra = rnd(c.M, c.ldc, seed=4)
        q = None if self.quads is None else self.quads.numpy()
        self.keep = torch.as_tensor(R.dropout_keep(SEED, SITE, c.p, c.M, wc, quad_of_row=q))
        if self.dead is not None:
            self.keep[self.dead] = True                          # rows of padding quads: zero operands, the mask is moot
        self.pre = None                                          # dgrad: the pre-activation / saved factor that is read
        if reads_pre(c):
            rows = pre_rows(c) or c.M
            v = rnd(rows, c.ldc, seed=5)
            if c.epi == DEPI_MUL_SAVED:                          # what EPI_GELU_DROP_SAVE leaves: gelu'(v) where kept, else 0
                kf = torch.as_tensor(R.dropout_keep(SEED, SITE, c.p, rows, c.ldc))
                v = torch.where(kf, gelu_grad(v.double()).float(), torch.zeros(()))
            self.pre = v

    def pre_of_rows(self, compact_space=False):
        """[M][wc] fp64: the pre row every output row reads (zeros for padding quads)"""
        c = self.c
        wc = widths(c)[1]
        if not pre_rows(c) or compact_space:
            return self.pre[:c.M, :wc].double()
        rows = (self.quads.long().clamp_min(0) * 4).repeat_interleave(4) + torch.arange(4).repeat(c.M // 4)
        out = self.pre[rows, :wc].double()
        out[self.dead] = 0
        return out


Ref = namedtuple("Ref", "acc S floor terms")


def reference(inp):
    c = inp.c
    wa, wc = widths(c)
    A, W = inp.a[:, :wa].double(), inp.w[:, :c.K].double()
    if c.side == "fwd":
        acc, S = A @ W.t(), A.abs() @ W.abs().t()
        if inp.bias is not None:
            acc, S = acc + inp.bias.double(), S + inp.bias.double().abs()
        wsum = W.abs().sum(1)
        terms = c.K + (1 if inp.bias is not None else 0)
    else:
        acc, S = A @ W, A.abs() @ W.abs()
        wsum = W.abs().sum(0)
        terms = c.nseg * c.nper
    floor = 3 * 2.0 ** -126 * (A.abs().sum(1)[:, None] + wsum[None, :])
    return Ref(acc, S, floor, terms)


def slabs_of_rows(M, out8):
    """fp64 [M]: slabs summed for every row under the route out8 reports"""
    ns = torch.zeros(M, dtype=torch.float64)
    if out8[0] in (X6_SPLITK_ALL, F32_SMALL) and out8[1] > 1:
        ns += out8[1]
    if out8[0] == X6 and out8[2] == TAIL_SLABS:
        ns[out8[3]:] = out8[4]
    return ns


def bound(ref, mode, out8):
    drop = DROP[mode] if out8[0] in BF16_KINDS else 0.0
    ns = slabs_of_rows(ref.acc.shape[0], out8)
    return (drop + (ref.terms + ns[:, None]) * U * 1.01) * ref.S + ref.floor


# ------------------------------------------------------------------------------------------------ outputs and their judge
def expected(inp, ref, acc=None, keep=None, pre_compact=False):
    """{name: fp64 [M][wc]}: what the call leaves in the output ("out") and in the saved pre ("pre"), from the accumulator
    `acc` (default: the reference's) under the mask `keep` (default: the case's)"""
    c = inp.c
    acc = ref.acc if acc is None else acc
    keep = inp.keep if keep is None else keep
    s = scale_of(c.p)
    wc = widths(c)[1]
    zero = torch.zeros((), dtype=torch.float64)
    if c.side == "fwd":
        if c.epi == EPI_BIAS:
            return {"out": acc}
        if c.epi == EPI_DROP_RESID:
            return {"out": inp.extra[:, :wc].double() + torch.where(keep, acc * s, zero)}
        out = torch.where(keep, gelu(acc) * s, zero)
        return {"out": out, "pre": acc if c.epi == EPI_GELU_DROP else torch.where(keep, gelu_grad(acc), zero)}
    if c.epi == DEPI_STORE:
        return {"out": acc}
    if c.epi == DEPI_ACCUM:
        return {"out": inp.extra[:, :wc].double() + acc}
    f = inp.pre_of_rows(pre_compact)
    if c.epi == DEPI_GELU_BWD:
        return {"out": torch.where(keep, acc * gelu_grad(f) * s, zero)}
    return {"out": torch.where(f != 0, acc * f * s, zero)}


def allowances(inp, ref, B):
    """{name: (allowance fp64 [M][wc], dropped bool [M][wc] or None, value a dropped element holds exactly)}"""
    c = inp.c
    s = scale_of(c.p)
    wc = widths(c)[1]
    acc = ref.acc
    dropped = ~inp.keep
    if c.side == "fwd":
        if c.epi == EPI_BIAS:
            return {"out": (B, None, None)}
        if c.epi == EPI_DROP_RESID:
            res = inp.extra[:, :wc].double()
            return {"out": (s * B + 1.01 * U * (s * acc.abs() + (res + s * acc).abs()), dropped, res)}
        a_y = s * (2e-5 + 2e-5 * gelu(acc).abs() + LIP * B)
        if c.epi == EPI_GELU_DROP:
            return {"out": (a_y, dropped, 0.0), "pre": (B, None, None)}
        return {"out": (a_y, dropped, 0.0), "pre": (2e-5 + 1e-4 * gelu_grad(acc).abs() + LIP * B, dropped, 0.0)}
    if c.epi == DEPI_STORE:
        return {"out": (B, None, None)}
    if c.epi == DEPI_ACCUM:
        return {"out": (B + 1.01 * U * (inp.extra[:, :wc].double() + acc).abs(), None, None)}
    f = inp.pre_of_rows()
    if c.epi == DEPI_GELU_BWD:
        return {"out": (s * (2e-5 + 1e-4 * (acc * gelu_grad(f)).abs() + LIP * B), dropped, 0.0)}
    return {"out": (s * (2e-5 + 1e-4 * (acc * f).abs() + LIP * B), f == 0, 0.0)}


def judge(inp, ref, B, got):
    """worst |got - expected| / allowance over the outputs of a call (got: {name: [M][wc]}); inf when a dropped element is
    not exactly its dropped value, or a kept one whose expected distance from it exceeds the allowance sits on it"""
    c = inp.c
    want = expected(inp, ref)
    worst = 0.0
    live = None
    if c.side == "fwd" and inp.dead is not None:
        live = ~inp.dead                                         # forward rows of padding quads are not compared
    for name, (allow, dropped, dval) in allowances(inp, ref, B).items():
        g, w = got[name].double(), want[name]
        if live is not None:
            if not torch.isfinite(g).all():
                return math.inf
            g, w, allow = g[live], w[live], allow[live]
            dropped = None if dropped is None else dropped[live]
            dval = dval[live] if torch.is_tensor(dval) else dval
        worst = max(worst, ratio(g, w, allow))
        if dropped is not None:
            dv = dval if torch.is_tensor(dval) else torch.full_like(w, dval)
            on_it = g == dv
            if (dropped & ~on_it).any():
                return math.inf
            if (~dropped & on_it & ((w - dv).abs() > allow)).any():
                return math.inf
    return worst


# ------------------------------------------------------------------------------------------------ mistake simulators
# Each returns the outputs ({name: tensor}) a kernel with that mistake would leave, computed from the reference alone.
def _slab_rows(c, out8):
    return slabs_of_rows(c.M, out8) > 0


def mistake_tail_mask_at_row_0(inp, ref, out8):
    """the tail launch draws its dropout mask at row 0 instead of at its first row"""
    m1 = out8[3]
    keep = inp.keep.clone()
    keep[m1:] = inp.keep[:inp.c.M - m1]
    return expected(inp, ref, keep=keep)


def _k_ranges(c, ns):
    red = c.K if c.side == "fwd" else c.nseg * c.nper
    per = -(-(red // 32) // ns) * 32
    return [(z * per, min(red, (z + 1) * per)) for z in range(ns)]


def mistake_last_split_missing(inp, ref, out8):
    """the fix-up sums one slab too few"""
    c = inp.c
    rows = _slab_rows(c, out8)
    ns = int(slabs_of_rows(c.M, out8).max())
    k0, k1 = _k_ranges(c, ns)[-1]
    A, W = inp.a[:, :widths(c)[0]].double(), inp.w[:, :c.K].double()
    part = A[:, k0:k1] @ W[:, k0:k1].t() if c.side == "fwd" else A[:, k0:k1] @ W[k0:k1]
    acc = ref.acc.clone()
    acc[rows] -= part[rows]
    return expected(inp, ref, acc=acc)


def mistake_bias_per_slab(inp, ref, out8):
    """every slab carries the bias"""
    ns = slabs_of_rows(inp.c.M, out8)
    return expected(inp, ref, acc=ref.acc + (ns - 1).clamp_min(0)[:, None] * inp.bias.double()[None, :])


def mistake_fixup_skips_ragged_patch(inp, ref, out8):
    """the fix-up leaves the last, ragged 4-row patch unwritten (NaN, as the tests fill the outputs)"""
    c = inp.c
    assert c.M % 4
    out = {k: v.clone() for k, v in expected(inp, ref).items()}
    for v in out.values():
        v[c.M // 4 * 4:] = float("nan")
    return out


def mistake_segment_boundary_one_tile_off(inp, ref, tile=128):
    """the first tile of weight rows of segment 1 is read one tile further"""
    c = inp.c
    assert c.nseg >= 2 and c.nper >= 2 * tile or c.nseg == 3
    w = inp.w.clone()
    w[c.nper:c.nper + tile] = inp.w[c.nper + tile:c.nper + 2 * tile]
    shifted = Inputs.__new__(Inputs)
    shifted.__dict__.update(inp.__dict__)
    shifted.w = w
    return expected(inp, ref, acc=reference(shifted).acc)


def mistake_ldc_for_n(inp, ref, out8):
    """the fix-up reads the dense [M][N] slabs with the output's leading dimension"""
    c = inp.c
    n = widths(c)[1]
    assert c.ldc > n
    flat = ref.acc.reshape(-1)
    idx = torch.arange(c.M)[:, None] * c.ldc + torch.arange(n)[None, :]
    acc = torch.where(idx < flat.numel(), flat[idx.clamp_max(flat.numel() - 1)], torch.zeros((), dtype=torch.float64))
    return expected(inp, ref, acc=acc)


def mistake_pre_in_compact_space(inp, ref):
    """pre read at the compact row instead of through the quad map"""
    return expected(inp, ref, pre_compact=True)


# ------------------------------------------------------------------------------------------------ the library's queries
def ws_bytes_of(lib, c):
    n = c.nseg * c.nper
    return int(lib.gct_linear_fwd_ws_bytes(c.M, c.K, n) if c.side == "fwd" else lib.gct_linear_dgrad_ws_bytes(c.M, n, c.K))


def query(lib, c, mode, ws_bytes=None):
    """out8 of gct_linear_fwd_route / gct_linear_dgrad_route for the case (ws_bytes None: the case's own workspace)"""
    import ctypes
    if ws_bytes is None:
        ws_bytes = ws_bytes_of(lib, c) if c.ws == "full" else 0
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    if c.side == "fwd":
        rc = lib.gct_linear_fwd_route(c.M, c.K, c.nseg, c.nper, c.lda, c.ldw, c.ldc, c.epi, int(c.aligned), int(c.planes),
                                      int(c.bias), mode, ws_bytes, ctypes.addressof(out))
    else:
        rc = lib.gct_linear_dgrad_route(c.M, c.nseg, c.nper, c.K, c.lda, c.ldw, c.ldc, c.epi, int(c.aligned), int(c.planes),
                                        mode, ws_bytes, ctypes.addressof(out))
    assert rc == 0, (case_id(c), rc)
    return tuple(out)


def launches_of(out8):
    """kernel launches that out8[0], [1], [2] imply"""
    if out8[0] == NONE:
        return 0
    if out8[0] == X6:
        return 1 + out8[2]
    return 2 if out8[1] > 1 else 1
