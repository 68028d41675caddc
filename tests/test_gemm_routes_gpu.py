"""gct_linear_fwd / gct_linear_dgrad against tests/gemm_ref.py (fp64 on the CPU, derived bound, tests/rng_ref.py masks) on
every route gct_linear_fwd_route / gct_linear_dgrad_route report, through raw library calls, in bf16x6 and bf16x3 mode
and, for the rows marked for it, in fp32 mode:

  X6S (shape rule, 128-row weight segments, dgrad), X6 plain, X6 with the tail rows on 64 x 128 tiles, X6 with the tail
  rows K-split into slabs + fix-up, X6_SPLITK_ALL, PANEL_THIN, PANEL32, F32_SMALL with one and with several K ranges (a
  ragged last one), F32_FAST, F32_VEC, F32 -- each bf16 route once more with three segments, a ragged M, an N that is no
  multiple of the tile, leading dimensions wider than the rows and a quad map (pre in the forward's row space for the
  dgrad epilogues that read it); the tails with dropout epilogues (the tail continues the head's coordinates).

Every call: outputs start as NaN in buffers ld wide, the columns beyond the row must stay NaN; ws is exactly the
*_ws_bytes query long plus a 4 KiB guard that must stay untouched, once NaN-filled and once zero-filled (bit-equal
results); the call repeated (bit-equal: deterministic).  gct_gemm_last_route must equal the shape query, which must equal
the route the row names; the launch counters move by what the route implies.  Short workspaces (one slab fewer, none)
degrade the slab routes as the query says, within the bound, without a write past the shortened workspace.  One capture
of the small-tile-tail row: one kernel, no tail.  tests/test_gemm_routes_host.py shows that these inputs tell a kernel's
likely mistakes apart by >= 100 x the bound.

Measured on MI355X, worst error / allowance per route (bf16x6, bf16x3; printed at the end of the module with -s):
  forward  X6S 0.056, 0.102   X6 0.062, 0.119   X6 + small-tile tail 0.019, 0.042   X6 + slab tail 0.004, 0.008
           X6_SPLITK_ALL 0.0014, 0.010   PANEL_THIN 0.011   PANEL32 0.011   F32_SMALL 0.044 (0.077 in fp32 mode at 3072 x 256)
           F32_SMALL with 3 K ranges 0.005   F32_FAST 0.083   F32_VEC 0.077   F32 0.109
  dgrad    X6S 0.056, 0.094   X6 0.072, 0.103   X6 + small-tile tail 0.010, 0.039   X6 + slab tail 0.004, 0.009
           X6_SPLITK_ALL 0.0004, 0.004   F32_FAST 0.090   F32_VEC 0.098   F32 0.128
No case is above 0.5: the allowance grows with the reduction length, the error of a sum of random terms with its root, so
the long reductions (K = 1280, 2048) sit lowest.  The 49 tests take 24 s, the longest (33000 x 264 x 1280 with the saved
GELU derivative, three modes' worth of calls and an fp64 reference) 2.9 s."""
import ctypes

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
WORST = {}                       # worst error / allowance per route label
MODE_NAMES = {G.F32: "f32", G.BF16X6: "bf16x6", G.BF16X3: "bf16x3"}


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib, ops
    yield _lib.load()
    ops.gemm_set_mode(G.BF16X6)
    for key in sorted(WORST):
        print(f"[gemm routes] worst err / allowance  {key}: {WORST[key][0]:.4f}  ({WORST[key][1]})")


def _check(rc, what):
    from gct_plus_amd import _lib
    _lib.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def counters(lib):
    out = (ctypes.c_int64 * 2)()
    _check(lib.gct_gemm_launch_counts(ctypes.addressof(out)), "gct_gemm_launch_counts")
    return {"fp32": int(out[0]), "x6": int(out[1]), "x6k": int(lib.gct_gemm_x6_kernel_launches()),
            "x3": int(lib.gct_gemm_x3_launches())}


def counter_moves(out8, mode):
    """what one call of this route adds to the counters: fp32 / x6 count calls, x6k / x3 the bf16 tile kernels launched (the
    fix-up kernel is none of them; the panel32 and 64 x 64 fp32 kernels are not counted at all)"""
    kind = out8[0]
    bf = kind in G.BF16_KINDS
    k = (1 + (1 if out8[2] else 0)) if bf else 0
    return {"fp32": 1 if kind in (G.PANEL_THIN, G.F32_FAST, G.F32_VEC, G.F32_SCALAR) else 0,
            "x6": 1 if bf and mode == G.BF16X6 else 0, "x6k": k if mode == G.BF16X6 else 0, "x3": k if mode == G.BF16X3 else 0}


def last_route(lib):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    _check(lib.gct_gemm_last_route(ctypes.addressof(out)), "gct_gemm_last_route")
    return tuple(out)


class Operands:
    """device copies of a case's operands and their addresses"""

    def __init__(self, inp):
        from gct_plus_amd import ops
        c = self.c = inp.c
        lead = 0 if c.aligned else 1
        self.a = torch.cat([torch.full((lead,), 7.0), inp.a.reshape(-1), torch.full((4 - lead,), 7.0)]).to(DEV)
        self.pa = self.a.data_ptr() + 4 * lead
        self.w = inp.w.reshape(-1).to(DEV)
        self.planes = ops.split_planes(self.w) if c.planes else None
        self.bias = None if inp.bias is None else inp.bias.to(DEV)
        self.extra = None if inp.extra is None else inp.extra.to(DEV)
        self.pre = None if inp.pre is None else inp.pre.to(DEV)
        # 32 readable entries behind the map, as the header asks (a tile's rows beyond M look theirs up)
        self.quads = None if inp.quads is None else torch.cat([inp.quads, torch.full((32,), -1, dtype=torch.int32)]).to(DEV)
        torch.cuda.synchronize()

    def seg(self, base, stride_elems):
        return [base + 4 * s * stride_elems if s < self.c.nseg else None for s in range(3)]


class Buffers:
    """the outputs (NaN, ld wide) and a workspace of exactly `ws_bytes` (filled with `fill`) + the guard"""

    def __init__(self, c, op, fill, ws_bytes):
        wc = G.widths(c)[1]
        self.out = torch.full((c.M, c.ldc), float("nan"), device=DEV)
        if c.side == "dgrad" and c.epi == G.DEPI_ACCUM:
            self.out[:, :wc] = op.extra[:, :wc]
        self.pre = None
        if c.side == "fwd" and c.epi in (G.EPI_GELU_DROP, G.EPI_GELU_DROP_SAVE):
            self.pre = torch.full((c.M, c.ldc), float("nan"), device=DEV)
        self.ws_bytes = ws_bytes
        self.ws = None
        if ws_bytes is not None:
            assert ws_bytes % 4 == 0
            self.ws = torch.empty(ws_bytes + GUARD, dtype=torch.uint8, device=DEV)
            self.ws[:ws_bytes].view(torch.float32).fill_(fill)
            self.ws[ws_bytes:] = 0xA5


def launch(lib, c, op, buf):
    """the raw library call (no synchronisation: it can be captured)"""
    w = op.seg(op.w.data_ptr(), c.nper * c.ldw)
    wp = None if op.planes is None else op.planes.data_ptr()
    pstride = 0 if op.planes is None else op.planes.stride(0)
    ws = None if buf.ws is None else buf.ws.data_ptr()
    wsb = 0 if buf.ws is None else buf.ws_bytes
    qm = None if op.quads is None else op.quads.data_ptr()
    if c.side == "fwd":
        b = op.seg(op.bias.data_ptr(), c.nper) if op.bias is not None else [None] * 3
        y = op.seg(buf.out.data_ptr(), c.nper)
        _check(lib.gct_linear_fwd(op.pa, c.lda, c.M, c.K, w[0], w[1], w[2], c.ldw, wp, pstride, b[0], b[1], b[2], c.nseg,
                                  c.nper, y[0], y[1], y[2], c.ldc, c.epi,
                                  op.extra.data_ptr() if c.epi == G.EPI_DROP_RESID else None,
                                  None if buf.pre is None else buf.pre.data_ptr(), c.p, G.SEED, G.SITE, ws, wsb, qm, _st()),
               "gct_linear_fwd")
    else:
        dy = op.seg(op.pa, c.nper)
        _check(lib.gct_linear_dgrad(dy[0], dy[1], dy[2], c.lda, c.M, c.nseg, c.nper, w[0], w[1], w[2], c.ldw, wp, pstride,
                                    c.K, buf.out.data_ptr(), c.ldc, c.epi, None if op.pre is None else op.pre.data_ptr(),
                                    c.p, G.SEED, G.SITE, ws, wsb, qm, G.pre_rows(c), _st()), "gct_linear_dgrad")


def collect(c, buf):
    """the outputs on the host, after the checks every call gets: the row's columns written, the others and the guard not"""
    torch.cuda.synchronize()
    wc = G.widths(c)[1]
    got = {"out": buf.out.cpu()}
    if buf.pre is not None:
        got["pre"] = buf.pre.cpu()
    for name, t in got.items():
        assert torch.isfinite(t[:, :wc]).all(), f"{G.case_id(c)}: an element of {name} was not written"
        assert torch.isnan(t[:, wc:]).all(), f"{G.case_id(c)}: {name} was written beyond column {wc}"
    if buf.ws is not None:
        assert bool((buf.ws[buf.ws_bytes:] == 0xA5).all()), f"{G.case_id(c)}: the call wrote past ws + {buf.ws_bytes}"
    return got


def call(lib, c, op, fill, ws_bytes):
    buf = Buffers(c, op, fill, ws_bytes)
    launch(lib, c, op, buf)
    return collect(c, buf)


def bits_equal(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def label(c, out8):
    tail = {0: "", 1: " + small-tile tail", 2: " + slab tail"}[out8[2]]
    return f"{c.side} {G.KIND_NAMES[out8[0]]}{tail}" + (f" x{out8[1]}" if out8[1] > 1 else "")


def hold(c, mode, inp, ref, out8, got, tag=""):
    wc = G.widths(c)[1]
    r = G.judge(inp, ref, G.bound(ref, mode, out8), {k: v[:, :wc] for k, v in got.items()})
    key = f"{label(c, out8)} [{MODE_NAMES[mode]}]"
    print(f"  {G.case_id(c)}{tag} {key}: err / allowance {r:.4f}")
    if r > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (r, G.case_id(c) + tag)
    assert r <= 1.0, f"{G.case_id(c)}{tag} {key}: worst error is {r:.3f} x the allowance"


def run(lib, c, mode, inp, ref, op):
    """the three calls of a case in one mode (ws NaN, ws zero, ws NaN again), the route, the counters, the values"""
    from gct_plus_amd import ops
    ops.gemm_set_mode(mode)
    out8 = G.query(lib, c, mode)
    if mode == G.F32:
        assert out8[0] == c.f32_route, (G.case_id(c), out8)
    else:
        assert out8[:5] == (c.route, c.splits, c.tail, c.m1, c.tsplits), (G.case_id(c), out8)
    ws_bytes = G.ws_bytes_of(lib, c) if c.ws == "full" else None
    c0 = counters(lib)
    got = call(lib, c, op, float("nan"), ws_bytes)
    c1 = counters(lib)
    assert last_route(lib) == out8, (G.case_id(c), mode, last_route(lib), out8)
    assert {k: c1[k] - c0[k] for k in c0} == counter_moves(out8, mode), (G.case_id(c), mode, out8, c0, c1)
    assert bits_equal(got, call(lib, c, op, 0.0, ws_bytes)), f"{G.case_id(c)}: the result depends on what ws held"
    assert bits_equal(got, call(lib, c, op, float("nan"), ws_bytes)), f"{G.case_id(c)}: two identical calls differ"
    hold(c, mode, inp, ref, out8, got)
    return out8


# ------------------------------------------------------------------------------------------------ every row of the table
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_route_and_values(lib, c):
    from gct_plus_amd import ops
    inp = G.Inputs(c)
    ref = G.reference(inp)
    op = Operands(inp)
    try:
        for mode in (G.BF16X6, G.BF16X3) + ((G.F32,) if c.f32 else ()):
            run(lib, c, mode, inp, ref, op)
    finally:
        ops.gemm_set_mode(G.BF16X6)


def test_every_route_kind_is_asserted_by_a_case_here():
    assert {c.route for c in G.CASES} == set(G.KINDS)


# ------------------------------------------------------------------------------------------------ short workspaces
@pytest.mark.parametrize("side,name", [("fwd", "x6-slab-tail"), ("fwd", "splitk-all-8"), ("fwd", "f32-small-split"),
                                       ("dgrad", "x6-slab-tail")])
def test_short_workspaces_degrade_the_slab_routes(lib, side, name):
    from gct_plus_amd import ops
    c = G.case(side, name)
    inp = G.Inputs(c)
    ref = G.reference(inp)
    op = Operands(inp)
    mode = G.BF16X6
    ops.gemm_set_mode(mode)
    full = G.query(lib, c, mode)
    slabs = max(full[1], full[4])
    assert slabs > 1 and full[6] % slabs == 0
    for ws_bytes in (full[6] - full[6] // slabs, 0):
        out8 = G.query(lib, c, mode, ws_bytes)
        assert out8[6] <= ws_bytes and (out8[1], out8[4]) < (full[1], full[4]) or out8[0] != full[0], (ws_bytes, out8, full)
        got = call(lib, c, op, float("nan"), ws_bytes)           # the guard sits right behind the shortened workspace
        assert last_route(lib) == out8, (ws_bytes, last_route(lib), out8)
        hold(c, mode, inp, ref, out8, got, tag=f" (ws {ws_bytes} B)")


# ------------------------------------------------------------------------------------------------ capture
def test_a_captured_stream_gets_one_kernel_and_no_tail(lib):
    from gct_plus_amd import ops
    c = G.case("fwd", "x6-small-tail")
    inp = G.Inputs(c)
    ref = G.reference(inp)
    op = Operands(inp)
    mode = G.BF16X6
    ops.gemm_set_mode(mode)
    ws_bytes = G.ws_bytes_of(lib, c)
    call(lib, c, op, float("nan"), ws_bytes)                     # not captured: head + tail
    assert last_route(lib)[2] == G.TAIL_SMALL
    buf = Buffers(c, op, float("nan"), ws_bytes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    k0 = counters(lib)
    with torch.cuda.graph(graph):                                # one stream, no branches
        launch(lib, c, op, buf)
    out8 = last_route(lib)
    assert out8 == (G.X6, 1, 0, 0, 1, 1, 0, 0), out8
    assert counters(lib)["x6k"] == k0["x6k"] + 1
    graph.replay()
    got = collect(c, buf)
    hold(c, mode, inp, ref, out8, got, tag=" (captured)")
