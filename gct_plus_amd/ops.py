"""Thin, allocation-explicit Python wrappers over the C ABI (include/gctplus_hip.h).

Every function takes/returns fp32 CUDA tensors, enqueues on the current torch stream and
never synchronises.  No autograd here: `engine.py` composes these into hand-written
forward/backward passes.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import contextlib
import math
import os
import threading
import weakref
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import check

EPI_BIAS, EPI_GELU_DROP, EPI_DROP_RESID, EPI_GELU_DROP_SAVE = 0, 1, 2, 3
DEPI_STORE, DEPI_ACCUM, DEPI_GELU_BWD, DEPI_MUL_SAVED = 0, 1, 2, 3


def _L():
    return _lib.load()


_raw_stream, _cur_dev = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _st():
    # the raw handle of the current stream: torch.cuda.current_stream() builds a Stream object through several
    # Python layers (8.7 us per call, a third of the host time of a training step)
    return _raw_stream(_cur_dev())


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.GctError(f"{name}: expected a CUDA (ROCm) tensor; gct_plus_amd has no CPU path")
    if t.dtype != dtype:
        raise _lib.GctError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


# ---------------------------------------------------------------------------- side stream
# Weight-gradient GEMMs are off the critical path of a backward pass (nothing downstream needs
# dW until the optimiser / all-reduce), so they are launched on a SIDE stream: their workgroups
# fill the partial last round of the critical-path dgrad GEMMs and the gaps of the small
# bandwidth kernels.  Correctness bookkeeping (all stream-ordered, no host syncs):
#   * the side stream waits for an event recorded on the main stream at launch (inputs ready);
#   * inputs are record_stream()'ed so the caching allocator cannot recycle them early;
#   * every buffer a pending wgrad READS is remembered (by storage pointer) with the wgrad's
#     completion event; any main-stream op that WRITES into an existing buffer waits on it first
#     (the in-place residual-gradient buffer `g` of engine.py is the case that matters);
#   * join_side() makes the main stream wait for everything (called at the end of each trunk's
#     backward, before autograd / all-reduce / Adam can touch the gradients).
# Measured on MI355X (bench.py, B=512): 112.5 ms/step without vs 112.7 ms with the side stream (round 1); with the
# bf16x6 kernels 49.2 without, 50.3 with, 50.7-50.9 with the side stream at low and the main stream at high priority
# (round 3: one 144 KB workgroup fills a CU, so a second stream only interleaves whole workgroups and splits the L2)
# -- no gain, so it is OFF by default (GCT_SIDE_STREAM=1 enables it; tests cover both settings).
SIDE_ENABLED = os.environ.get("GCT_SIDE_STREAM", "0") != "0"
_SIDE = {}
_PENDING = {}


def _side_stream(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _SIDE.get(idx)
    if st is None:
        st = torch.cuda.Stream(device=idx)
        _SIDE[idx] = st
    return st


def _wait_pending(t):
    """Main stream is about to WRITE into tensor t: wait for side-stream readers of its storage."""
    if _PENDING and t is not None:
        ev = _PENDING.pop(t.untyped_storage().data_ptr(), None)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)


def join_side(device=None):
    if _SIDE:
        cur = torch.cuda.current_stream()
        for st in _SIDE.values():
            cur.wait_stream(st)
        _PENDING.clear()


# ------------------------------------------------------------------------------ workspace
_WS = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Per (device, stream) scratch buffer, grown geometrically; kernels on one stream are
    ordered, so consecutive ops may reuse it."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _st())
    buf = _WS.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        n = max(int(nbytes * 1.25) // 4 + 64, 1 << 20)
        buf = torch.empty(n, dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


# Deferred slab reductions (csrc/reduce.hip): a layer's backward pass records the reductions that end its weight-gradient
# GEMMs and Norm backward kernels and runs them as ONE launch at the end of the layer (engine.enc_layer_bwd /
# dec_layer_bwd): 106 launches of 5-10 us per step become 12.  While recording, the workspaces of those calls must stay
# intact until the flush: kept_workspace() hands out consecutive regions of a second buffer instead of the shared one.
DEFER_REDUCTIONS = os.environ.get("GCT_DEFER_REDUCTIONS", "1") != "0"
class _DeferState(threading.local):        # per thread, like the library's record of pending reductions
    def __init__(self):
        self.d = {"on": False, "off": 0, "demand": 0, "want": 0}


_DEFER_TL = _DeferState()
_ARENA = {}


def kept_workspace(nbytes: int, device) -> torch.Tensor:
    """Workspace of a call whose slab reduction may be deferred: the shared scratch buffer when nothing is being
    recorded, otherwise a fresh region of the arena (the recorded reductions are flushed first when it is full)."""
    if not _DEFER_TL.d["on"]:
        return workspace(nbytes, device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), _st())
    n = (int(nbytes) + 255) // 256 * 64            # floats, 256-byte regions
    _DEFER_TL.d["demand"] += n
    buf = _ARENA.get(key)
    if buf is None or _DEFER_TL.d["off"] + n > buf.numel():
        # full (or absent): what was recorded so far is reduced now, on this stream, before anything overwrites it
        check(_L().gct_reduce_defer_flush(_st()), "gct_reduce_defer_flush")
        _DEFER_TL.d["off"] = 0
        if buf is None or n > buf.numel():
            buf = _ARENA[key] = torch.empty(max(n, _DEFER_TL.d["want"], 1 << 22), dtype=torch.float32, device=device)
    out = buf[_DEFER_TL.d["off"]:_DEFER_TL.d["off"] + n]
    _DEFER_TL.d["off"] += n
    return out


class deferred_reductions:
    """with deferred_reductions(): ... -- the slab reductions issued inside by THIS thread run as one launch at exit
    (bit-identical results: same lanes and summation order per destination).  Not while a graph is being captured, not
    with the side stream (its weight gradients are ordered by events, not by this stream), not nested."""

    def __enter__(self):
        self.mine = (DEFER_REDUCTIONS and not _DEFER_TL.d["on"] and not SIDE_ENABLED
                     and not torch.cuda.is_current_stream_capturing())
        if self.mine:
            key = (torch.cuda.current_device(), _st())
            buf = _ARENA.get(key)
            if buf is not None and buf.numel() < _DEFER_TL.d["want"]:
                del _ARENA[key]                    # grown on first use below: a whole layer fits from the second layer on
            _DEFER_TL.d.update(on=True, off=0, demand=0)
            check(_L().gct_reduce_defer_begin(), "gct_reduce_defer_begin")
        return self

    def __exit__(self, et, ev, tb):
        if self.mine:
            _DEFER_TL.d["on"] = False
            _DEFER_TL.d["want"] = max(_DEFER_TL.d["want"], _DEFER_TL.d["demand"])
            rc = _L().gct_reduce_defer_end(_st())
            if et is None:
                check(rc, "gct_reduce_defer_end")
        return False


_WS_NEED = {}


def _ws_need(fn: str, a: int, b: int, c: int) -> int:
    """Workspace size queries of the library (pure functions of the shape), remembered per shape."""
    key = (fn, a, b, c)
    v = _WS_NEED.get(key)
    if v is None:
        v = _WS_NEED[key] = int(getattr(_L(), fn)(a, b, c))
    return v


# ----------------------------------------------------------------------------------- norm
def norm_fwd(x2d, alpha, bias, eps=1e-6, out=None):
    _chk(x2d, "norm_fwd.x")
    rows, d = x2d.shape
    y = torch.empty_like(x2d) if out is None else out
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    check(_L().gct_norm_fwd(_p(x2d), _p(alpha), _p(bias), _p(y), _p(mean), _p(rstd), rows, d, eps,
                            _st()), "gct_norm_fwd")
    return y, mean, rstd


def norm_bwd(dy, x2d, alpha, mean, rstd, dalpha, dbias, dres=None, out=None, eps=1e-6, live=None, drop=None):
    """live (LiveRows): dy / dres / out are quad-compacted rows [live.Mc, d]; x2d, mean, rstd stay in the forward's
    row space -- or, when the forward itself ran on the compact rows (live.fwd), are compact too.
    drop = (buffer, p, seed, site): also write dropout_bwd(result) with that mask into buffer (the
    gradient's next consumer is the sub-layer whose output dropout used (seed, site))."""
    src_rows, d = x2d.shape
    rows = src_rows if live is None else live.Mc
    if live is not None and live.fwd:
        src_rows = 0                                   # x / mean / rstd are compact: the map only places the dropout bits
    dx = (torch.empty_like(x2d) if live is None else live.empty(d)) if out is None else out
    _wait_pending(out)
    if drop is not None:
        _wait_pending(drop[0])
    ws = kept_workspace(_L().gct_rowred_ws_bytes(rows, 2 * d), x2d.device)
    check(_L().gct_norm_bwd(_p(dy), _p(x2d), _p(alpha), _p(mean), _p(rstd), _p(dres), _p(dx),
                            _p(dalpha), _p(dbias), _p(ws), rows, d, eps,
                            None if live is None else _p(live.quad_list), src_rows,
                            None if drop is None else _p(drop[0]), 0.0 if drop is None else drop[1],
                            0 if drop is None else drop[2], 0 if drop is None else drop[3], _st()), "gct_norm_bwd")
    return dx


# ------------------------------------------------------------------------------ embedding
def embed_pe_fwd(tok, table, cond, pe2d, n_c, scale, p, seed, site, d=None):
    _chk(tok, "embed.tok", torch.int64)
    B, S = tok.shape
    if table is not None:
        vocab, d = table.shape
    else:
        vocab = 1
    out = torch.empty(B * (S + n_c), d, dtype=torch.float32, device=pe2d.device)
    check(_L().gct_embed_pe_fwd(_p(tok), _p(table), _p(cond), _p(pe2d), _p(out), B, S, n_c, d, vocab,
                                scale, p, seed, site, _st()), "gct_embed_pe_fwd")
    return out


def embed_pe_bwd(dout, tok, dtable, dcond, n_c, scale, p, seed, site, d=None):
    B, S = tok.shape
    if dtable is not None:
        vocab, d = dtable.shape
    else:
        vocab = 1
    # kept: the slab reduction that ends it is recorded, not launched, under deferred_reductions()
    ws = kept_workspace(_L().gct_embed_ws_bytes(B, S, d, vocab), dout.device)
    check(_L().gct_embed_pe_bwd(_p(dout), _p(tok), _p(dtable), _p(dcond), _p(ws), B, S, n_c, d, vocab,
                                scale, p, seed, site, _st()), "gct_embed_pe_bwd")


# --------------------------------------------------------------------------------- linear
# Optional per-launch timing of the GEMM family (bench.py roofline leg): when PROFILE is a
# dict, every gct_linear_* launch is bracketed by HIP events on the launch stream and logged as
# (kernel kind, flops, start event, end event).  Off (None) in normal operation.
PROFILE = None
PROFILE_KINDS = None      # None: every GEMM kind; else a set such as {"gemm_fwd"}


class _Timed:
    def __init__(self, kind, flops, nbytes=0):
        self.kind, self.flops, self.nbytes = kind, flops, nbytes

    def __enter__(self):
        self.on = PROFILE is not None and (PROFILE_KINDS is None or self.kind in PROFILE_KINDS)
        if self.on:
            self.c0 = gemm_launch_counts()[1]
            self.k0 = _L().gct_gemm_x6_kernel_launches()
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            # launches that took the bf16x6 kernels are logged under their own key
            kind = self.kind + "[x6]" if gemm_launch_counts()[1] > self.c0 else self.kind
            PROFILE.setdefault(kind, []).append((self.flops, self.e0, self.e1))
            PROFILE["_x6_kernel_launches:" + kind] = PROFILE.get("_x6_kernel_launches:" + kind, 0) + \
                (_L().gct_gemm_x6_kernel_launches() - self.k0)
            # algorithmic HBM bytes of the calls (every operand read once, every result written once)
            PROFILE["_bytes:" + kind] = PROFILE.get("_bytes:" + kind, 0) + self.nbytes


def _seg3(ts: Sequence[Optional[torch.Tensor]]):
    ts = list(ts) + [None] * (3 - len(ts))
    return [_p(t) for t in ts]


# ---- bf16x6 GEMM mode: pre-split weight planes --------------------------------------------------
GEMM_F32, GEMM_BF16X6 = 0, 1
GEMM_BF16X3 = 2   # opt-in: two bf16 pieces, three products, < 3.02 * 2^-16 |a*b| dropped per product (gemm_x6.inc)
_PLANES = []     # [(base_ptr, end_ptr, planes tensor (int16 [3, numel]), numel)]


def gemm_set_mode(mode: int):
    check(_L().gct_gemm_set_mode(int(mode)), "gct_gemm_set_mode")


def gemm_get_mode() -> int:
    return _L().gct_gemm_get_mode()


def gemm_x3_launches() -> int:
    """Launches of the bf16x3 (2-piece) GEMM kernels since load."""
    return int(_L().gct_gemm_x3_launches())


def gemm_launch_counts():
    """(launches of the fp32-MFMA tile kernels, launches of the bf16x6 kernels) since load."""
    import ctypes
    out = (ctypes.c_int64 * 2)()
    check(_L().gct_gemm_launch_counts(ctypes.cast(out, ctypes.c_void_p)), "gct_gemm_launch_counts")
    return int(out[0]), int(out[1])


def wgrad_route(M, nseg, nper, K, lddy, ldx, aligned16=True, want_bias=True, mode=None):
    """(kind, nsplit, rows per split, bias fused) of gct_linear_wgrad for a shape (gct_wgrad_route: no launch)."""
    import ctypes
    out = (ctypes.c_int64 * 4)()
    check(_L().gct_wgrad_route(M, nseg, nper, K, lddy, ldx, int(aligned16), int(want_bias),
                               gemm_get_mode() if mode is None else int(mode), ctypes.addressof(out)), "gct_wgrad_route")
    return tuple(int(v) for v in out)


def linear_fwd_route(M, K, nseg, nper, ldx=None, ldw=None, ldy=None, epi=EPI_BIAS, aligned16=True, have_planes=True,
                     have_bias=True, mode=None, ws_bytes=None):
    """out8 of gct_linear_fwd_route (no launch): (route kind, slabs, tail, first tail row, tail slabs, launches, bytes of
    ws written, 0).  ws_bytes None: a workspace of gct_linear_fwd_ws_bytes."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    if ws_bytes is None:
        ws_bytes = _L().gct_linear_fwd_ws_bytes(M, K, nseg * nper)
    check(_L().gct_linear_fwd_route(M, K, nseg, nper, K if ldx is None else ldx, K if ldw is None else ldw,
                                    nseg * nper if ldy is None else ldy, epi, int(aligned16), int(have_planes),
                                    int(have_bias), gemm_get_mode() if mode is None else int(mode), int(ws_bytes),
                                    ctypes.addressof(out)), "gct_linear_fwd_route")
    return tuple(int(v) for v in out)


def linear_dgrad_route(M, nseg, nper, K, lddy=None, ldw=None, lddx=None, depi=DEPI_STORE, aligned16=True,
                       have_planes=True, mode=None, ws_bytes=None):
    """out8 of gct_linear_dgrad_route (no launch), as linear_fwd_route."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    if ws_bytes is None:
        ws_bytes = _L().gct_linear_dgrad_ws_bytes(M, nseg * nper, K)
    check(_L().gct_linear_dgrad_route(M, nseg, nper, K, nseg * nper if lddy is None else lddy, K if ldw is None else ldw,
                                      K if lddx is None else lddx, depi, int(aligned16), int(have_planes),
                                      gemm_get_mode() if mode is None else int(mode), int(ws_bytes),
                                      ctypes.addressof(out)), "gct_linear_dgrad_route")
    return tuple(int(v) for v in out)


def gemm_last_route():
    """out8 of gct_gemm_last_route: what the latest linear_fwd / linear_dgrad of this thread executed."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    check(_L().gct_gemm_last_route(ctypes.addressof(out)), "gct_gemm_last_route")
    return tuple(int(v) for v in out)


def split_planes(flat: torch.Tensor, planes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flat fp32 [numel] -> int16 [3, numel] holding the hi / mid / lo bf16 pieces of every element
    (exact: hi + mid + lo == x).  numel % 4 == 0."""
    _chk(flat, "flat")
    n = flat.numel()
    if planes is None:
        planes = torch.empty(3, n, dtype=torch.int16, device=flat.device)
    check(_L().gct_split_planes(_p(flat), n, _p(planes), planes.stride(0), _st()), "gct_split_planes")
    return planes


def _drop_planes(base: int, end: int):
    _PLANES[:] = [e for e in _PLANES if e[1] <= base or e[0] >= end]


def register_planes(flat: torch.Tensor, planes: torch.Tensor):
    """Weights that live inside `flat` are looked up in `planes` by linear_fwd / linear_dgrad.
    The registration dies with the `flat` tensor object (its address range may be handed to other
    tensors by the caching allocator afterwards) and replaces anything it overlaps."""
    base, end = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    known = any(e[0] == base and e[1] == end and e[4]() is flat for e in _PLANES)
    _drop_planes(base, end)
    _PLANES.append((base, end, planes, flat.numel(), weakref.ref(flat)))
    if not known:
        weakref.finalize(flat, _drop_planes, base, end)


def unregister_planes(flat: torch.Tensor):
    _drop_planes(flat.data_ptr(), flat.data_ptr() + flat.numel() * 4)


def _plane_ptr(ws_):
    """(pointer to plane 0 of ws_[0], plane stride) if every segment lies in one registered buffer."""
    if not _PLANES:
        return None, 0
    a = ws_[0].data_ptr()
    for base, end, planes, numel, ref in _PLANES:
        if base <= a < end:
            if ref() is None:
                return None, 0
            if all(base <= w.data_ptr() < end for w in ws_[1:]):
                return planes.data_ptr() + (a - base) // 2, planes.stride(0)
            return None, 0
    return None, 0


def linear_fwd(x2d, ws_: Sequence[torch.Tensor], bs: Sequence[Optional[torch.Tensor]],
               outs: Sequence[torch.Tensor], ldy: int, epi=EPI_BIAS, resid=None, pre=None,
               p=0.0, seed=0, site=0, splitk_ws: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
               live=None, planes=None):
    """y_s = epi(x @ w_s^T + b_s); outs are (views of) pre-allocated [M, nper] blocks with
    leading dimension ldy.  splitk_ws: force the skinny-M split-K kernel with this workspace; ws: a caller-owned
    workspace (>= gct_linear_fwd_ws_bytes) for the general path (fixed address: graph capture); live (LiveRows): the
    rows are quad-compacted -- the dropout masks of the fused epilogues are drawn at the original coordinates; planes:
    (address of plane 0 of ws_[0], plane stride) of weights that are not registered (KvFold)."""
    M, K = x2d.shape
    nper = ws_[0].shape[0]
    w = _seg3(ws_)
    b = _seg3(bs)
    y = _seg3(outs)
    need = _ws_need("gct_linear_fwd_ws_bytes", M, K, nper * len(ws_))     # skinny split-K slabs or bf16x6 tail slabs
    for t in (splitk_ws, ws):
        if t is not None and t.numel() * 4 < need:
            raise _lib.GctError(f"linear_fwd: workspace of {t.numel() * 4} B < {need} B "
                                f"(gct_linear_fwd_ws_bytes({M}, {K}, {nper * len(ws_)}))")
    if splitk_ws is not None:      # skinny-M path (decode): split-K through this workspace; no planes, no quad map
        wp, pstride, wsb, quad_map, timed = None, 0, splitk_ws, None, contextlib.nullcontext()
    else:
        wp, pstride = _plane_ptr(ws_) if planes is None else planes
        wsb = ws if ws is not None else (workspace(need, x2d.device) if need > 256 else None)
        quad_map = None if live is None else _p(live.quad_list)
        N = nper * len(ws_)
        nbytes = 4 * M * K + (6 if wp else 4) * N * K + 4 * N + 4 * M * N * (2 if epi in (EPI_GELU_DROP, EPI_DROP_RESID, EPI_GELU_DROP_SAVE) else 1)
        timed = _Timed("gemm_fwd", 2.0 * M * K * N, nbytes)
    with timed:
        check(_L().gct_linear_fwd(_p(x2d), x2d.stride(0), M, K, w[0], w[1], w[2], ws_[0].stride(0),
                                  wp, pstride, b[0], b[1], b[2], len(ws_), nper, y[0], y[1], y[2],
                                  ldy, epi, _p(resid), _p(pre), p, seed, site, _p(wsb),
                                  0 if wsb is None else wsb.numel() * 4, quad_map, _st()),
              "gct_linear_fwd")


def linear_dgrad(dys: Sequence[torch.Tensor], lddy: int, M: int, ws_: Sequence[torch.Tensor], dx,
                 depi=DEPI_STORE, pre=None, p=0.0, seed=0, site=0, live=None, pre_full=False, planes=None):
    nper, K = ws_[0].shape
    d = _seg3(dys)
    w = _seg3(ws_)
    _wait_pending(dx)
    with _Timed("gemm_dgrad", 2.0 * M * K * nper * len(ws_)):
        wp, pstride = _plane_ptr(ws_) if planes is None else planes
        need = _ws_need("gct_linear_dgrad_ws_bytes", M, nper * len(ws_), K)
        wsb = workspace(need, dx.device) if need > 256 else None
        check(_L().gct_linear_dgrad(d[0], d[1], d[2], lddy, M, len(ws_), nper, w[0], w[1], w[2],
                                    ws_[0].stride(0), wp, pstride, K, _p(dx), dx.stride(0), depi,
                                    _p(pre), p, seed, site, _p(wsb), 0 if wsb is None else wsb.numel() * 4,
                                    None if live is None else _p(live.quad_list),
                                    pre.shape[0] if (live is not None and pre is not None and pre_full) else 0,
                                    _st()), "gct_linear_dgrad")


def nonzero_row_tiles(x2d: torch.Tensor):
    """(list, count): ascending indices of the 32-row tiles of x2d that hold a non-zero element, and their
    number as a device scalar (no host round trip).  Feed to linear_wgrad(kt=...) for GEMMs whose dY rows are
    zero wherever x2d's are (the decoder backward under an ignore_index loss)."""
    _chk(x2d, "x2d")
    rows, cols = x2d.shape
    nt = (rows + 31) // 32
    lst = torch.empty(max(nt, 1), dtype=torch.int32, device=x2d.device)
    cnt = torch.empty(1, dtype=torch.int32, device=x2d.device)
    flags = torch.empty(max(nt, 1), dtype=torch.uint8, device=x2d.device)
    check(_L().gct_nonzero_row_tiles(_p(x2d), x2d.stride(0), rows, cols, _p(lst), _p(cnt), _p(flags), _st()),
          "gct_nonzero_row_tiles")
    return lst, cnt


_SKIPPED = {}
_SKIPPED_MSG = ("{} decoder rows that an earlier forward skipped (loss_rows: rows that do not reach the loss) received a "
                "non-zero gradient in its backward pass: that gradient was ignored, and the optimizer steps launched since "
                "then were skipped on the device (FusedAdam's guard), so no wrong update has been applied; this error is "
                "raised at the first host read-back after the fact.  Call the model without loss_rows "
                "(forward_propagation(..., skip_ignored=False)) for losses other than the reference's ignore_index "
                "cross-entropy.")


def assert_no_skipped_row_gradients():
    """Read the counter now (one synchronisation) and raise if it is non-zero: the trainer calls this at the end of an
    epoch so that a gradient on a skipped row in the LAST step of a run is reported too."""
    n = int(skipped_row_gradients().item())
    if n:
        skipped_row_gradients().zero_()
        raise _lib.GctError(_SKIPPED_MSG.format(n))


def skipped_row_gradients():
    """Device counter (int32[1], one per device) of gradient rows that fell on decoder rows a forward had skipped."""
    dev = torch.cuda.current_device()
    t = _SKIPPED.get(dev)
    if t is None:
        t = _SKIPPED[dev] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", dev))
    return t


class LiveRows:
    """Device-side description of the rows of a decoder gradient that are not identically zero, the check that makes
    shortcuts on them exact, and the compaction map of the decoder backward (csrc/liverows.hip).
      kt          feeds linear_wgrad(kt=...): lists every tile when the check failed -- no host decision needed;
      host()      reads the counters back (ONE device->host sync);
      quad_list / cstart / n_b / Mc  (after host()): rows are compacted in aligned quads, compact row 4i+e <->
                  original row 4*quad_list[i]+e, Mc compact rows (multiple of 128)."""
    SLACK = 256        # rows behind Mc in every compact buffer: attention stages whole L-row windows of a sample
    fwd = False        # True (instance): the FORWARD ran on these compact rows too (engine.decoder_trunk_fwd)

    def __init__(self, g2d, B, T, mask_u8, lists=True):
        _chk(g2d, "g2d")
        dev = g2d.device
        M = B * T
        assert g2d.shape[0] == M
        nt, nq = (M + 31) // 32, (M + 3) // 4
        i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)            # noqa: E731
        self.B, self.T, self.M, self.dev = B, T, M, dev
        self.live = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
        self.n_b, self.info = i32(B), i32(8)
        self.cstart = i32(B) if lists else None
        self.quad_list = i32(nq + 32) if lists else None
        qrank = i32(nq) if lists else None
        self.tile_list, self.tile_count = i32(nt), i32(1)
        flags = torch.empty(max(nt, 1), dtype=torch.uint8, device=dev)
        if mask_u8 is None:
            sb = sq = 0
        else:
            _chk(mask_u8, "live_rows.mask", torch.uint8)
            sb, sq = _mask_strides(mask_u8, B, T, T)
        check(_L().gct_live_rows(_p(g2d), g2d.stride(0), B, T, g2d.shape[1], _p(mask_u8), sb, sq, _p(self.live),
                                 _p(self.n_b), _p(self.info), _p(self.cstart), _p(self.quad_list), _p(qrank),
                                 _p(self.tile_list), _p(self.tile_count), _p(flags), _st()), "gct_live_rows")
        self.kt = (self.tile_list, self.tile_count)
        self._host = None
        self.Mc = None

    @classmethod
    def from_rows(cls, rows_u8, B, T, mask_u8):
        """The same maps from a given row set (rows_u8 [B, T], non-zero = live) instead of from a gradient: the decoder
        forward over the rows that reach the loss."""
        _chk(rows_u8, "live_rows.rows", torch.uint8)
        return cls(rows_u8.reshape(B * T, 1).to(torch.float32), B, T, mask_u8)

    def _fill_host(self, v):
        self._host = dict(n_live=v[0], violations=v[1], nonprefix=v[2], tiles=v[3], padded=v[4], quads=v[5], empty=v[6])
        self.Mc = v[4]

    def host(self):
        if self._host is None:
            PendingReadBack(self).finish()                  # ONE read-back (also of the skipped-row gradient counter)
        return self._host

    def scatter_add(self, src2d, dst2d):
        """dst2d [M, cols] rows += the compact rows src2d [Mc, cols]."""
        cols = src2d.shape[1]
        check(_L().gct_scatter_add_quads(_p(src2d), src2d.stride(0), _p(self.quad_list), self.Mc, cols, _p(dst2d),
                                         dst2d.stride(0), self.M, _st()), "gct_scatter_add_quads")
        return dst2d

    def check_grad(self, g2d):
        """The backward of a forward that ran on these rows only: count the gradient rows outside them that are not
        zero (device counter, read at the next host() of any LiveRows -- no synchronisation here)."""
        check(_L().gct_dead_rows_nonzero(_p(g2d), g2d.stride(0), self.M, g2d.shape[1], _p(self.live),
                                         _p(skipped_row_gradients()), _st()), "gct_dead_rows_nonzero")

    def empty(self, cols):
        """A compact [Mc, cols] activation (with SLACK rows of allocation behind it)."""
        return torch.empty(self.Mc + self.SLACK, cols, dtype=torch.float32, device=self.dev)[:self.Mc]

    def empty_zero_gaps(self, cols):
        """A compact [Mc, cols] buffer for a kernel that writes the rows cstart[b] .. + n_b[b] of every sample only
        (attention over compact rows): uninitialised, except that the rows in between -- padded rows that travel with a
        live quad, the padding quads at the end -- are zero, so that the GEMMs that consume all Mc rows see finite
        values there (a few rows per sample instead of a fill of the whole buffer)."""
        t = self.empty(cols)
        check(_L().gct_zero_gap_rows(_p(t), t.stride(0), cols, _p(self.cstart), _p(self.n_b), self.B, self.Mc, _st()),
              "gct_zero_gap_rows")
        return t

    def gather(self, src2d, out=None):
        """src2d [M, cols] (row stride >= cols) -> compact [Mc, cols]; padding rows are zero."""
        cols = src2d.shape[1]
        dst = self.empty(cols) if out is None else out
        check(_L().gct_gather_quads(_p(src2d), src2d.stride(0), src2d.shape[0], _p(self.quad_list), self.Mc, cols,
                                    _p(dst), dst.stride(0), _st()), "gct_gather_quads")
        return dst

    def scatter(self, src2d, out=None):
        """compact [Mc, cols] -> [M, cols], zero rows where nothing is live."""
        cols = src2d.shape[1]
        dst = torch.zeros(self.M, cols, dtype=torch.float32, device=self.dev) if out is None else out
        check(_L().gct_scatter_quads(_p(src2d), src2d.stride(0), _p(self.quad_list), self.Mc, cols, _p(dst),
                                     dst.stride(0), self.M, _st()), "gct_scatter_quads")
        return dst


HOST_BLOCKED_S = [0.0]      # host seconds spent waiting in PendingReadBack.finish (a training step's one synchronisation)


class PendingReadBack:
    """host() of several LiveRows / KeyRows with ONE device->host copy, in two halves: the constructor queues the
    asynchronous copy of the maps' info records (and of the skipped-row gradient counter) behind the kernels that wrote
    them and records an event; finish() waits for that event only -- not for whatever was queued on the stream
    afterwards -- and fills the host side in.  The trainer queues a batch's maps one step ahead
    (Model/forward_propagation1.prefetch), so finish() finds them done."""

    def __init__(self, *objs):
        seen, self.objs = set(), []
        for o in objs:
            if o is not None and o._host is None and id(o) not in seen:
                seen.add(id(o))
                self.objs.append(o)
        self.host = self.ev = None
        if self.objs:
            dev = torch.cat([o.info for o in self.objs] + [skipped_row_gradients()])
            self.host = torch.empty(dev.numel(), dtype=dev.dtype, pin_memory=True)
            self.host.copy_(dev, non_blocking=True)
            self.ev = torch.cuda.Event()
            self.ev.record()

    def finish(self):
        if self.host is None:
            return
        import time
        t0 = time.perf_counter()
        self.ev.synchronize()
        HOST_BLOCKED_S[0] += time.perf_counter() - t0
        v = self.host.tolist()
        self.host = None
        for i, o in enumerate(self.objs):
            if o._host is None:
                o._fill_host(v[8 * i:8 * i + 8])
        if v[-1] != 0:
            skipped_row_gradients().zero_()
            raise _lib.GctError(_SKIPPED_MSG.format(v[-1]))


class KeyRows(LiveRows):
    """The compaction map of the KEY side of cross-attention, from a key-padding mask [B, Lk] (gct_key_rows): the
    padded rows of the encoder memory are masked keys, so their K / V projections (and dK / dV) need not exist.
    Same interface as LiveRows (gather / scatter / empty / quad_list / cstart / n_b / Mc after host())."""

    def __init__(self, mask_u8, B, Lk):
        _chk(mask_u8, "key_rows.mask", torch.uint8)
        dev = mask_u8.device
        M = B * Lk
        nq = (M + 3) // 4
        i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)            # noqa: E731
        self.B, self.T, self.M, self.dev = B, Lk, M, dev
        self.live = torch.empty(max(M, 1), dtype=torch.uint8, device=dev)
        self.n_b, self.info = i32(B), i32(8)
        self.cstart, self.quad_list = i32(B), i32(nq + 32)
        qrank = i32(nq)
        check(_L().gct_key_rows(_p(mask_u8), Lk, B, Lk, _p(self.live), _p(self.n_b), _p(self.info), _p(self.cstart),
                                _p(self.quad_list), _p(qrank), _st()), "gct_key_rows")
        self._host = None
        self.Mc = None

    # (host(): LiveRows' -- the same 8-word info record, read together with whatever else is pending)


def linear_wgrad(dys: Sequence[torch.Tensor], lddy: int, x2d, dws: Sequence[torch.Tensor],
                 dbs: Sequence[Optional[torch.Tensor]], kt=None):
    M, K = x2d.shape
    nper = dws[0].shape[0]
    nseg = len(dws)
    d = _seg3(dys)
    dw = _seg3(dws)
    db = _seg3(dbs)

    def launch():
        ws = kept_workspace(_ws_need("gct_wgrad_ws_bytes", M, nseg * nper, K), x2d.device)
        with _Timed("gemm_wgrad+bias+reduce", 2.0 * M * K * nper * nseg):
            check(_L().gct_linear_wgrad(d[0], d[1], d[2], lddy, M, nseg, nper, _p(x2d), x2d.stride(0),
                                        K, dw[0], dw[1], dw[2], K, db[0], db[1], db[2], _p(ws),
                                        _p(kt[0]) if kt else None, _p(kt[1]) if kt else None, _st()),
                  "gct_linear_wgrad")

    if not SIDE_ENABLED or torch.cuda.is_current_stream_capturing():
        launch()
        return
    main = torch.cuda.current_stream()
    side = _side_stream(x2d.device)
    ready = torch.cuda.Event()
    ready.record(main)
    side.wait_event(ready)
    with torch.cuda.stream(side):
        launch()
        done = torch.cuda.Event()
        done.record(side)
    for t in list(dys) + [x2d]:
        t.record_stream(side)
        _PENDING[t.untyped_storage().data_ptr()] = done


# One Linear's backward as one call (gct_linear_bwd): where both problems take the 128 x 256 bf16 tile kernel the library
# runs them as ONE launch whose weight-gradient split is chosen for the shared grid (csrc/gemm.hip plan_bwd_pair).  Tests
# flip this attribute to run the same model both ways (and restore it); there is no environment knob.
PAIR_BWD = True


def linear_bwd_route(M, nseg, nper, K, lddy, ldx, ldw, lddx, depi=DEPI_STORE, aligned16=True, have_planes=True,
                     want_bias=True, mode=None, ws_bytes=None):
    """(paired, nsplit, rows per split, bias fused, wgrad blocks, dgrad blocks, modelled pair time, modelled time of the
    two separate calls) of gct_linear_bwd for a shape (gct_linear_bwd_route: no launch; times in dgrad K-tile times)."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    if ws_bytes is None:
        ws_bytes = _ws_need("gct_linear_bwd_ws_bytes", M, nseg * nper, K)
    check(_L().gct_linear_bwd_route(M, nseg, nper, K, lddy, ldx, ldw, lddx, int(depi), int(aligned16), int(have_planes),
                                    int(want_bias), gemm_get_mode() if mode is None else int(mode), int(ws_bytes),
                                    ctypes.addressof(out)), "gct_linear_bwd_route")
    v = [int(t) for t in out]
    return (v[0], v[1], v[2], v[3], v[4], v[5], v[6] / 1000.0, v[7] / 1000.0)


def linear_bwd(dys: Sequence[torch.Tensor], lddy: int, x2d, ws_: Sequence[torch.Tensor], dws: Sequence[torch.Tensor],
               dbs: Sequence[Optional[torch.Tensor]], dx, depi=DEPI_STORE, pre=None, p=0.0, seed=0, site=0, kt=None,
               live=None, pre_full=False, M=None, planes=None):
    """linear_wgrad(dys, lddy, x2d, dws, dbs, kt) and linear_dgrad(dys, lddy, M, ws_, dx, depi, ...) of the same dY."""
    M = x2d.shape[0] if M is None else M
    if not PAIR_BWD or SIDE_ENABLED or M != x2d.shape[0] or torch.cuda.is_current_stream_capturing():
        linear_wgrad(dys, lddy, x2d, dws, dbs, kt=kt)
        linear_dgrad(dys, lddy, M, ws_, dx, depi=depi, pre=pre, p=p, seed=seed, site=site, live=live, pre_full=pre_full,
                     planes=planes)
        return
    K = x2d.shape[1]
    nper, nseg = dws[0].shape[0], len(dws)
    d, dw, db, w = _seg3(dys), _seg3(dws), _seg3(dbs), _seg3(ws_)
    _wait_pending(dx)
    wneed = _ws_need("gct_linear_bwd_ws_bytes", M, nseg * nper, K)   # the size the plan is made for (linear_bwd_route's)
    wws = kept_workspace(wneed, x2d.device)
    need = _ws_need("gct_linear_dgrad_ws_bytes", M, nper * nseg, K)
    wsb = workspace(need, dx.device) if need > 256 else None
    wp, pstride = _plane_ptr(ws_) if planes is None else planes
    with _Timed("gemm_bwd", 4.0 * M * K * nper * nseg):
        check(_L().gct_linear_bwd(d[0], d[1], d[2], lddy, M, nseg, nper, _p(x2d), x2d.stride(0), K,
                                  dw[0], dw[1], dw[2], K, db[0], db[1], db[2], _p(wws), wneed,
                                  _p(kt[0]) if kt else None, _p(kt[1]) if kt else None,
                                  w[0], w[1], w[2], ws_[0].stride(0), wp, pstride,
                                  _p(dx), dx.stride(0), depi, _p(pre), p, seed, site,
                                  _p(wsb), 0 if wsb is None else wsb.numel() * 4,
                                  None if live is None else _p(live.quad_list),
                                  pre.shape[0] if (live is not None and pre is not None and pre_full) else 0, _st()),
              "gct_linear_bwd")


KV_FOLD_MAX_LAYERS = 16                        # GCT_KV_FOLD_MAX_LAYERS (include/gctplus_hip.h)


class KvFold:
    """Cross-attention K | V straight from the latent (gct_kv_fold_*): the decoder memory e = z W_z^T + b_z feeds
    nothing but the k_linear | v_linear projections of the decoder layers, so layer l's K | V are
    z A_l^T + c_l with A_l = W_kv,l W_z and c_l = W_kv,l b_z + b_kv,l.  One object per decoder forward: it holds A, c
    and the bf16 planes of A for all layers (written by ONE gct_kv_fold_fwd call) and, for the backward, the stacked
    weights and the buffers P_l = dkv_l^T z, s_l = colsum(dkv_l) that the layers' weight-gradient GEMMs fill.
    kv: [(k_linear, v_linear)] of the layers (nn.Linear, weights [d, dm]); fc_z: nn.Linear(lat -> dm)."""

    @staticmethod
    def usable(kv, fc_z):
        if not kv or len(kv) > KV_FOLD_MAX_LAYERS or fc_z.bias is None:
            return False
        d, dm = kv[0][0].weight.shape
        al16 = lambda t: t.data_ptr() % 16 == 0 and getattr(t, "_gct_gview", t).data_ptr() % 16 == 0     # noqa: E731
        return (d % 4 == 0 and dm % 4 == 0 and fc_z.weight.shape[1] % 4 == 0 and fc_z.weight.shape[0] == dm and
                fc_z.weight.is_contiguous() and al16(fc_z.weight) and al16(fc_z.bias) and
                all(m.weight.shape == (d, dm) and m.bias is not None and m.weight.is_contiguous() and al16(m.weight)
                    for pair in kv for m in pair))

    def __init__(self, kv, fc_z):
        import ctypes
        self.kv, self.fc_z = kv, fc_z
        wz, bz = fc_z.weight, fc_z.bias
        self.L, (self.d, self.dm), self.lat = len(kv), kv[0][0].weight.shape, wz.shape[1]
        L, d, dm, lat = self.L, self.d, self.dm, self.lat
        dev, R = wz.device, 2 * L * d
        _chk(wz, "kv_fold.fc_z.weight")
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)       # noqa: E731
        self.wstack, self.a, self.c = f32(R, dm), f32(R, lat), f32(R)
        self.p, self.s = f32(R, lat), f32(R)                                          # the backward's P_l and s_l
        self.a_planes = torch.empty(3, R * lat, dtype=torch.int16, device=dev)
        self.planes = (self.a_planes.data_ptr(), self.a_planes.stride(0))
        mods = [m for pair in kv for m in pair]
        wa = (ctypes.c_int64 * len(mods))(*[m.weight.data_ptr() for m in mods])
        ba = (ctypes.c_int64 * len(mods))(*[m.bias.data_ptr() for m in mods])
        need = int(_L().gct_kv_fold_ws_bytes(L, d, dm, lat))
        wsb = workspace(need, dev)
        wzp, wzs = _plane_ptr([wz])
        check(_L().gct_kv_fold_fwd(L, ctypes.addressof(wa), ctypes.addressof(ba), d, dm, _p(wz), wzp, wzs, _p(bz), lat,
                                   _p(self.wstack), _p(self.a), _p(self.c), _p(self.a_planes), self.a_planes.stride(0),
                                   _p(wsb), wsb.numel() * 4, _st()), "gct_kv_fold_fwd")

    def _rows(self, t, layer):
        d = self.d
        return [t[2 * layer * d:(2 * layer + 1) * d], t[(2 * layer + 1) * d:(2 * layer + 2) * d]]

    def layer_planes(self, layer):
        return (self.planes[0] + 2 * (2 * layer * self.d * self.lat), self.planes[1])

    def fwd(self, layer, zc, outs, ldy):
        """kvb_l = zc A_l^T + c_l into outs (k, v) of leading dimension ldy."""
        linear_fwd(zc, self._rows(self.a, layer), self._rows(self.c, layer), outs, ldy, planes=self.layer_planes(layer))

    def bwd(self, layer, dys, lddy, zc, dz, depi, M):
        """P_l, s_l from dkv_l (dys) and the rows zc; dz (nullable) = / += dkv_l A_l."""
        if dz is None:
            linear_wgrad(dys, lddy, zc, self._rows(self.p, layer), self._rows(self.s, layer))
        else:
            linear_bwd(dys, lddy, zc, self._rows(self.a, layer), self._rows(self.p, layer), self._rows(self.s, layer),
                       dz, depi=depi, M=M, planes=self.layer_planes(layer))

    def wgrad_layer(self, layer, dwk, dwv, dbk, dbv):
        """dW_kv,l = P_l W_z^T + s_l (x) b_z and db_kv,l = s_l, once the layer's slab reductions have run."""
        if SIDE_ENABLED:
            join_side()
        d = self.d
        check(_L().gct_kv_fold_wgrad(_p(self.p[2 * layer * d:]), _p(self.s[2 * layer * d:]), d, self.lat,
                                     _p(self.fc_z.weight), _p(self.fc_z.bias), self.dm, _p(dwk), _p(dwv), _p(dbk),
                                     _p(dbv), _st()), "gct_kv_fold_wgrad")

    def finish(self, dwz, dbz):
        """dW_z = sum_l W_kv,l^T P_l and db_z = sum_l W_kv,l^T s_l, after every layer's backward."""
        if SIDE_ENABLED:
            join_side()
        linear_wgrad([self.wstack], self.dm, self.p, [dwz], [None])
        need = int(_L().gct_kv_fold_ws_bytes(self.L, self.d, self.dm, self.lat))
        wsb = workspace(need, dwz.device)
        check(_L().gct_kv_fold_dbz(_p(self.wstack), _p(self.s), self.wstack.shape[0], self.dm, _p(dbz), _p(wsb),
                                   wsb.numel() * 4, _st()), "gct_kv_fold_dbz")


def dropout_bwd(dout2d, p, seed, site, out=None, live=None):
    rows, cols = dout2d.shape
    if live is not None:
        rows = live.Mc
    dy = torch.empty_like(dout2d) if out is None else out
    _wait_pending(out)
    check(_L().gct_dropout_bwd(_p(dout2d), _p(dy), rows, cols, p, seed, site,
                               None if live is None else _p(live.quad_list), _st()), "gct_dropout_bwd")
    return dy


# ------------------------------------------------------------------------------ attention
# GCT_ATTN_DIRECT_MAX_KEYS of include/gctplus_hip.h: up to this many keys the barrier-free kernels run (the backward
# then needs its workspace); the forward over compact query rows (`live`) exists only there
ATTN_DIRECT_MAX_KEYS = 96


class MaskBits:
    """An attention mask packed for the kernels (gct_attn_mask_pack): one bit per key, 8 words per query row.
    Built once per trunk call from the reference's bool / int64 mask and shared by every layer, head and the
    backward pass.  `u8` keeps the byte form (ops.LiveRows checks the decoder's zero-row shortcut against it)."""

    def __init__(self, mask_u8, B, Lq, Lk):
        _chk(mask_u8, "attn.mask", torch.uint8)
        if Lk > 256 or Lq > 256:
            raise _lib.GctError(f"attention: sequence length {max(Lq, Lk)} > 256 unsupported")
        sb, sq = _mask_strides(mask_u8, B, Lq, Lk)
        rows = 1 if sq == 0 else Lq
        self.u8, self.B, self.Lq, self.Lk = mask_u8, B, Lq, Lk
        self.bits = torch.empty(B, rows, 8, dtype=torch.int32, device=mask_u8.device)
        self.sb, self.sq = rows * 8, (0 if sq == 0 else 8)
        # visible key tiles per (batch, query tile): lets the kernels request K before the mask rows are back
        ntr = 1 if sq == 0 else (Lq + 15) // 16
        self.tiles = torch.empty(B, ntr, dtype=torch.int32, device=mask_u8.device)
        self.t_sb, self.t_su = ntr, (0 if sq == 0 else 1)
        check(_L().gct_attn_mask_pack(_p(mask_u8), sb, sq, B, Lq, Lk, _p(self.bits), _p(self.tiles), _st()),
              "gct_attn_mask_pack")


def pack_mask(mask, B, Lq, Lk) -> Optional["MaskBits"]:
    """None | MaskBits | uint8 / bool / int64 mask of [B,Lk], [B,1,Lk] or [B,Lq,Lk] elements -> MaskBits."""
    if mask is None or isinstance(mask, MaskBits):
        if isinstance(mask, MaskBits) and (mask.B, mask.Lk) != (B, Lk):
            raise _lib.GctError(f"packed mask was built for B={mask.B}, Lk={mask.Lk}, not B={B}, Lk={Lk}")
        return mask
    return MaskBits(to_mask_u8(mask), B, Lq, Lk)


def _mb(mask, B, Lq, Lk):
    """(pointer, batch stride, row stride, owner): the caller keeps `owner` referenced until its launch is enqueued --
    a mask packed on the fly lives only in that object, and a freed block may be handed to the next torch.empty."""
    mb = pack_mask(mask, B, Lq, Lk)
    if mb is None:
        return None, 0, 0, None
    if mb.t_su and mb.Lq != Lq:
        raise _lib.GctError(f"packed mask was built for Lq={mb.Lq}, not Lq={Lq}")
    return mb.bits.data_ptr(), mb.sb, mb.sq, mb


def _tb(mb):
    """(tile words, batch stride, query-tile stride) of a packed mask."""
    return (None, 0, 0) if mb is None else (mb.tiles.data_ptr(), mb.t_sb, mb.t_su)


def attn_fwd(q, k, v, ld_q, ld_k, ld_v, mask, B, H, Lq, Lk, dk, p, seed, site, out=None,
             want_probs=False, keys=None, live=None):
    """q/k/v: tensors whose data_ptr is element (b=0,l=0,h=0,0) with row strides ld_*.
    mask: None | MaskBits | uint8 [B,Lk] / [B,1,Lk] (key padding) / [B,Lq,Lk] (packed on the fly).
    live (LiveRows): q and the output hold the compact query rows only; keys (LiveRows / KeyRows): so do k / v."""
    dev = q.device
    if out is not None:
        o = out
    elif live is not None:     # rows of a live quad outside every sample's live prefix are not written: keep them finite
        o = live.empty_zero_gaps(H * dk)
    else:
        o = torch.empty(B * Lq, H * dk, dtype=torch.float32, device=dev)
    lse = torch.empty(B * H * Lq, dtype=torch.float32, device=dev)
    probs = torch.empty(B, H, Lq, Lk, dtype=torch.float32, device=dev) if want_probs else None
    mp, sb, sq, mask_owner = _mb(mask, B, Lq, Lk)
    check(_L().gct_attn_fwd(_p(q), ld_q, _p(k), ld_k, _p(v), ld_v, mp, sb, sq, _p(o),
                            o.stride(0), _p(lse), _p(probs), B, H, Lq, Lk, dk,
                            1.0 / math.sqrt(dk), p, seed, site, None if keys is None else _p(keys.cstart),
                            None if keys is None else _p(keys.n_b), *_tb(mask_owner),
                            None if live is None else _p(live.cstart), None if live is None else _p(live.n_b),
                            _st()), "gct_attn_fwd")
    del mask_owner
    return o, lse, probs


_ATTN_BWD_WS = {}


def _attn_bwd_ws(dev, nbytes):
    """Scratch of the two-launch attention backward: one buffer per (device, stream) like `workspace`, grown on demand
    (launches on one stream are ordered, so consecutive calls may share it; two streams never share one)."""
    if nbytes <= 0:
        return None
    key = (dev, _st())
    ws = _ATTN_BWD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ATTN_BWD_WS[key] = ws
    return ws


def attn_bwd(q, k, v, ld_q, ld_k, ld_v, mask, o, dout, lse, dq, dk_, dv, ld_dq, ld_dk, ld_dv,
             B, H, Lq, Lk, dk, p, seed, site, live=None, kv_compact=False, keys=None):
    """live (LiveRows): dout / dq are quad-compacted; kv_compact: so are dk / dv (self-attention); keys (KeyRows):
    k / v / dk / dv hold the visible keys only (cross-attention).  live.fwd: the forward ran on the compact rows, so
    q and o are compact as well (and, for self-attention, k / v: pass keys=live, kv_compact=False)."""
    ws = _attn_bwd_ws(q.device, int(_L().gct_attn_bwd_ws_bytes(B, H, Lq, Lk)))
    mp, sb, sq, mask_owner = _mb(mask, B, Lq, Lk)
    check(_L().gct_attn_bwd(_p(q), ld_q, _p(k), ld_k, _p(v), ld_v, mp, sb, sq, _p(o),
                            _p(dout), o.stride(0), _p(lse), _p(dq), ld_dq, _p(dk_), ld_dk,
                            _p(dv), ld_dv, B, H, Lq, Lk, dk, 1.0 / math.sqrt(dk), p, seed, site,
                            None if live is None else _p(live.cstart), None if live is None else _p(live.n_b),
                            int(bool(kv_compact)) | (2 if (live is not None and live.fwd) else 0),
                            None if keys is None else _p(keys.cstart),
                            None if keys is None else _p(keys.n_b), *_tb(mask_owner), _p(ws),
                            0 if ws is None else ws.numel(),
                            _st()), "gct_attn_bwd")
    del mask_owner


def _mask_strides(mask_u8, B, Lq, Lk):
    if mask_u8 is None:
        return 0, 0
    _chk(mask_u8, "attn.mask", torch.uint8)
    n = mask_u8.numel()
    if n == B * Lk:
        return Lk, 0
    if n == B * Lq * Lk:
        return Lq * Lk, Lk
    raise _lib.GctError(f"attention mask with {n} elements fits neither [B,Lk] nor [B,Lq,Lk] "
                        f"(B={B}, Lq={Lq}, Lk={Lk})")


def trg_mask_u8(target: torch.Tensor, pad_id: int) -> torch.Tensor:
    """uint8 [B,T,T] form of Model.modules.get_trg_mask(target, pad_id, use_cond2dec=False) built from the token ids in
    one launch (reference Model/modules.py:47-58 builds an int64 [B,T,T] tensor: 27 MB at B = 512).  Nonzero = the
    query may attend, exactly where the reference's mask is nonzero (including its `* pad_idx` quirk)."""
    _chk(target, "trg_mask.target", torch.int64)
    B, T = target.shape
    out = torch.empty(B, T, T, dtype=torch.uint8, device=target.device)
    check(_L().gct_trg_mask_tokens(_p(target), target.stride(0), int(pad_id), B, T, _p(out), _st()),
          "gct_trg_mask_tokens")
    return out


def to_mask_u8(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """Reference masks are bool [B,1,Lk] (Model/modules.py:38-44) or int64 [B,T,T]
    (modules.py:47-58); the kernels take uint8 (0 = masked)."""
    if mask is None:
        return None
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).to(torch.uint8).contiguous()


# -------------------------------------------------------------------------------- VAE / loss
def reparam_fwd(mu, log_var, eps, seed, site):
    z = torch.empty_like(mu)
    eps_out = torch.empty_like(mu)
    check(_L().gct_reparam_fwd(_p(mu), _p(log_var), _p(eps), _p(eps_out), _p(z), mu.numel(), seed,
                               site, _st()), "gct_reparam_fwd")
    return z, eps_out


def reparam_bwd(dz, log_var, eps, dmu_ext, dlv_ext, dmu, dlv):
    check(_L().gct_reparam_bwd(_p(dz), _p(log_var), _p(eps), _p(dmu_ext), _p(dlv_ext), _p(dmu),
                               _p(dlv), dz.numel(), _st()), "gct_reparam_bwd")


def kld_fwd(mu, log_var):
    out = torch.empty((), dtype=torch.float32, device=mu.device)
    ws = workspace(4096, mu.device)
    check(_L().gct_kld_fwd(_p(mu), _p(log_var), _p(out), _p(ws), mu.numel(), _st()), "gct_kld_fwd")
    return out


def kld_bwd(mu, log_var, gout):
    dmu, dlv = torch.empty_like(mu), torch.empty_like(log_var)
    check(_L().gct_kld_bwd(_p(mu), _p(log_var), _p(gout), _p(dmu), _p(dlv), mu.numel(), _st()),
          "gct_kld_bwd")
    return dmu, dlv


LATENT_MAX_DIM = 1024                          # GCT_LATENT_MAX_DIM (include/gctplus_hip.h)


def _kl_rows(what, mu, log_var, live):
    """(mu, log_var, live u8 [R] or None, R, D) of the per-dimension KL calls, checked before a launch."""
    _chk(mu, f"{what}.mu"), _chk(log_var, f"{what}.log_var")
    if mu.dim() < 1 or mu.shape != log_var.shape:
        raise _lib.GctError(f"{what}: mu {tuple(mu.shape)} and log_var {tuple(log_var.shape)} must have one shape [..., D]")
    if not (mu.is_contiguous() and log_var.is_contiguous()):
        raise _lib.GctError(f"{what}: mu and log_var must be contiguous")
    D = mu.shape[-1]
    if D % 4 or not 4 <= D <= LATENT_MAX_DIM:
        raise _lib.GctError(f"{what}: latent width {D} must be a multiple of 4 in [4, {LATENT_MAX_DIM}]")
    R = mu.numel() // D
    if live is not None:
        if live.dtype not in (torch.bool, torch.uint8) or live.device != mu.device:
            raise _lib.GctError(f"{what}: live must be a bool or uint8 tensor on mu's device")
        shapes = [(R,)]
        if mu.dim() == 3:
            shapes += [tuple(mu.shape[:2]), (mu.shape[0], 1, mu.shape[1])]
        if tuple(live.shape) not in shapes:
            raise _lib.GctError(f"{what}: live {tuple(live.shape)} fits none of {shapes}")
        live = to_mask_u8(live).view(-1)
    return mu, log_var, live, R, D


def _kld_dims_ws(D, device):
    return workspace(_L().gct_kld_dims_ws_bytes(D), device)


def kld_dims_fwd(mu, log_var, live=None, free_bits=0.0, n_mol=1):
    """Per-dimension KL with free bits over the live rows (include/gctplus_hip.h: gct_kld_dims_fwd;
    engine.kl_dims_reference).  mu, log_var fp32 [..., D]; live bool/u8 [B, Le], [B, 1, Le] or [R] (None: every row).
    Returns (out fp32 [4] = objective, raw, n_floor, live rows; kl_dim fp32 [D]; gate fp32 [D]); nothing is read back."""
    mu, log_var, live, R, D = _kl_rows("kld_dims_fwd", mu, log_var, live)
    free_bits, n_mol = float(free_bits), int(n_mol)
    if not (math.isfinite(free_bits) and free_bits >= 0.0 and abs(free_bits) <= 3.4028234663852886e38):
        raise _lib.GctError(f"kld_dims_fwd: free_bits {free_bits!r} must be a finite number >= 0")
    if not 1 <= n_mol < 2 ** 31:
        raise _lib.GctError(f"kld_dims_fwd: n_mol {n_mol} must be >= 1")
    out = torch.empty(4, dtype=torch.float32, device=mu.device)
    kl_dim = torch.empty(D, dtype=torch.float32, device=mu.device)
    gate = torch.empty(D, dtype=torch.float32, device=mu.device)
    check(_L().gct_kld_dims_fwd(_p(mu), _p(log_var), _p(live), R, D, free_bits, n_mol, _p(out), _p(kl_dim), _p(gate),
                                _p(_kld_dims_ws(D, mu.device)), _st()), "gct_kld_dims_fwd")
    return out, kl_dim, gate


def kld_dims_bwd(mu, log_var, live, gate, gout):
    """(dmu, dlv) of kld_dims_fwd's objective times the device scalar gout: kld_bwd's bits where gate[j] != 0 and the
    row is live, exact +0.0 elsewhere.  gate: the fp32 [D] the forward wrote."""
    mu, log_var, live, R, D = _kl_rows("kld_dims_bwd", mu, log_var, live)
    _chk(gate, "kld_dims_bwd.gate"), _chk(gout, "kld_dims_bwd.gout")
    if tuple(gate.shape) != (D,) or not gate.is_contiguous() or gout.numel() != 1:
        raise _lib.GctError(f"kld_dims_bwd: gate must be fp32 [{D}] and gout one fp32 scalar")
    dmu, dlv = torch.empty_like(mu), torch.empty_like(log_var)
    check(_L().gct_kld_dims_bwd(_p(mu), _p(log_var), _p(live), _p(gate), _p(gout), _p(dmu), _p(dlv), R, D, _st()),
          "gct_kld_dims_bwd")
    return dmu, dlv


def latent_moments_state(D, device):
    """A zeroed running state of latent_moments: fp64 [6, D] (rows: include/gctplus_hip.h, gct_latent_moments)."""
    return torch.zeros(6, int(D), dtype=torch.float64, device=device)


def latent_moments(mu, log_var, live, acc):
    """Adds one batch's live rows into acc (latent_moments_state): per dimension the sums of mu, mu^2, exp(log_var),
    log_var and the KL term, and the live-row count.  Two launches; nothing is returned and nothing is read back."""
    mu, log_var, live, R, D = _kl_rows("latent_moments", mu, log_var, live)
    if acc.dtype != torch.float64 or tuple(acc.shape) != (6, D) or acc.device != mu.device or not acc.is_contiguous():
        raise _lib.GctError(f"latent_moments: acc must come from latent_moments_state({D}, mu.device)")
    check(_L().gct_latent_moments(_p(mu), _p(log_var), _p(live), R, D, _p(acc), _p(_kld_dims_ws(D, mu.device)), _st()),
          "gct_latent_moments")


def _host_i32(x, name, count=None):
    """A per-row table the caller holds on the HOST (list, numpy array or CPU tensor) as a contiguous int32 CPU tensor:
    its range checks are done here, before a launch, because the library never reads device memory."""
    t = torch.as_tensor(x)
    if t.numel() == 0:
        t = t.to(torch.int64)
    if t.is_cuda or t.is_floating_point() or t.dim() != 1 or (count is not None and t.numel() != count):
        raise ValueError(f"{name}: expected {'' if count is None else str(count) + ' '}integers on the host, one per row")
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise _lib.GctError(f"{name}: does not fit int32")
    return t.to(torch.int32).contiguous()


def latent_stats(mu, log_var, rows):
    """gct_latent_stats: mu, log_var fp32 [n, Le, D] contiguous on the device, rows [n] host integers (molecule i owns
    its first rows[i] latent rows, 1 <= rows[i] <= Le; later rows are never read) -> stats fp32 [n, 4, D]: mean and
    unbiased standard deviation of mu, then of log_var, per dimension (0 where rows[i] == 1)."""
    _chk(mu, "latent_stats.mu"), _chk(log_var, "latent_stats.log_var")
    if mu.dim() != 3 or log_var.shape != mu.shape or not mu.is_contiguous() or not log_var.is_contiguous():
        raise ValueError("latent_stats: mu and log_var must be contiguous [n, Le, D] tensors of one shape")
    n, Le, D = mu.shape
    rows = _host_i32(rows, "latent_stats.rows", n)
    if n and (int(rows.min()) < 1 or int(rows.max()) > Le):
        raise _lib.GctError(f"latent_stats: rows must lie in [1, {Le}], got {int(rows.min())}..{int(rows.max())}")
    stats = torch.empty(n, 4, D, dtype=torch.float32, device=mu.device)
    rows_dev = rows.to(mu.device)                   # held until the launch is enqueued
    check(_L().gct_latent_stats(_p(mu), _p(log_var), n, Le, D, _p(rows_dev), _p(stats), _st()), "gct_latent_stats")
    return stats


def latent_interp(stats, a, b, alpha, noise_std, lens, items, T, seed):
    """gct_latent_interp: stats fp32 [n, 4, D] on the device (latent_stats); a, b, lens, items [R] host integers and
    alpha, noise_std [R] host floats, one per output row -> z fp32 [R, T, D]: row r interpolates molecule a[r] towards
    b[r] over its first lens[r] tokens (zeros behind them) with the random streams of items[r].  The per-row tables
    travel to the device as one copy.  GctError before any launch when lens is outside [0, T], a or b outside [0, n),
    or an item negative."""
    _chk(stats, "latent_interp.stats")
    if stats.dim() != 3 or stats.shape[1] != 4 or not stats.is_contiguous():
        raise ValueError("latent_interp: stats must be a contiguous [n, 4, D] tensor")
    n, D, T = stats.shape[0], stats.shape[2], int(T)
    a = _host_i32(a, "latent_interp.a")
    R = a.numel()
    b, lens, items = (_host_i32(t, f"latent_interp.{k}", R) for k, t in (("b", b), ("lens", lens), ("items", items)))
    fl = [torch.as_tensor(t, dtype=torch.float32).reshape(-1).contiguous() for t in (alpha, noise_std)]
    if any(t.numel() != R or t.is_cuda for t in fl):
        raise ValueError(f"latent_interp: alpha and noise_std take {R} host floats, one per row")
    if R:
        if int(lens.min()) < 0 or int(lens.max()) > T:
            raise _lib.GctError(f"latent_interp: lens must lie in [0, T = {T}], got {int(lens.min())}..{int(lens.max())}")
        if min(int(a.min()), int(b.min())) < 0 or max(int(a.max()), int(b.max())) >= n:
            raise _lib.GctError(f"latent_interp: a and b must lie in [0, n = {n})")
        if int(items.min()) < 0:
            raise _lib.GctError("latent_interp: items must be >= 0")
    tab = torch.stack([a, b, lens, items, fl[0].view(torch.int32), fl[1].view(torch.int32)]).to(stats.device)
    z = torch.empty(R, max(T, 0), D, dtype=torch.float32, device=stats.device)
    check(_L().gct_latent_interp(_p(stats), n, D, _p(tab[0]), _p(tab[1]), _p(tab[4]), _p(tab[5]), _p(tab[2]),
                                 _p(tab[3]), R, T, _p(z), int(seed), _st()), "gct_latent_interp")
    return z


def latent_iw(mu, log_var, rows, items, k0, Kc, seed, want_eps=False):
    """gct_latent_iw: mu, log_var fp32 [n, Le, D] contiguous on the device; rows, items [n] host integers (molecule i
    owns its first rows[i] latent rows and draws from the streams of items[i]) -> (z fp32 [n * Kc, Le, D], logw fp32
    [n * Kc], eps or None): the draws k0 .. k0 + Kc - 1 of q(z | x) for every molecule, output row i * Kc + (k - k0),
    with logw = log p(z) - log q(z | x) of the row; zeros behind a molecule's rows.  want_eps: also the N(0, 1) draws
    themselves (the tests' handle; z and logw do not depend on it).  ValueError / GctError before any launch for
    malformed tensors, rows outside [1, Le], a negative item, and whatever the library's limits refuse."""
    _chk(mu, "latent_iw.mu"), _chk(log_var, "latent_iw.log_var")
    if mu.dim() != 3 or log_var.shape != mu.shape or not mu.is_contiguous() or not log_var.is_contiguous():
        raise ValueError("latent_iw: mu and log_var must be contiguous [n, Le, D] tensors of one shape")
    n, Le, D = mu.shape
    k0, Kc = int(k0), int(Kc)
    rows = _host_i32(rows, "latent_iw.rows", n)
    items = _host_i32(items, "latent_iw.items", n)
    if n and (int(rows.min()) < 1 or int(rows.max()) > Le):
        raise _lib.GctError(f"latent_iw: rows must lie in [1, {Le}], got {int(rows.min())}..{int(rows.max())}")
    if n and int(items.min()) < 0:
        raise _lib.GctError("latent_iw: items must be >= 0")
    if not (1 <= D <= LATENT_MAX_DIM and Le >= 1 and k0 >= 0 and Kc >= 0):
        # the library's own refusals, raised here before any output is allocated with a size it would not accept
        raise _lib.GctError(f"latent_iw: D={D} outside [1, {LATENT_MAX_DIM}], Le={Le} < 1 or a bad draw range "
                            f"k0={k0}, Kc={Kc}")
    tab = torch.stack([rows, items]).to(mu.device)      # one copy; held until the launch is enqueued
    R = n * Kc
    z = torch.empty(R, Le, D, dtype=torch.float32, device=mu.device)
    logw = torch.empty(R, dtype=torch.float32, device=mu.device)
    eps = torch.empty_like(z) if want_eps else None
    check(_L().gct_latent_iw(_p(mu), _p(log_var), n, Le, D, _p(tab[0]), _p(tab[1]), k0, Kc, _p(z), _p(logw), _p(eps),
                             int(seed), _st()), "gct_latent_iw")
    return z, logw, eps


def iw_combine(logp, logw, n, K):
    """gct_iw_combine: logp, logw fp32 [n * K] contiguous on the device (row i * K + k: the decoder's log p(x | z_k)
    and latent_iw's log p(z_k) - log q(z_k | x)) -> (iwae, elbo, recon, ess) fp32 [n]: the importance-weighted bound
    logsumexp_k(logp + logw) - log K, the mean log-weight, the mean logp and the effective sample size, in fp64 with one
    rounding.  ValueError before any launch for K < 1 or tensors that are not [n * K]."""
    _chk(logp, "iw_combine.logp"), _chk(logw, "iw_combine.logw")
    n, K = int(n), int(K)
    if n < 0 or K < 1:
        raise ValueError(f"iw_combine: n must be >= 0 and K >= 1, got n={n}, K={K}")
    for name, t in (("logp", logp), ("logw", logw)):
        if t.dim() != 1 or t.numel() != n * K or not t.is_contiguous():
            raise ValueError(f"iw_combine: {name} must be a contiguous [{n * K}] tensor, got {list(t.shape)}")
    out = torch.empty(4, n, dtype=torch.float32, device=logp.device)
    check(_L().gct_iw_combine(_p(logp), _p(logw), n, K, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _st()),
          "gct_iw_combine")
    return out[0], out[1], out[2], out[3]


def ce_fwd(logits2d, target, pad_id):
    _chk(target, "ce.target", torch.int64)
    rows, V = logits2d.shape
    out = torch.empty((), dtype=torch.float32, device=logits2d.device)
    ws = workspace(4096, logits2d.device)
    check(_L().gct_ce_fwd(_p(logits2d), _p(target), _p(out), _p(ws), rows, V, pad_id, _st()),
          "gct_ce_fwd")
    return out


def ce_bwd(logits2d, target, gout, pad_id):
    rows, V = logits2d.shape
    dl = torch.empty_like(logits2d)
    check(_L().gct_ce_bwd(_p(logits2d), _p(target), _p(gout), _p(dl), rows, V, pad_id, _st()),
          "gct_ce_bwd")
    return dl


# ------------------------------------------------------------------------------- optimiser
def adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, guard=True, clip_state=None):
    """guard: the update is skipped ON THE DEVICE when a gradient has landed on a decoder row that the forward skipped
    (skipped_row_gradients() != 0): the wrong gradient is never applied, and the next read-back raises.
    clip_state: a state written by grad_norm (with the same gscale): the step consumes (g * gscale) * coef and is
    skipped on the device when the norm was not finite.  None: the unclipped kernel, as ever."""
    if clip_state is not None:
        _chk_clip_state(clip_state, p.device)
    check(_L().gct_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, b1, b2, eps, step, gscale,
                             _p(skipped_row_gradients()) if guard else None, _p(clip_state), _st()), "gct_adam_step")


GRAD_NORM_MAX_GRID = 2048          # workgroups of 256 lanes, each lane 4 float4 per trip (csrc/adam.hip's header)
CLIP_STATE_WORDS = 8               # norm, coef, nonfinite, steps, clipped_steps, nonfinite_steps, largest norm, reserved


def _chk_clip_state(state, device):
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.float32 or state.numel() != CLIP_STATE_WORDS
            or not state.is_contiguous() or state.device != device):
        raise ValueError(f"clip state: {CLIP_STATE_WORDS} contiguous float32 words on {device} (new_clip_state)")


def new_clip_state(device):
    """A zeroed clipping state (include/gctplus_hip.h: gct_grad_norm); view words 2-5 as int32 to read the counters."""
    return torch.zeros(CLIP_STATE_WORDS, dtype=torch.float32, device=device)


def grad_norm_ws(n, device):
    """The slab of fp64 partials gct_grad_norm needs for n elements (the caller's, reusable for any smaller n)."""
    return torch.empty(_L().gct_grad_norm_ws_bytes(int(n)) // 8, dtype=torch.float64, device=device)


def grad_norm(g, state, ws, max_norm, gscale=1.0):
    """state <- norm = |gscale| * ||g||_2, coef = min(1, max_norm / (norm + 1e-6)) and the running counters, on the
    device, in two launches; g (flat fp32) is only read.  ws: grad_norm_ws(g.numel(), ...).  Nothing is returned and
    nothing is read by the host."""
    _chk(g, "grad_norm.g", torch.float32)
    if not g.is_contiguous():
        raise ValueError("grad_norm: g must be contiguous (one flat buffer)")
    _chk_clip_state(state, g.device)
    if ws.dtype != torch.float64 or ws.device != g.device or ws.numel() * 8 < _L().gct_grad_norm_ws_bytes(g.numel()):
        raise ValueError("grad_norm: ws must come from grad_norm_ws(n >= g.numel(), g.device)")
    check(_L().gct_grad_norm(_p(g), g.numel(), float(gscale), float(max_norm), _p(state), _p(ws), _st()),
          "gct_grad_norm")


# ---------------------------------------------------------------------------------- utility
def copy_rows(src, src_rpb, src_off, dst, dst_rpb, dst_off, rows, rpb, cols, accumulate=False):
    check(_L().gct_copy_rows(_p(src), src_rpb, src_off, _p(dst), dst_rpb, dst_off, rows, rpb, cols,
                             int(accumulate), _st()), "gct_copy_rows")


def small_linear_fwd(x, w, b):
    rows, K = x.shape
    N = w.shape[0]
    y = torch.empty(rows, N, dtype=torch.float32, device=x.device)
    check(_L().gct_small_linear_fwd(_p(x), _p(w), _p(b), _p(y), rows, K, N, _st()),
          "gct_small_linear_fwd")
    return y


def small_linear_bwd(dy, x, dw, db):
    rows, K = x.shape
    N = dw.shape[0]
    check(_L().gct_small_linear_bwd(_p(dy), _p(x), _p(dw), _p(db), rows, K, N, _st()),
          "gct_small_linear_bwd")


def add(a, b, out=None):
    y = torch.empty_like(a) if out is None else out
    check(_L().gct_add(_p(a), _p(b), _p(y), a.numel(), _st()), "gct_add")
    return y


# ----------------------------------------------------------------------------------- decode
def _check_row_off(row_off, n):
    if row_off is not None and (row_off.dtype != torch.int32 or row_off.numel() < n or not row_off.is_contiguous()):
        raise ValueError("row_off must be a contiguous int32 tensor with one offset per row")


def _check_step_rows(n, row_off, item, **tables):
    """Rows of a decode step (csrc/decode_rows.h): row_off alone (mixed), or with item and its per-item tables (stream)."""
    _check_row_off(row_off, n)
    names = ["item", *tables]
    if len({t is None for t in (item, *tables.values())}) != 1:
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} go together")
    if item is not None:
        _check_row_off(item, n)
        if row_off is None or any(t.dtype != torch.int32 or not t.is_contiguous() for t in tables.values()):
            raise ValueError(f"streamed rows need row_off and {'a ' if len(tables) == 1 else ''}contiguous int32 "
                             f"{' / '.join(tables)}")


def attn_decode(q, ldq, k, v, kv_row, kv_batch, valid_u8, valid_sb, out, n, H, Lc, dk, pos=None, cache_off=0,
                knew=None, vnew=None, ldn=0, klen=None, row_off=None):
    """klen (int32 [n], optional, fixed caches only): leading keys to look at per sample (the rest are masked).
    row_off (int32 [n], optional, with pos only): row b sits at position *pos - row_off[b] (mixed prefix lengths)."""
    _check_row_off(row_off, n)
    check(_L().gct_attn_decode(_p(q), ldq, _p(k), _p(v), kv_row, kv_batch, _p(valid_u8), valid_sb,
                               _p(out), out.stride(0), n, H, Lc, dk, 1.0 / math.sqrt(dk), _p(pos), cache_off,
                               _p(knew), _p(vnew), ldn, _p(klen), _p(row_off), _st()), "gct_attn_decode")


def attn_decode_z(q, qoff, z, ckv, nc, valid_u8, out, ooff, n, H, dk, klen=None):
    """Cross-attention of one decode step over the latent rows z [n, Le, lat] (gct_attn_decode_z): q [n, ldq] holds the
    plain query in columns [0, H*dk) (read only with condition rows) and the G^T-folded query at qoff; ckv [n*nc, >= 2*H*dk]
    the shifted keys | values of the nc condition rows; out [n, ldo] gets the per-head latent context at ooff (and the
    condition rows' part in columns [0, H*dk) when nc > 0)."""
    Le, lat = z.shape[1], z.shape[2]
    check(_L().gct_attn_decode_z(_p(q), q.stride(0), qoff, _p(z), z.stride(0), lat, Le, _p(ckv),
                                 0 if ckv is None else nc * ckv.stride(0), 0 if ckv is None else ckv.stride(0), nc,
                                 _p(valid_u8), 0 if valid_u8 is None else valid_u8.stride(0), _p(klen), _p(out),
                                 out.stride(0), ooff, n, H, dk, 1.0 / math.sqrt(dk), _st()), "gct_attn_decode_z")


SAMPLE_FILTER_MAX_VOCAB = 1024                  # GCT_SAMPLE_FILTER_MAX_VOCAB (include/gctplus_hip.h)


def sample_filter_settings(top_k, top_p, temperature, vocab):
    """The GctSampleFilter of validated settings (decode.check_sample_filter) as an int32 CPU tensor [4]:
    {k, top_p, 1/T, 0}, the two floats stored bit for bit (copy it to a device tensor for select_token's filt_dev)."""
    t = torch.zeros(4, dtype=torch.int32)
    t[0] = vocab if top_k is None else int(top_k)
    f = t.view(torch.float32)
    f[1] = 1.0 if top_p is None else float(top_p)
    f[2] = 1.0 / float(temperature)
    return t


def select_token(logits2d, ys, pos, valid_u8, done_u8, mode, pad_id, eos_id, seed=0, probs_out=None, pos_dev=None,
                 valid_off=0, seed_dev=None, row_off=None, filt_dev=None, item=None, prefix_len=None, item_base=0):
    """row_off (int32 [n], optional, with pos_dev only): row r writes at *pos_dev - row_off[r] + 1.
    filt_dev (int32 [4] on the device, optional, mode 1 only): top-k / nucleus / temperature settings
    (sample_filter_settings), read by the kernel; V <= SAMPLE_FILTER_MAX_VOCAB.
    item (int32 [n]) + prefix_len (int32 [items]), with row_off: continuous batching -- row r decodes pool item item[r]
    (< 0: parked, nothing written), keeps the prefix tokens the refill laid out, and draws with the key
    (item_base + item, pos)."""
    n, V = logits2d.shape
    _check_step_rows(n, row_off, item, prefix_len=prefix_len)
    if filt_dev is not None and (filt_dev.dtype != torch.int32 or filt_dev.numel() != 4 or not filt_dev.is_contiguous()):
        raise ValueError("filt_dev must be a contiguous int32 tensor of 4 entries (sample_filter_settings)")
    check(_L().gct_select_token(_p(logits2d), V, _p(ys), ys.stride(0), pos, _p(valid_u8),
                                valid_u8.stride(0) if valid_u8 is not None else 0, _p(done_u8),
                                _p(probs_out), n, mode, pad_id, eos_id, seed, _p(pos_dev), valid_off, _p(seed_dev),
                                _p(row_off), _p(filt_dev), _p(item), _p(prefix_len), item_base, _st()), "gct_select_token")


# token classes of the grammar table, class | ring number << 8 (GCT_GRAMMAR_* of include/gctplus_hip.h)
(GRAMMAR_ATOM, GRAMMAR_BOND, GRAMMAR_OPEN, GRAMMAR_CLOSE, GRAMMAR_RING, GRAMMAR_DOT, GRAMMAR_EOS, GRAMMAR_PAD,
 GRAMMAR_BANNED) = range(9)
GRAMMAR_MAX_RINGS = 64


def grammar_mask(logits2d, masked, table, ys, pos_dev, width=None, row_off=None, gram=None, item=None, prefix_len=None,
                 limit=None, kv_src=None, valid_off=0):
    """gct_grammar_mask, in front of select_token on the same device counter: masked [n, V] = logits2d where the grammar
    (smiles.SmilesGrammar; table int32 [V]) and the length budget allow the token as the next one of the row, -inf
    elsewhere.  gram int32 [2] on the device = (budget G, prefix width t0_max), row r's prefix being t0_max - row_off[r]
    tokens; or item / prefix_len / limit as in select_token and the stream's state.  width: token columns of ys in use
    (default all).  Parked rows and rows inside their prefix are not written.
    kv_src (int32 [n, >= valid_off + width], uniform rows only) + valid_off: gct_grammar_mask_anc -- the row's history
    is read through the ancestry map, token j from row kv_src[r, valid_off + j] (in front of smc_select)."""
    n, V = logits2d.shape
    _chk(logits2d, "grammar_mask.logits"), _chk(masked, "grammar_mask.masked"), _chk(ys, "grammar_mask.ys", torch.int64)
    _chk(table, "grammar_mask.table", torch.int32), _chk(pos_dev, "grammar_mask.pos", torch.int32)
    if not logits2d.is_contiguous() or not masked.is_contiguous() or masked.shape != logits2d.shape:
        raise ValueError("grammar_mask: logits and masked must be contiguous [n, V] buffers of one shape")
    if table.numel() != V or not table.is_contiguous() or ys.dim() != 2 or ys.shape[0] < n or ys.stride(1) != 1:
        raise ValueError("grammar_mask: table int32 [V], ys [n, T] with unit column stride")
    _check_step_rows(n, row_off, item, prefix_len=prefix_len, limit=limit)
    if item is None and (gram is None or gram.dtype != torch.int32 or gram.numel() != 2 or
                         not gram.is_contiguous()):
        raise ValueError("gram must be a contiguous int32 tensor (budget, prefix width)")
    T = ys.shape[1] if width is None else int(width)
    if kv_src is not None:
        if row_off is not None or item is not None:
            raise ValueError("grammar_mask: rows behind an ancestry map are uniform rows (no row_off, no items)")
        if (kv_src.dtype != torch.int32 or kv_src.dim() != 2 or kv_src.shape[0] < n or kv_src.stride(1) != 1 or
                kv_src.shape[1] < int(valid_off) + T or int(valid_off) < 0):
            raise ValueError("grammar_mask: kv_src int32 [n, >= valid_off + width] with unit column stride")
        check(_L().gct_grammar_mask_anc(_p(logits2d), _p(masked), V, _p(table), _p(ys), ys.stride(0), T, n, _p(pos_dev),
                                        _p(gram), _p(kv_src), kv_src.stride(0), int(valid_off), _st()),
              "gct_grammar_mask_anc")
        return
    check(_L().gct_grammar_mask(_p(logits2d), _p(masked), V, _p(table), _p(ys), ys.stride(0),
                                ys.shape[1] if width is None else int(width), n, _p(pos_dev), _p(row_off), _p(gram),
                                _p(item), _p(prefix_len), _p(limit), _st()), "gct_grammar_mask")


# status codes of the chemistry check (GCT_CHEM_* of include/gctplus_hip.h), and its per-token word:
# cap (bits 0..3, CHEM_NO_CAP: none) | H count << 4 | aromatic << 8 | carbon-like << 9 | bond order << 12
CHEM_OK, CHEM_SYNTAX, CHEM_VALENCE, CHEM_RING_BOND, CHEM_AROMATIC = range(5)
CHEM_NO_CAP = 15
SMILES_MAX_SPAN = 256                               # columns of a row's span that every SMILES kernel stages
CHEM_MAX_SPAN = SMILES_MAX_SPAN


def _smiles_rows(name, ys, **vectors):
    """The checks every smiles_* wrapper makes on its rows: ys int64 [n, W >= 1] with unit column stride and the
    per-row `vectors` (name -> (tensor, dtype): start, key), contiguous [n].  Returns (n, W, the rows' stride).  `name`
    (the caller's) opens every message, here and in the helpers below."""
    _chk(ys, f"{name}.ys", torch.int64)
    if ys.dim() != 2 or ys.shape[1] < 1 or (ys.shape[1] > 1 and ys.stride(1) != 1):
        raise ValueError(f"{name}: ys [n, W >= 1] with unit column stride")
    n, W = ys.shape
    for what, (t, dtype) in vectors.items():
        _chk(t, f"{name}.{what}", dtype)
        if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous tensor [{n}], got {list(t.shape)}")
    return n, W, max(W, ys.stride(0))


def _smiles_tables(name, **tables):
    """The per-token tables (name -> (tensor, dtype)): contiguous [V >= 1], all of one shape.  Returns V."""
    V = None
    for what, (t, dtype) in tables.items():
        _chk(t, f"{name}.{what}", dtype)
        if t.dim() != 1 or t.numel() < 1 or not t.is_contiguous() or t.numel() != (V or t.numel()):
            raise ValueError(f"{name}: {' and '.join(tables)} must be contiguous [V] tensors of one length, got "
                             f"{list(t.shape)} for {what}")
        V = t.numel()
    return V


def _smiles_rings(name, ring_ids, n_rings):
    _chk(ring_ids, f"{name}.ring_ids", torch.int32)
    if ring_ids.dim() != 1 or ring_ids.numel() != 64 or not ring_ids.is_contiguous() or not 0 <= int(n_rings) <= 63:
        raise ValueError(f"{name}: ring_ids int32 [64], contiguous, with at most 63 numbers in use")


def _smiles_ids(name, V, needed, optional):
    """Token ids (name -> id): `needed` in [0, V), `optional` in [-1, V) with -1 for none."""
    for ids, lo, note in ((needed, 0, ""), (optional, -1, " (-1: none)")):
        for what, v in ids.items():
            if not lo <= int(v) < V:
                raise ValueError(f"{name}: {what} {v} is outside the vocabulary of {V} tokens{note}")


def _smiles_out(name, given, like, **wanted):
    """The outputs (name -> (shape, dtype)): freshly allocated on like's device, or the contiguous tensors of the tuple
    `given`, one per entry.  Returns the tuple."""
    if given is None:
        return tuple(torch.empty(shape, dtype=dtype, device=like.device) for shape, dtype in wanted.values())
    given = tuple(given)
    if len(given) != len(wanted):
        raise ValueError(f"{name}: out = ({', '.join(wanted)})")
    for (what, (shape, dtype)), t in zip(wanted.items(), given):
        _chk(t, f"{name}.out {what}", dtype)
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{name}: out must hold contiguous tensors {[list(w[0]) for w in wanted.values()]}, got "
                             f"{list(t.shape)} for {what}")
    return given


def smiles_check(ys, start, table, chem, out=None):
    """gct_smiles_check: out int32 [n, 4] = (status, position, atoms, ring_bonds) of every row's span ys[r, start[r]:]
    (smiles.SmilesChemistry.check is the statement).  ys int64 [n, W] with unit column stride, start int32 [n] on the
    device with 0 <= start[r] <= W and W - start[r] <= 256 (the caller's to guarantee: a row outside that range is
    reported as SYNTAX at position 0), table / chem int32 [V] (SmilesChemistry.device_tables).  One launch."""
    n, W, ld = _smiles_rows("smiles_check", ys, start=(start, torch.int32))
    V = _smiles_tables("smiles_check", table=(table, torch.int32), chem=(chem, torch.int32))
    if out is None:
        out = torch.empty(n, 4, dtype=torch.int32, device=ys.device)
    _chk(out, "smiles_check.out", torch.int32)
    if tuple(out.shape) != (n, 4) or not out.is_contiguous():
        raise ValueError(f"smiles_check: out must be a contiguous int32 tensor [{n}, 4], got {list(out.shape)}")
    if n:
        check(_L().gct_smiles_check(_p(ys), ld, W, n, _p(start), V, _p(table), _p(chem), _p(out), _st()),
              "gct_smiles_check")
    return out


# status codes of the SMILES randomiser (GCT_RAND_* of include/gctplus_hip.h), the site of its Philox streams
# (GCT_SITE_RANDOMIZE of csrc/common.h) and its per-token word:
# class | ring number << 8 | bond order << 16 | unsupported (a / or \ bond, an atom with @) << 20
RAND_OK, RAND_KEPT, RAND_SYNTAX, RAND_UNSUPPORTED, RAND_NO_RING, RAND_TOO_LONG = range(6)
RAND_MAX_SPAN = SMILES_MAX_SPAN
RANDOMIZE_SITE = 0x5A11E5


def smiles_randomize(ys, start, key, table, ring_ids, n_rings, open_id, close_id, pad_id, eos_id, sep_id, seed, p,
                     out_width=None, return_perm=False, out=None):
    """gct_smiles_randomize: every row's span ys[r, start[r]:] written out again as a random spelling of the same
    molecule (randomize.SmilesRandomizer.randomize_reference is the statement).  ys int64 [n, W] with unit column
    stride, start int32 [n] and key int64 [n] on the device, table int32 [V] and ring_ids int32 [64]
    (SmilesRandomizer.device_tables), sep_id -1 for none.  Returns (tokens int64 [n, out_width], info int32 [n, 4],
    perm int32 [n, out_width] or None), freshly allocated or the contiguous tensors of out = (tokens, info, perm or None).
    One launch."""
    name = "smiles_randomize"
    n, W, ld = _smiles_rows(name, ys, start=(start, torch.int32), key=(key, torch.int64))
    V = _smiles_tables(name, table=(table, torch.int32))
    _smiles_rings(name, ring_ids, n_rings)
    _smiles_ids(name, V, dict(open_id=open_id, close_id=close_id, pad_id=pad_id, eos_id=eos_id), dict(sep_id=sep_id))
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"{name}: p must be a probability in [0, 1], got {p}")
    out_width = W if out_width is None else int(out_width)
    if out_width < W:
        raise ValueError(f"{name}: out_width {out_width} is narrower than the rows ({W} columns)")
    with_perm = return_perm if out is None else tuple(out)[2:] != (None,)   # (without: the kernel takes a null pointer)
    wanted = dict(tokens=((n, out_width), torch.int64), info=((n, 4), torch.int32))
    if with_perm:
        wanted["perm"] = ((n, out_width), torch.int32)
    got = _smiles_out(name, out if out is None or with_perm else tuple(out)[:2], ys, **wanted)
    tokens, info, perm = got if with_perm else got + (None,)
    if n:
        check(_L().gct_smiles_randomize(_p(ys), ld, W, n, _p(start), _p(key), V, _p(table), _p(ring_ids), int(n_rings),
                                        int(open_id), int(close_id), int(pad_id), int(eos_id), int(sep_id),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), _p(tokens), _p(info), _p(perm),
                                        out_width, _st()), "gct_smiles_randomize")
    return tokens, info, perm


# status codes of the molecule keys (GCT_KEY_* of include/gctplus_hip.h) and the rounds of refinement, GCT_KEY_ROUNDS
KEY_GRAPH, KEY_STRING_SYNTAX, KEY_STRING_UNSUPPORTED = range(3)
KEY_ROUNDS = 3
KEY_MAX_SPAN = SMILES_MAX_SPAN


def smiles_key(ys, start, table32, label64, pad_id, eos_id, sep_id, out=None):
    """gct_smiles_key: a spelling-independent 64-bit key of the molecule in every row's span ys[r, start[r]:], and of the
    scaffold in front of a <sep> (molkey.SmilesKeys.key_reference is the statement).  ys int64 [n, W] with unit column
    stride, start int32 [n] on the device, table32 int32 [V] and label64 int64 [V] (SmilesKeys.device_tables), sep_id -1
    for none.  Returns (key int64 [n, 2], info int32 [n, 4]), freshly allocated or the contiguous tensors of
    out = (key, info).  One launch."""
    n, W, ld = _smiles_rows("smiles_key", ys, start=(start, torch.int32))
    V = _smiles_tables("smiles_key", table32=(table32, torch.int32), label64=(label64, torch.int64))
    _smiles_ids("smiles_key", V, dict(pad_id=pad_id, eos_id=eos_id), dict(sep_id=sep_id))
    key, info = _smiles_out("smiles_key", out, ys, key=((n, 2), torch.int64), info=((n, 4), torch.int32))
    if n:
        check(_L().gct_smiles_key(_p(ys), ld, W, n, _p(start), V, _p(table32), _p(label64), int(pad_id), int(eos_id),
                                  int(sep_id), _p(key), _p(info), _st()), "gct_smiles_key")
    return key, info


# status codes of the Murcko scaffolds (GCT_SCA_* of include/gctplus_hip.h)
SCA_OK, SCA_ACYCLIC, SCA_SYNTAX, SCA_UNSUPPORTED, SCA_NO_TOKEN, SCA_NO_RING, SCA_TOO_LONG = range(7)
SCA_MAX_SPAN = SMILES_MAX_SPAN


def smiles_scaffold(ys, start, table32, label64, ring_ids, n_rings, open_id, close_id, pad_id, eos_id, sep_id, n_id,
                    nh_id, out_width=None, out=None):
    """gct_smiles_scaffold: the Murcko scaffold of the molecule in every row's span ys[r, start[r]:] -- its key, its
    spelling and the atoms it keeps -- and the key of the scaffold in front of a <sep>
    (scaffold.SmilesScaffolds.scaffold_reference is the statement).  ys int64 [n, W] with unit column stride, start int32
    [n] on the device, table32 int32 [V] and label64 int64 [V] (SmilesKeys.device_tables), ring_ids int32 [64]
    (SmilesRandomizer.device_tables); sep_id, n_id (the token `n`) and nh_id (`[nH]`) -1 for none.  Returns (tokens int64
    [n, out_width], key int64 [n, 2], info int32 [n, 4], member int32 [n, W]), freshly allocated or the contiguous
    tensors of out = (tokens, key, info, member).  One launch."""
    name = "smiles_scaffold"
    n, W, ld = _smiles_rows(name, ys, start=(start, torch.int32))
    V = _smiles_tables(name, table32=(table32, torch.int32), label64=(label64, torch.int64))
    _smiles_rings(name, ring_ids, n_rings)
    _smiles_ids(name, V, dict(open_id=open_id, close_id=close_id, pad_id=pad_id, eos_id=eos_id),
                dict(sep_id=sep_id, n_id=n_id, nh_id=nh_id))
    out_width = W if out_width is None else int(out_width)
    if out_width < 1:
        raise ValueError(f"{name}: out_width {out_width} has no column for <eos>")
    out = _smiles_out(name, out, ys, tokens=((n, out_width), torch.int64), key=((n, 2), torch.int64),
                      info=((n, 4), torch.int32), member=((n, W), torch.int32))
    tokens, key, info, member = out
    if n:
        check(_L().gct_smiles_scaffold(_p(ys), ld, W, n, _p(start), V, _p(table32), _p(label64), _p(ring_ids),
                                       int(n_rings), int(open_id), int(close_id), int(pad_id), int(eos_id), int(sep_id),
                                       int(n_id), int(nh_id), _p(tokens), out_width, _p(key), _p(info), _p(member),
                                       _st()), "gct_smiles_scaffold")
    return out


# status codes of the circular fingerprints (GCT_FP_* of include/gctplus_hip.h), their radius and their width in bits
FP_GRAPH, FP_SYNTAX, FP_UNSUPPORTED = range(3)
FP_RADIUS = 2
FP_BITS = 1024
FP_WORDS = FP_BITS // 64
FP_MAX_SPAN = SMILES_MAX_SPAN


def smiles_fp(ys, start, table32, label64, pad_id, eos_id, sep_id, out=None):
    """gct_smiles_fp: the FP_BITS-bit circular fingerprint of the molecule in every row's span ys[r, start[r]:] -- behind
    a <sep> if there is one (fingerprint.SmilesFingerprints.fp_reference is the statement).  ys int64 [n, W] with unit
    column stride, start int32 [n] on the device, table32 int32 [V] and label64 int64 [V] (SmilesKeys.device_tables),
    sep_id -1 for none.  Returns (bits int64 [n, 16], info int32 [n, 4] = (status, bits set, atoms, bonds)), freshly
    allocated or the contiguous tensors of out = (bits, info).  One launch."""
    n, W, ld = _smiles_rows("smiles_fp", ys, start=(start, torch.int32))
    V = _smiles_tables("smiles_fp", table32=(table32, torch.int32), label64=(label64, torch.int64))
    _smiles_ids("smiles_fp", V, dict(pad_id=pad_id, eos_id=eos_id), dict(sep_id=sep_id))
    bits, info = _smiles_out("smiles_fp", out, ys, bits=((n, FP_WORDS), torch.int64), info=((n, 4), torch.int32))
    if n:
        check(_L().gct_smiles_fp(_p(ys), ld, W, n, _p(start), V, _p(table32), _p(label64), int(pad_id), int(eos_id),
                                 int(sep_id), _p(bits), _p(info), _st()), "gct_smiles_fp")
    return bits, info


# status codes of the molecular descriptors (GCT_DESC_* of include/gctplus_hip.h) and the columns of a row
DESC_OK, DESC_SYNTAX, DESC_UNSUPPORTED, DESC_UNKNOWN_ATOM = range(4)
(DESC_STATUS, DESC_HEAVY_ATOMS, DESC_HYDROGENS, DESC_MW_MDA, DESC_CHARGE, DESC_HBD, DESC_HBA, DESC_ROTATABLE, DESC_RINGS,
 DESC_AROMATIC_RINGS, DESC_TPSA_CENTI, DESC_RING_BONDS) = range(12)
DESC_COLUMNS = 12
DESC_MAX_SPAN = SMILES_MAX_SPAN


def smiles_desc(ys, start, table32, desc32, pad_id, eos_id, sep_id, out=None):
    """gct_smiles_desc: the integer descriptors of the molecule in every row's span ys[r, start[r]:] -- behind a <sep> if
    there is one (descriptor.SmilesDescriptors.desc_reference is the statement).  ys int64 [n, W] with unit column
    stride, start int32 [n] on the device, table32 int32 [V] (SmilesKeys.device_tables) and desc32 int32 [V]
    (SmilesDescriptors.device_tables), sep_id -1 for none.  Returns values int32 [n, 12] (the DESC_* columns), freshly
    allocated or the contiguous tensor `out`.  One launch."""
    n, W, ld = _smiles_rows("smiles_desc", ys, start=(start, torch.int32))
    V = _smiles_tables("smiles_desc", table32=(table32, torch.int32), desc32=(desc32, torch.int32))
    _smiles_ids("smiles_desc", V, dict(pad_id=pad_id, eos_id=eos_id), dict(sep_id=sep_id))
    values, = _smiles_out("smiles_desc", None if out is None else (out,), ys, values=((n, DESC_COLUMNS), torch.int32))
    if n:
        check(_L().gct_smiles_desc(_p(ys), ld, W, n, _p(start), V, _p(table32), _p(desc32), int(pad_id), int(eos_id),
                                   int(sep_id), _p(values), _st()), "gct_smiles_desc")
    return values


def fp_tanimoto_plan(n, m):
    """(tile_b, splits) of gct_fp_tanimoto for n rows of a against m rows of b: b is walked in tiles of tile_b rows, in
    `splits` independent parts whose partials a second launch folds.  A function of (n, m) alone, never of the device."""
    if int(n) < 0 or int(m) < 0:
        raise ValueError(f"fp_tanimoto_plan: n = {n}, m = {m}")
    return _L().gct_fp_tanimoto_tile_b(), _L().gct_fp_tanimoto_splits(int(n), int(m))


def _fp_rows(name, what, bits, cnt):
    _chk(bits, f"{name}.{what}", torch.int64)
    _chk(cnt, f"{name}.cnt_{what}", torch.int32)
    if bits.dim() != 2 or bits.shape[1] != FP_WORDS or bits.stride(1) != 1 or (bits.shape[0] > 1 and bits.stride(0) < FP_WORDS):
        raise ValueError(f"{name}: {what} int64 [rows, {FP_WORDS}] with unit column stride and a row stride of at least "
                         f"{FP_WORDS}, got {list(bits.shape)} with strides {list(bits.stride())}")
    if cnt.dim() != 1 or cnt.numel() != bits.shape[0] or not cnt.is_contiguous():
        raise ValueError(f"{name}: cnt_{what} must be a contiguous tensor [{bits.shape[0]}], got {list(cnt.shape)}")
    if cnt.device != bits.device:
        raise ValueError(f"{name}: {what} and cnt_{what} are on different devices")
    return bits.shape[0], max(FP_WORDS, bits.stride(0))


def fp_tanimoto(a, cnt_a, b, cnt_b, p=1, out=None):
    """gct_fp_tanimoto: for every row of a, over the present rows of b (fingerprint.tanimoto_reference is the statement),
    (best fp32 [n] = the largest Tanimoto similarity, arg int32 [n] = the lowest row of b that attains it, total fp64 [n]
    = the sum of T^p, p 1 or 2).  a int64 [n, 16], b int64 [m, 16]: smiles_fp's words, unit column stride, any row
    stride of at least 16; cnt_a, cnt_b int32: their numbers of set bits, 0 for an absent row.  An absent row of a, and
    every row when no row of b is present: (0, -1, 0).  Freshly allocated or the contiguous tensors of
    out = (best, arg, total).  One launch, two when fp_tanimoto_plan(n, m) has more than one split."""
    name = "fp_tanimoto"
    n, lda = _fp_rows(name, "a", a, cnt_a)
    m, ldb = _fp_rows(name, "b", b, cnt_b)
    if b.device != a.device:
        raise ValueError(f"{name}: a and b are on different devices")
    if int(p) not in (1, 2):
        raise ValueError(f"{name}: p must be 1 or 2, got {p}")
    if m > 1 << 30:
        raise ValueError(f"{name}: {m} rows of b, at most 2^30")
    best, arg, total = _smiles_out(name, out, a, best=((n,), torch.float32), arg=((n,), torch.int32),
                                   total=((n,), torch.float64))
    if n:
        nbytes = _L().gct_fp_tanimoto_ws_bytes(n, m)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=a.device) if nbytes else None
        check(_L().gct_fp_tanimoto(_p(a), lda, _p(cnt_a), n, _p(b), ldb, _p(cnt_b), m, int(p), _p(ws), nbytes, _p(best),
                                   _p(arg), _p(total), _st()), "gct_fp_tanimoto")
    return best, arg, total


def _seq_geometry(name, logits2d, ys, rows_per_seq, V, prefix_lens, prior2d=None):
    """The checks every seq_* wrapper makes on (ys, logits, prefix_lens), with seq_dist's prior logits next to the
    agent's: (n, W, R, V, ld, ld_prior).  `name` (the caller's) opens every message, here and in the helpers below."""
    _chk(ys, f"{name}.ys", torch.int64)
    if ys.dim() != 2 or ys.stride(1) != 1:
        raise ValueError(f"{name}: ys must be [n, W] with unit column stride")
    n, W = ys.shape
    R = W - 1 if rows_per_seq is None else int(rows_per_seq)
    ld = ld_prior = 0
    if logits2d is not None:
        _chk(logits2d, f"{name}.logits")
        if logits2d.dim() != 2 or logits2d.stride(1) != 1 or logits2d.shape[0] < n * R:
            raise ValueError(f"{name}: logits must be [>= {n * R}, V] with unit column stride, got "
                             f"{list(logits2d.shape)}")
        V, ld = logits2d.shape[1], logits2d.stride(0)
    if prior2d is not None:
        _chk(prior2d, f"{name}.prior_logits")
        if prior2d.dim() != 2 or prior2d.stride(1) != 1 or prior2d.shape[0] < n * R or prior2d.shape[1] != int(V):
            raise ValueError(f"{name}: prior logits must be [>= {n * R}, {int(V)}] with unit column stride, got "
                             f"{list(prior2d.shape)}")
        ld_prior = prior2d.stride(0)
    if prefix_lens is not None:
        _check_row_off(prefix_lens, n)
    return n, W, R, int(V), ld, ld_prior


def _seq_vector(name, what, t, n):
    """A per-sequence input (an incoming gradient, PPO's advantage): None, or fp32 [n] contiguous."""
    if t is not None:
        _chk(t, f"{name}.{what}")
        if t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous fp32 tensor of {n} entries")


def _seq_table(name, what, t, n, W):
    """A per-token input (an incoming gradient, PPO's old_token_logp): None, or fp32 [n, W] with unit column stride.
    Returns the row stride to pass (0 for None)."""
    if t is None:
        return 0
    _chk(t, f"{name}.{what}")
    if t.shape != (n, W) or t.stride(1) != 1:
        raise ValueError(f"{name}: {what} must be [{n}, {W}] with unit column stride")
    return t.stride(0)


def _seq_dlogits(name, out, logits2d, ys, R, V, launch):
    """What every backward wrapper does with its result: allocate dlogits in the shape of logits2d (zeros on the rows
    behind the last sequence: they belong to nobody) or validate the caller's `out`, then `launch(dlogits)` -- unless
    there is no sequence: nothing to write then (an empty tensor has no address).  Returns dlogits."""
    n = ys.shape[0]
    if out is None:
        rows = max(n * R, 0 if logits2d is None else logits2d.shape[0])
        out = torch.empty(rows, V, device=ys.device)
        if rows > n * R:
            out[n * R:].zero_()
    _chk(out, f"{name}.dlogits")
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n * R or out.shape[1] != V:
        raise ValueError(f"{name}: out must be [>= {n * R}, {V}] with unit column stride")
    if n:
        launch(out)
    return out


def seq_logp(logits2d, ys, prefix_lens=None, pad_id=1, row_shift=0, rows_per_seq=None, V=None, out=None):
    """gct_seq_logp (decode.score_reference states the rule): ys int64 [n, W] full token rows, logits2d fp32
    [n * rows_per_seq, V] with unit column stride (a strided view is fine: ld = its row stride); the logits row of token
    column c of sequence r is r * rows_per_seq + row_shift + c - 1 (rows_per_seq defaults to W - 1).  prefix_lens int32
    [n] on the device or None (every row: 1).  logits2d None (with V given) passes a null pointer: the library refuses.
    Returns (token_logp [n, W] fp32, logp [n] fp32, tokens [n] int32, hits [n] int32), or fills `out`, a tuple of them."""
    n, W, R, V, ld, _ = _seq_geometry("seq_logp", logits2d, ys, rows_per_seq, V, prefix_lens)
    dev = ys.device
    if out is None:
        out = (torch.empty(n, W, device=dev), torch.empty(n, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    tl, lp, nt, nh = out
    _chk(tl, "seq_logp.token_logp"), _chk(lp, "seq_logp.logp")
    _chk(nt, "seq_logp.tokens", torch.int32), _chk(nh, "seq_logp.hits", torch.int32)
    if tl.shape != (n, W) or tl.stride(1) != 1 or any(t.numel() != n or not t.is_contiguous() for t in (lp, nt, nh)):
        raise ValueError("seq_logp: out must be (token_logp [n, W], logp [n], tokens [n], hits [n])")
    check(_L().gct_seq_logp(_p(logits2d), ld, V, R, int(row_shift), _p(ys), ys.stride(0), _p(prefix_lens),
                            int(pad_id), n, W, _p(tl), tl.stride(0), _p(lp), _p(nt), _p(nh), _st()), "gct_seq_logp")
    return out


def seq_logp_bwd(logits2d, ys, prefix_lens=None, pad_id=1, row_shift=0, rows_per_seq=None, g_logp=None, g_token=None,
                 V=None, out=None):
    """gct_seq_logp_bwd (decode.seq_logp_grad_reference states the rule): the gradient of seq_logp's logp [n] and
    token_logp [n, W] with respect to the logits, for the geometry seq_logp takes (same checks: ys int64 [n, W], logits2d
    fp32 [>= n * rows_per_seq, V] with unit column stride, a strided view is fine; prefix_lens int32 [n] or None).
    g_logp fp32 [n] / g_token fp32 [n, W] with unit column stride: the incoming gradients, either may be None (0), the
    library refuses both.  logits2d None (with V given) passes a null pointer: the library refuses.
    Returns dlogits fp32, contiguous, in the shape of logits2d (or fills `out`, [>= n * rows_per_seq, V] with unit column
    stride): every row is written -- zeros on the rows that are not scored or whose weight is 0, whose logits are not
    read."""
    n, W, R, V, ld, _ = _seq_geometry("seq_logp_bwd", logits2d, ys, rows_per_seq, V, prefix_lens)
    _seq_vector("seq_logp_bwd", "g_logp", g_logp, n)
    ld_g = _seq_table("seq_logp_bwd", "g_token", g_token, n, W)
    return _seq_dlogits("seq_logp_bwd", out, logits2d, ys, R, V, lambda dl: check(_L().gct_seq_logp_bwd(
        _p(logits2d), ld, V, R, int(row_shift), _p(ys), ys.stride(0), _p(prefix_lens), int(pad_id), n, W, _p(g_logp),
        _p(g_token), ld_g, _p(dl), dl.stride(0), _st()), "gct_seq_logp_bwd"))


def seq_dist(logits2d, ys, prefix_lens=None, pad_id=1, row_shift=0, rows_per_seq=None, prior_logits2d=None, V=None,
             out=None):
    """gct_seq_dist (decode.dist_reference states the rule): the entropy of the next-token distribution and -- with
    prior_logits2d, a second model's logits in the same row numbering (its own row stride) -- its KL divergence from
    that model's, for the geometry seq_logp takes (same checks on ys, logits2d, prefix_lens; logits2d None with V given
    passes a null pointer: the library refuses).
    Returns (token_entropy [n, W], entropy [n], token_kl [n, W] | None, kl [n] | None) fp32, or fills `out`, a tuple of
    them (the kl pair None exactly when there is no prior; otherwise the library refuses)."""
    n, W, R, V, ld, ld_prior = _seq_geometry("seq_dist", logits2d, ys, rows_per_seq, V, prefix_lens, prior_logits2d)
    dev = ys.device
    if out is None:
        out = (torch.empty(n, W, device=dev), torch.empty(n, device=dev))
        out += (None, None) if prior_logits2d is None else (torch.empty(n, W, device=dev), torch.empty(n, device=dev))
    te, en, tk, kl = out
    if (tk is None) != (kl is None):
        raise ValueError("seq_dist: out needs both token_kl and kl, or neither")
    for tab, vec, what in ((te, en, "entropy"), (tk, kl, "kl"))[:1 if tk is None else 2]:
        _chk(tab, f"seq_dist.token_{what}"), _chk(vec, f"seq_dist.{what}")
        if tab.shape != (n, W) or tab.stride(1) != 1 or vec.numel() != n or not vec.is_contiguous():
            raise ValueError(f"seq_dist: out must hold token_{what} [n, W] and {what} [n]")
    if tk is not None and tk.stride(0) != te.stride(0):
        raise ValueError("seq_dist: token_entropy and token_kl must have one row stride")
    if n == 0:
        return out                                       # no sequence: nothing to write (an empty tensor has no address)
    check(_L().gct_seq_dist(_p(logits2d), ld, V, R, int(row_shift), _p(prior_logits2d), ld_prior, _p(ys), ys.stride(0),
                            _p(prefix_lens), int(pad_id), n, W, _p(te), te.stride(0), _p(en), _p(tk), _p(kl), _st()),
          "gct_seq_dist")
    return out


def seq_dist_bwd(logits2d, ys, prefix_lens=None, pad_id=1, row_shift=0, rows_per_seq=None, prior_logits2d=None,
                 g_entropy=None, g_token_entropy=None, g_kl=None, g_token_kl=None, V=None, out=None):
    """gct_seq_dist_bwd (decode.dist_grad_reference states the rule): the gradient of seq_dist's four outputs with
    respect to the AGENT's logits, for the geometry seq_dist takes (same checks).  g_entropy / g_kl fp32 [n],
    g_token_entropy / g_token_kl fp32 [n, W] with unit column stride: the incoming gradients, each may be None (0); the
    library refuses all four None, and the kl pair without prior_logits2d.
    Returns dlogits fp32, contiguous, in the shape of logits2d (or fills `out`, [>= n * rows_per_seq, V] with unit column
    stride): every row is written -- zeros on the rows that are not scored or whose weights are 0, where neither model's
    logits are read."""
    n, W, R, V, ld, ld_prior = _seq_geometry("seq_dist_bwd", logits2d, ys, rows_per_seq, V, prefix_lens, prior_logits2d)
    _seq_vector("seq_dist_bwd", "g_entropy", g_entropy, n), _seq_vector("seq_dist_bwd", "g_kl", g_kl, n)
    ld_ge = _seq_table("seq_dist_bwd", "g_token_entropy", g_token_entropy, n, W)
    ld_gk = _seq_table("seq_dist_bwd", "g_token_kl", g_token_kl, n, W)
    return _seq_dlogits("seq_dist_bwd", out, logits2d, ys, R, V, lambda dl: check(_L().gct_seq_dist_bwd(
        _p(logits2d), ld, V, R, int(row_shift), _p(prior_logits2d), ld_prior, _p(ys), ys.stride(0), _p(prefix_lens),
        int(pad_id), n, W, _p(g_entropy), _p(g_token_entropy), ld_ge, _p(g_kl), _p(g_token_kl), ld_gk, _p(dl),
        dl.stride(0), _st()), "gct_seq_dist_bwd"))


def _ppo_inputs(name, old_token_logp, advantage, n, W):
    """The checks seq_ppo / seq_ppo_bwd make on the sampling-time table and the advantages (None passes a null pointer:
    the library refuses): the row stride of old_token_logp."""
    ld_old = _seq_table(name, "old_token_logp", old_token_logp, n, W)
    _seq_vector(name, "advantage", advantage, n)
    return ld_old


def seq_ppo(logits2d, ys, old_token_logp, advantage, clip_lo, clip_hi, prefix_lens=None, pad_id=1, row_shift=0,
            rows_per_seq=None, V=None, out=None):
    """gct_seq_ppo (decode.ppo_reference states the rule): PPO's clipped surrogate of the scored tokens, for the geometry
    seq_logp takes (same checks on ys, logits2d, prefix_lens; logits2d None with V given passes a null pointer: the
    library refuses).  old_token_logp fp32 [n, W] with unit column stride (its own row stride), advantage fp32 [n],
    clip_lo in [0, 1), clip_hi >= 0 (the library refuses others).
    Returns (token_logp [n, W], token_surrogate [n, W], logp [n], surrogate [n], approx_kl [n] fp32, tokens [n],
    hits [n], clipped [n] int32), or fills `out`, a tuple of them (the two tables with one row stride)."""
    n, W, R, V, ld, _ = _seq_geometry("seq_ppo", logits2d, ys, rows_per_seq, V, prefix_lens)
    ld_old = _ppo_inputs("seq_ppo", old_token_logp, advantage, n, W)
    dev = ys.device
    if out is None:
        out = (torch.empty(n, W, device=dev), torch.empty(n, W, device=dev)) + tuple(
            torch.empty(n, device=dev) for _ in range(3)) + tuple(
            torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    tl, ts, lp, su, kl, nt, nh, nc = out
    for t in (tl, ts, lp, su, kl):
        _chk(t, "seq_ppo.out")
    _chk(nt, "seq_ppo.tokens", torch.int32), _chk(nh, "seq_ppo.hits", torch.int32)
    _chk(nc, "seq_ppo.clipped", torch.int32)
    if (any(t.shape != (n, W) or t.stride(1) != 1 for t in (tl, ts)) or tl.stride(0) != ts.stride(0) or
            any(t.numel() != n or not t.is_contiguous() for t in (lp, su, kl, nt, nh, nc))):
        raise ValueError("seq_ppo: out must be (token_logp [n, W], token_surrogate [n, W] of one row stride, logp [n], "
                         "surrogate [n], approx_kl [n], tokens [n], hits [n], clipped [n])")
    if n == 0:
        return out                                       # no sequence: nothing to write (an empty tensor has no address)
    check(_L().gct_seq_ppo(_p(logits2d), ld, V, R, int(row_shift), _p(ys), ys.stride(0), _p(prefix_lens), int(pad_id), n,
                           W, _p(old_token_logp), ld_old, _p(advantage), float(clip_lo), float(clip_hi), _p(tl), _p(ts),
                           tl.stride(0), _p(lp), _p(su), _p(kl), _p(nt), _p(nh), _p(nc), _st()), "gct_seq_ppo")
    return out


def seq_ppo_bwd(logits2d, ys, old_token_logp, advantage, clip_lo, clip_hi, prefix_lens=None, pad_id=1, row_shift=0,
                rows_per_seq=None, g_surrogate=None, g_token_surrogate=None, V=None, out=None):
    """gct_seq_ppo_bwd (decode.ppo_grad_reference states the rule): the gradient of seq_ppo's surrogate [n] and
    token_surrogate [n, W] with respect to the logits, for the geometry and inputs seq_ppo takes (same checks).
    g_surrogate fp32 [n] / g_token_surrogate fp32 [n, W] with unit column stride: the incoming gradients, either may be
    None (0), the library refuses both.
    Returns dlogits fp32, contiguous, in the shape of logits2d (or fills `out`, [>= n * rows_per_seq, V] with unit column
    stride): every row is written -- zeros on the rows that are not scored, whose advantage or weight is 0 (their logits
    are not read), and on the rows of clipped tokens."""
    n, W, R, V, ld, _ = _seq_geometry("seq_ppo_bwd", logits2d, ys, rows_per_seq, V, prefix_lens)
    ld_old = _ppo_inputs("seq_ppo_bwd", old_token_logp, advantage, n, W)
    _seq_vector("seq_ppo_bwd", "g_surrogate", g_surrogate, n)
    ld_g = _seq_table("seq_ppo_bwd", "g_token_surrogate", g_token_surrogate, n, W)
    return _seq_dlogits("seq_ppo_bwd", out, logits2d, ys, R, V, lambda dl: check(_L().gct_seq_ppo_bwd(
        _p(logits2d), ld, V, R, int(row_shift), _p(ys), ys.stride(0), _p(prefix_lens), int(pad_id), n, W,
        _p(old_token_logp), ld_old, _p(advantage), float(clip_lo), float(clip_hi), _p(g_surrogate),
        _p(g_token_surrogate), ld_g, _p(dl), dl.stride(0), _st()), "gct_seq_ppo_bwd"))


def chosen_logp(logits2d, ys, pos_dev, out, pad_id, row_off=None, item=None, prefix_len=None):
    """gct_chosen_logp, after select_token on the same logits [n, V] and device counter: out[dst, p] = the model's
    log-probability (raw logits, temperature 1) of the token ys[r, p] the selection has just written at
    p = *pos_dev - row_off[r] + 1, 0 for pad.  item / prefix_len as in select_token: dst = item[r], nothing written for a
    parked row or a prefix token; otherwise dst = r.  out fp32 [rows, >= width], unit column stride."""
    n, V = logits2d.shape
    _chk(logits2d, "chosen_logp.logits"), _chk(out, "chosen_logp.out"), _chk(ys, "chosen_logp.ys", torch.int64)
    _chk(pos_dev, "chosen_logp.pos", torch.int32)
    if not logits2d.is_contiguous() or out.dim() != 2 or out.stride(1) != 1 or ys.stride(1) != 1:
        raise ValueError("chosen_logp: contiguous logits and unit column strides of ys / out")
    _check_step_rows(n, row_off, item, prefix_len=prefix_len)
    check(_L().gct_chosen_logp(_p(logits2d), V, _p(ys), ys.stride(0), _p(pos_dev), _p(row_off), _p(item),
                               _p(prefix_len), int(pad_id), _p(out), out.stride(0), out.shape[0], n, _st()),
          "gct_chosen_logp")


STEP_STATS = ("model_entropy", "behaviour_logp", "behaviour_entropy", "behaviour_kl")     # gct_step_stats' tables


def step_stats(logits2d, probs, ys, pos_dev, pad_id, greedy=False, row_off=None, item=None, prefix_len=None, **out):
    """gct_step_stats, after select_token on the same raw logits [n, V] and device counter (decode.step_stats_reference
    states the rules).  probs [n, V] or None: what select_token wrote to probs_out in this step -- the behaviour
    distribution q; None: q = the model's own softmax; greedy: q = the one-hot at the chosen token.  **out: the tables
    to write, any of STEP_STATS, at least one -- fp32 [rows, >= width] of one shape and row stride, unit column
    stride, written at (dst, p) with chosen_logp's dst and p, 0 for pad.  item / prefix_len / row_off as in chosen_logp."""
    n, V = logits2d.shape
    _chk(logits2d, "step_stats.logits"), _chk(ys, "step_stats.ys", torch.int64)
    _chk(pos_dev, "step_stats.pos", torch.int32)
    tables = [out.pop(name, None) for name in STEP_STATS]
    if out:
        raise ValueError(f"step_stats: no table named {sorted(out)} (the tables are {', '.join(STEP_STATS)})")
    given = [t for t in tables if t is not None]
    if not given:
        raise ValueError(f"step_stats: no table to write ({', '.join(STEP_STATS)})")
    for name, t in zip(STEP_STATS, tables):
        if t is not None:
            _chk(t, f"step_stats.{name}")
            if t.dim() != 2 or t.stride(1) != 1 or t.shape != given[0].shape or t.stride(0) != given[0].stride(0):
                raise ValueError("step_stats: the tables are fp32 [rows, width] of one shape and row stride, unit "
                                 "column stride")
    if n == 0:                                              # nothing to do (and an empty tensor has no address to pass)
        return
    if not logits2d.is_contiguous() or ys.dim() != 2 or ys.shape[0] < n or ys.stride(1) != 1 or pos_dev.numel() < 1:
        raise ValueError("step_stats: contiguous logits [n, V], ys [>= n, T] with unit column stride, a device counter")
    if probs is not None:
        _chk(probs, "step_stats.probs")
        if probs.shape != logits2d.shape or not probs.is_contiguous():
            raise ValueError("step_stats: probs must be a contiguous [n, V] buffer of the logits' shape")
    _check_step_rows(n, row_off, item, prefix_len=prefix_len)
    check(_L().gct_step_stats(_p(logits2d), _p(probs), V, _p(ys), ys.stride(0), _p(pos_dev), _p(row_off), _p(item),
                              _p(prefix_len), int(pad_id), int(bool(greedy)), *[_p(t) for t in tables],
                              given[0].stride(0), given[0].shape[0], n, _st()), "gct_step_stats")


STREAM_MAX_ROWS, STREAM_MAX_LAYERS = 8192, 16   # GCT_STREAM_MAX_ROWS / GCT_STREAM_MAX_LAYERS (include/gctplus_hip.h)


def stream_state_fields(header_text=None):
    """[(field, count)] of GctStreamState in declaration order, parsed from include/gctplus_hip.h (every field is 8
    bytes wide: a pointer or an int64_t; count > 1: an array)."""
    import re
    text = _lib._read_header("gctplus_hip.h") if header_text is None else header_text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    body = re.search(r"typedef\s+struct\s+GctStreamState\s*\{([^{}]*)\}\s*GctStreamState\s*;", text)
    if not body:
        raise _lib.GctError("include/gctplus_hip.h does not define GctStreamState")
    consts = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)\s*$", text, flags=re.M)}
    out = []
    for decl in body.group(1).split(";"):
        if not decl.strip():
            continue
        for part in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$", part.strip())
            dim = m.group(2)
            out.append((m.group(1), 1 if dim is None else (int(dim) if dim.isdigit() else consts[dim])))
    return out


class StreamState:
    """Host image of a GctStreamState: `set(name=tensor | int | [tensors])` fills fields, `refill()` enqueues
    gct_stream_refill on the current stream.  Holds the tensors it points to."""

    def __init__(self):
        import ctypes
        self.fields = stream_state_fields()
        self.slot, n = {}, 0
        for name, count in self.fields:
            self.slot[name] = (n, count)
            n += count
        self.words = (ctypes.c_int64 * n)()
        self.keep = {}

    def set(self, **kw):
        for name, v in kw.items():
            at, count = self.slot[name]
            vals = list(v) if isinstance(v, (list, tuple)) else [v]
            if len(vals) > count:
                raise ValueError(f"GctStreamState.{name} holds {count} entries, got {len(vals)}")
            self.keep[name] = vals
            for i in range(count):
                x = vals[i] if i < len(vals) else None
                self.words[at + i] = 0 if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else int(x))
        return self

    def refill(self):
        import ctypes
        check(_L().gct_stream_refill(ctypes.addressof(self.words), _st()), "gct_stream_refill")


def decode_embed(ys, pos, pe_off, table, pe, out, scale, row_off=None):
    """gct_decode_embed: out[b] = table[ys[b, p]] * scale + pe[pe_off + p], p = *pos (- row_off[b])."""
    n, d = out.shape
    _check_row_off(row_off, n)
    check(_L().gct_decode_embed(_p(ys), ys.stride(0), _p(pos), pe_off, _p(table), table.shape[0], _p(pe), _p(out), n, d,
                                scale, _p(row_off), _st()), "gct_decode_embed")


BEAM_MAX_K, BEAM_MAX_VOCAB = 16, 65536          # GCT_BEAM_MAX_K / GCT_BEAM_MAX_VOCAB (include/gctplus_hip.h)


def attn_decode_beam(q, ldq, k, v, kv_row, kv_batch, valid_u8, valid_sb, out, n, H, T, dk, pos, cache_off, knew, vnew,
                     ldn, kv_src):
    """gct_attn_decode_beam: the device-position attn_decode whose key / value / valid flag j of row b come from physical
    row kv_src[b, j] (int32 [n, >= T]); this step's key / value are appended to row b."""
    check(_L().gct_attn_decode_beam(_p(q), ldq, _p(k), _p(v), kv_row, kv_batch, _p(valid_u8), valid_sb, _p(out),
                                    out.stride(0), n, H, T, dk, 1.0 / math.sqrt(dk), _p(pos), cache_off, _p(knew),
                                    _p(vnew), ldn, _p(kv_src), kv_src.stride(0), _st()), "gct_attn_decode_beam")


def beam_select(logits2d, beam_size, scores, finished_u8, lengths_i32, ys, valid_u8, valid_off, kv_src, done_u8,
                pos_dev, pad_id, eos_id, parent_i32=None):
    """gct_beam_select over logits [n*k, V]: the k best children of each sample (decode.beam_step_reference), written
    in place to the beam state, ys[:, *pos_dev + 1], valid, the kv_src map and done [n]."""
    rows, V = logits2d.shape
    k = int(beam_size)
    T = kv_src.shape[1]
    check(_L().gct_beam_select(_p(logits2d), V, rows // k, k, _p(scores), _p(finished_u8), _p(lengths_i32),
                               _p(parent_i32), _p(ys), ys.stride(0), _p(valid_u8), valid_u8.stride(0), valid_off,
                               _p(kv_src), kv_src.stride(0), T, _p(done_u8), _p(pos_dev), pad_id, eos_id, _st()),
          "gct_beam_select")


def beam_select_gumbel(logits2d, beam_size, scores, gumbels, finished_u8, lengths_i32, ys, valid_u8, valid_off, kv_src,
                       done_u8, pos_dev, pad_id, eos_id, seed=0, seed_dev=None, noise_in=None, noise_out=None,
                       parent_i32=None):
    """gct_beam_select_gumbel over logits [n*k, V]: the stochastic beam step (decode.sbs_step_reference) -- beam_select
    with the rows' Gumbel values `gumbels` [n*k] fp32 as one more array of state, written in place like the rest.
    seed_dev (int64 / uint64 [1] on the device) replaces seed; noise_in [n*k, V] fp32 replaces the draw; noise_out
    [n*k, V] fp32 receives the variates used for live beams."""
    rows, V = logits2d.shape
    k = int(beam_size)
    T = kv_src.shape[1]
    for name, t in (("noise_in", noise_in), ("noise_out", noise_out)):
        if t is not None and (t.shape != logits2d.shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"beam_select_gumbel: {name} must be contiguous fp32 {list(logits2d.shape)}")
    check(_L().gct_beam_select_gumbel(_p(logits2d), V, rows // k, k, _p(scores), _p(finished_u8), _p(lengths_i32),
                                      _p(parent_i32), _p(ys), ys.stride(0), _p(valid_u8), valid_u8.stride(0), valid_off,
                                      _p(kv_src), kv_src.stride(0), T, _p(done_u8), _p(pos_dev), pad_id, eos_id,
                                      _p(gumbels), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(seed_dev), _p(noise_in),
                                      _p(noise_out), _st()), "gct_beam_select_gumbel")


def smc_select(logits2d, masked, particles, logw, logp, finished_u8, lengths_i32, ys, valid_u8, valid_off, kv_src, done_u8,
               pos_dev, pad_id, eos_id, log_z, resamples_i32, tau_dev, seed=0, seed_dev=None, u_in=None, u_out=None,
               parent_i32=None):
    """gct_smc_select over logits / masked [n*k, V] (raw rows, and the rows grammar_mask(kv_src=) wrote): one step of
    sequential Monte Carlo under the grammar (decode.smc_step_reference) -- weight, resample, draw -- written in place to
    the particle state (logw / logp fp32 [n*k], finished, lengths), log_z fp64 [n], resamples int32 [n], ys[:, *pos_dev +
    1], valid, the kv_src map and done [n].  tau_dev: fp32 [1] on the device, the ESS threshold; seed_dev (int64 [1] on
    the device) replaces seed; u_in fp32 [n, k + 1] replaces the k draw uniforms and the resampling uniform; u_out fp32
    [n, k + 1] receives the step's uniforms."""
    rows, V = logits2d.shape
    k = int(particles)
    n = rows // k
    T = kv_src.shape[1]
    _chk(logits2d, "smc_select.logits"), _chk(masked, "smc_select.masked"), _chk(logw, "smc_select.logw")
    _chk(logp, "smc_select.logp"), _chk(log_z, "smc_select.log_z", torch.float64), _chk(tau_dev, "smc_select.tau")
    _chk(resamples_i32, "smc_select.resamples", torch.int32)
    if not logits2d.is_contiguous() or not masked.is_contiguous() or masked.shape != logits2d.shape or n * k != rows:
        raise ValueError("smc_select: logits and masked must be contiguous [n*k, V] buffers of one shape")
    if min(logw.numel(), logp.numel(), finished_u8.numel(), lengths_i32.numel()) < rows or \
            min(log_z.numel(), resamples_i32.numel(), done_u8.numel()) < n or tau_dev.numel() < 1:
        raise ValueError("smc_select: particle state [n*k], sample state [n], tau [1]")
    for name, t in (("u_in", u_in), ("u_out", u_out)):
        if t is not None and (tuple(t.shape) != (n, k + 1) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"smc_select: {name} must be contiguous fp32 [{n}, {k + 1}]")
    check(_L().gct_smc_select(_p(logits2d), _p(masked), V, n, k, _p(logw), _p(logp), _p(finished_u8), _p(lengths_i32),
                              _p(parent_i32), _p(ys), ys.stride(0), _p(valid_u8), valid_u8.stride(0), valid_off,
                              _p(kv_src), kv_src.stride(0), T, _p(done_u8), _p(pos_dev), pad_id, eos_id, _p(log_z),
                              _p(resamples_i32), _p(tau_dev), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(seed_dev), _p(u_in),
                              _p(u_out), _st()), "gct_smc_select")
