"""Hand-written forward/backward passes of the GCT-Plus Transformer-VAE on top of the HIP
kernels (gct_plus_amd.ops).  No PyTorch arithmetic runs here: torch is used for device
memory (caching allocator), streams and the autograd *boundary* -- one autograd.Function per
trunk (encoder, sampler, decoder, linear, losses); inside a trunk the backward is explicit,
so residual-gradient joins, the 6-way accumulation of the encoder-memory gradient and the
dropout masks are handled by kernels/epilogues instead of autograd nodes.

Reference semantics (file:line relative to /root/reference):
  encoder layer   Model/layers.py:20-38   (residuals start from the NORMALISED x)
  decoder layer   Model/layers.py:56-82   (standard pre-norm)
  MHA             Model/sublayers.py:61-74, attention() :29-41
  FFN             Model/sublayers.py:85-89
  encoder/decoder Model/vaetf.py:32-54, 79-114 ; Model/cvaetf.py:35-61, 93-133
  sampler         Model/sublayers.py:14-26
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .flat import HANDED_SLOTS

_SEED = {"base": None, "ctr": 0}

# Compacted decoder backward (decoder_trunk_bwd): on by default, GCT_COMPACT_BWD=0 keeps the dense path.  Taken only
# when the compact rows are at most this fraction of all rows (the gathers cost ~1 ms per step).
COMPACT_BWD = os.environ.get("GCT_COMPACT_BWD", "1") != "0"
COMPACT_MAX_FRACTION = 0.85
# The three shortcuts of the row plan (read by RowPlan.launch only, decided by plan_rows):
# cross-attention over the visible rows of the encoder memory only: GCT_COMPACT_KV=0 disables.
COMPACT_KV = os.environ.get("GCT_COMPACT_KV", "1") != "0"
# decoder FORWARD over the rows that reach the loss only (loss_rows): GCT_COMPACT_FWD=0 disables.
COMPACT_FWD = os.environ.get("GCT_COMPACT_FWD", "1") != "0"
# K | V projections of the ENCODER self-attention over the visible rows only (mha_fwd): GCT_COMPACT_ENC_KV=0 disables.
COMPACT_ENC_KV = os.environ.get("GCT_COMPACT_ENC_KV", "1") != "0"
# Cross-attention K | V straight from the latent (ops.KvFold; decoder_trunk_fwd takes it when the memory has no cond2lat
# rows).  Tests flip this attribute to run the same model both ways (and restore it); there is no environment knob.
KV_FOLD = True


# Data parallelism (dp.FlatDataParallel) sets this while a backward pass is running: called as
# GRAD_NOTIFY(params, grads) when a trunk backward has finished writing the gradients of a layer, so that the layer's
# bucket of the flat gradient buffer can be exchanged while the layers underneath are still in their backward pass
# (autograd's post-accumulate hooks only fire when the whole trunk Function returns).
GRAD_NOTIFY = None


def _grads_done(module, G: "GradSink"):
    if GRAD_NOTIFY is not None:
        # with GCT_SIDE_STREAM=1 the layer's weight gradients were written on the side stream: the exchange that the
        # notifier may launch is ordered behind the CURRENT stream only, so the side stream joins first
        if ops.SIDE_ENABLED:
            ops.join_side()
        ps = list(module.parameters())
        GRAD_NOTIFY(ps, [G.out.get(p) for p in ps])


# Callers of the row planner (plan_rows)
MODEL = "model"          # the training-style forward, Vaetf / Cvaetf.forward (plan_ahead / prefetch included)
DECODER = "decoder"      # a Decoder called on its own: model.decode, the samplers
PREFILL = "prefill"      # decode.KVDecoder.prefill
ENCODER = "encoder"      # the encoder called on its own: model.encode


class RowMaps(NamedTuple):
    """plan_rows' answer: which maps to build, and the rows each one covers (for the usable_* tests)."""
    enc_keys: bool = False
    dec_keys: bool = False
    live: bool = False
    nc_lat: int = 0          # visible condition rows in front of the decoder's memory (use_cond2lat)
    enc_rows: int = 0        # B * Le
    dec_rows: int = 0        # B * (Le + nc_lat)
    live_rows: int = 0       # B * T, condition rows of use_cond2dec included


def plan_rows(caller, B=0, T=0, Le=0, mask_shape=None, *, loss_rows=False, trg_mask=False, get_attn=False,
              cond2dec=False, cond2lat=False, nconds=0, n_enc=0, n_dec=0, capturing=False, compact_fwd=False,
              compact_kv=False, compact_enc_kv=False) -> RowMaps:
    """Which row maps a caller builds -- the one owner of the three compaction shortcuts:
      enc_keys  the visible rows of the encoder's key-padding mask  -> encoder self-attention K | V on those rows;
      dec_keys  the visible rows of the decoder's memory            -> cross-attention K | V on those rows;
      live      the decoder rows that reach the loss (loss_rows)    -> decoder forward and backward on those rows.
    Pure: no launch, no environment.  T: target rows (without the condition rows of cond2dec); Le: rows of the encoder
    memory; mask_shape: shape of the key-padding mask, None when there is none on the device; loss_rows, trg_mask:
    whether the caller has them; the switches and `capturing` are RowPlan.launch's reads of COMPACT_* and the stream.
    Each caller keeps the rules it had before the planner:
      - under stream capture nothing is built (the maps' row counts would be baked into the graph);
      - the model forward builds nothing with get_attn, and needs the reference's [B, 1, Le] mask;
      - a decoder on its own (and prefill) compacts the memory keys with get_attn too, and needs B * Le mask elements;
      - only the model forward maps the encoder's keys; the encoder on its own builds nothing;
      - the live rows need loss_rows and a target mask, no cond2dec, no get_attn, and every attention of the trunk
        within the direct kernels' key limit (ops.ATTN_DIRECT_MAX_KEYS: the forward over compact query rows)."""
    c2d = cond2dec and nconds > 0
    nc_lat = nconds if (not c2d and cond2lat and nconds > 0) else 0
    Td, Lk = T + (nconds if c2d else 0), Le + nc_lat
    none = RowMaps(nc_lat=nc_lat, enc_rows=B * Le, dec_rows=B * Lk, live_rows=B * Td)
    if caller == ENCODER or capturing:
        return none
    if caller == MODEL:
        if get_attn or mask_shape is None or tuple(mask_shape) != (B, 1, Le):
            return none
        mask_ok = True
    elif caller in (DECODER, PREFILL):
        mask_ok = mask_shape is not None and math.prod(mask_shape) == B * Le
    else:
        raise ValueError(f"plan_rows: unknown caller {caller!r}")
    return none._replace(
        enc_keys=bool(caller == MODEL and compact_enc_kv and n_enc > 0),
        dec_keys=bool(mask_ok and compact_kv and n_dec > 0),
        live=bool(compact_fwd and loss_rows and trg_mask and not get_attn and not c2d and n_dec > 0
                  and Td <= ops.ATTN_DIRECT_MAX_KEYS and Lk <= ops.ATTN_DIRECT_MAX_KEYS))


class RowPlan:
    """The row maps of a forward (plan_rows decides which): launched together with ONE asynchronous read-back of their
    info records, used after finish().  The model forward launches its plan at its start -- or the trainer a step ahead,
    between a step's forward and its backward (Model/forward_propagation1.prefetch), so that the read-back completes
    while that backward runs and the next forward never waits for the device.  After finish():
      enc_keys  ops.KeyRows of the encoder's key-padding mask, or None
      dec_keys  ops.KeyRows of the decoder's memory mask, or None
      live      ops.LiveRows of the rows that reach the loss, or None: the decoder returns these rows COMPACT and the
                caller scatters them (ScatterRowsFn)
    A map the read-back shows to be unusable (usable_keys / usable_live) is None too."""

    def __init__(self, ek=None, dk=None, lr=None, rows=(0, 0, 0)):
        self._maps, self._rows = (ek, dk, lr), rows
        self._pending = ops.PendingReadBack(ek, dk, lr)          # ONE read-back for all three
        self._usable = None
        self.enc_keys = self.dec_keys = self.live = None

    @staticmethod
    def usable_keys(h, rows):
        """A KeyRows map (host info record h, over `rows` rows) pays and is exact: every sample's visible keys are a
        prefix, none is empty, and some -- not more than COMPACT_MAX_FRACTION -- remain."""
        return h["nonprefix"] == 0 and h["empty"] == 0 and 0 < h["padded"] <= COMPACT_MAX_FRACTION * rows

    @staticmethod
    def usable_live(h, rows):
        """A LiveRows map: no live query sees a dead row, the live rows are a prefix, and the compaction pays."""
        return h["violations"] == 0 and h["nonprefix"] == 0 and 0 < h["padded"] <= COMPACT_MAX_FRACTION * rows

    @classmethod
    def launch(cls, caller, dec=None, src_mask=None, trg_mask=None, loss_rows=None, B=0, T=0, Le=0, n_enc=0):
        """Launch what plan_rows(caller, ...) asks for.  dec: the decoder whose flags and layers count; src_mask /
        trg_mask: the masks as the trunks get them; loss_rows: bool / uint8 [B, T] or None; n_enc: encoder layers."""
        shape = None if (src_mask is None or not src_mask.is_cuda) else tuple(src_mask.shape)
        want = plan_rows(caller, B, T, Le, shape, loss_rows=loss_rows is not None, trg_mask=trg_mask is not None,
                         get_attn=getattr(dec, "get_attn", False), cond2dec=getattr(dec, "use_cond2dec", False),
                         cond2lat=getattr(dec, "use_cond2lat", False), nconds=getattr(dec, "nconds", 0), n_enc=n_enc,
                         n_dec=0 if dec is None else len(dec.layers), capturing=torch.cuda.is_current_stream_capturing(),
                         compact_fwd=COMPACT_FWD, compact_kv=COMPACT_KV, compact_enc_kv=COMPACT_ENC_KV)
        if not (want.enc_keys or want.dec_keys or want.live):
            return cls()
        ek = dk = lr = None
        if want.enc_keys or want.dec_keys:
            sm = ops.to_mask_u8(src_mask).view(B, Le)
            if want.enc_keys:
                ek = ops.KeyRows(sm, B, Le)
            if want.dec_keys and want.nc_lat > 0:
                ones = torch.ones(B, want.nc_lat, dtype=torch.uint8, device=sm.device)
                dk = ops.KeyRows(torch.cat([ones, sm], dim=1).contiguous(), B, Le + want.nc_lat)
            elif want.dec_keys:
                dk = ek if ek is not None else ops.KeyRows(sm, B, Le)   # the same mask: one map serves both trunks
        if want.live:                                    # (never with cond2dec: T is all the decoder's rows)
            lr = ops.LiveRows.from_rows(loss_rows.to(torch.uint8).contiguous().reshape(B, T), B, T,
                                        ops.to_mask_u8(trg_mask))
        return cls(ek, dk, lr, (want.enc_rows, want.dec_rows, want.live_rows))

    def finish(self) -> "RowPlan":
        """Wait for the read-back (once) and keep the usable maps.  Under stream capture the live map is left out (the
        decoder then runs on every row) and the key maps are kept."""
        if self._usable is None:
            self._pending.finish()                       # the forward's ONE host synchronisation
            (ek, dk, lr), (re, rd, rt) = self._maps, self._rows
            self._usable = (ek if ek is not None and self.usable_keys(ek.host(), re) else None,
                            dk if dk is not None and self.usable_keys(dk.host(), rd) else None,
                            lr if lr is not None and self.usable_live(lr.host(), rt) else None)
            if self._usable[2] is not None:
                self._usable[2].fwd = True
        self.enc_keys, self.dec_keys, self.live = self._usable
        if self.live is not None and torch.cuda.is_current_stream_capturing():
            self.live = None
        return self


def next_seed() -> int:
    """Fresh 64-bit dropout/eps seed per trunk call, derived from torch.manual_seed()."""
    if _SEED["base"] != torch.initial_seed():
        _SEED["base"] = torch.initial_seed()
        _SEED["ctr"] = 0
    _SEED["ctr"] += 1
    return (_SEED["base"] * 0x9E3779B97F4A7C15 + _SEED["ctr"] * 0xD1B54A32D192ED03) & ((1 << 64) - 1)


class Run:
    """Per-call dropout context: probability, seed and a site counter (every dropout
    application in the trunk gets its own Philox stream)."""

    def __init__(self, p: float, training: bool):
        self.p = float(p) if training else 0.0
        self.seed = next_seed() if self.p > 0 else 0
        self._site = 0
        # decoder backward only: (list, count) of the 32-row token tiles whose incoming gradient is not
        # identically zero -- the weight-gradient GEMMs over decoder rows reduce over these tiles only
        self.kt = None

    def site(self) -> int:
        self._site += 1
        return self._site


class GradSink:
    """Where parameter gradients are written.  Parameters of a flattened model carry
    `_gct_gview` (a view into the model's flat gradient buffer); the kernels write straight
    into it and autograd adopts the view as .grad (zero copies).  If .grad already aliases
    that view (no zero_grad(set_to_none=True) since the last backward), or the slot has already been handed
    to another Function of the same backward pass (model used twice in one graph: flat.HANDED_SLOTS), a
    temporary is used so accumulation semantics stay correct."""

    def __init__(self):
        self.out = {}

    def __call__(self, p: torch.nn.Parameter) -> torch.Tensor:
        t = self.out.get(p)
        if t is None:
            v = getattr(p, "_gct_gview", None)
            if v is not None and id(p) not in HANDED_SLOTS and \
                    (p.grad is None or p.grad.data_ptr() != v.data_ptr()):
                # a FRESH view object: AccumulateGrad only adopts (instead of cloning) a
                # gradient tensor nobody else holds a reference to
                t = v.view(v.shape)
                HANDED_SLOTS.add(id(p))
            else:
                t = torch.empty_like(p)
            self.out[p] = t
        return t

    def collect(self, params):
        ops.join_side()      # weight gradients were produced on the side stream (ops.linear_wgrad)
        return tuple(self.out.get(p) for p in params)


def _empty(rows, cols, like):
    return torch.empty(rows, cols, dtype=torch.float32, device=like.device)


# ------------------------------------------------- what a forward saves for its backward
class MhaSaved(NamedTuple):
    xq: torch.Tensor                     # query-side input [B*Lq, d] (compact rows under a live forward)
    xkv: torch.Tensor                    # key-side input: xq itself, the memory, or the gathered visible rows
    qb: torch.Tensor                     # q [Mq, d], or the fused q | k | v [Mq, 3d] when kvb is None
    kvb: Optional[torch.Tensor]          # k | v [Mk, 2d]; None: self-attention through the fused buffer
    o: torch.Tensor                      # attention output, before the output projection
    lse: torch.Tensor
    mask_u8: object                      # the mask as the attention kernels got it
    B: int
    Lq: int
    Lk: int
    site_p: int                          # dropout site of the attention probabilities
    site_o: int                          # dropout site of the output projection
    fused: bool                          # the output projection fused resid + dropout(.)
    keys: object                         # ops.KeyRows the K / V rows were compacted with, or None
    self_split: bool                     # self-attention whose K | V ran on the visible rows of xq only

    @property
    def qkv(self) -> torch.Tensor:
        assert self.kvb is None, "no fused q | k | v buffer: K | V were projected on their own"
        return self.qb


class FfnSaved(NamedTuple):
    x: torch.Tensor
    gelu_d: torch.Tensor                 # gelu'(pre-activation) where kept, 0 where dropped
    hdn: torch.Tensor                    # dropout(gelu(.)), the input of linear_2
    site_h: int                          # dropout site of the hidden activation
    site_o: int                          # dropout site of the output
    fused: bool                          # linear_2 fused resid + dropout(.)


class EncLayerSaved(NamedTuple):
    x_in: torch.Tensor
    m1: torch.Tensor                     # mean / rstd of norm_1(x_in)
    r1: torch.Tensor
    attn: MhaSaved
    a: torch.Tensor                      # n1 + dropout(attn(n1))
    m2: torch.Tensor                     # mean / rstd of norm_2(a)
    r2: torch.Tensor
    ffn: FfnSaved


class DecLayerSaved(NamedTuple):
    x: torch.Tensor
    m1: torch.Tensor                     # mean / rstd of norm_1(x)
    r1: torch.Tensor
    attn_1: MhaSaved                     # self-attention
    xa: torch.Tensor                     # x + dropout(attn_1(.))
    m2: torch.Tensor
    r2: torch.Tensor
    attn_2: MhaSaved                     # cross-attention over the encoder memory
    xb: torch.Tensor                     # xa + dropout(attn_2(.))
    m3: torch.Tensor
    r3: torch.Tensor
    ffn: FfnSaved


class EncoderSaved(NamedTuple):
    src: torch.Tensor
    econds: Optional[torch.Tensor]
    site_pe: int                         # dropout site of the embedding
    layers: List[EncLayerSaved]
    x_last: torch.Tensor                 # the last layer's output, input of the final Norm
    mean: torch.Tensor
    rstd: torch.Tensor
    B: int
    L: int


class DecoderSaved(NamedTuple):
    trg: torch.Tensor
    z2: torch.Tensor                     # z as [B*Le, latent]
    dconds: Optional[torch.Tensor]
    site_pe: int
    layers: List[DecLayerSaved]
    x_last: torch.Tensor
    mean: torch.Tensor
    rstd: torch.Tensor
    B: int
    T: int                               # decoder rows per sample, condition rows of cond2dec included
    Le: int
    Lk: int                              # memory rows per sample: Le + the condition rows of cond2lat
    c2d: bool
    c2l: bool
    trg_mask_u8: Optional[torch.Tensor]  # unpacked: the backward's ops.LiveRows checks its rows against it
    keys: object                         # plan.dec_keys of the forward
    live: object                         # plan.live of the forward: the trunk ran on these compact rows
    fold: object = None                  # ops.KvFold: the cross-attention K | V came from the rows of z (attn_2.xkv)


# ------------------------------------------------------------------------------------- MHA
def mha_fwd(run: Run, m, xq, xkv, B, Lq, Lk, mask_u8, resid, want_probs=False, keys=None, live=None, fold=None):
    """m: MultiHeadAttention module (q_linear, k_linear, v_linear, out).  xq [B*Lq,d],
    xkv [B*Lk,d] (the same tensor object for self-attention).  With `resid` the output
    projection fuses  resid + dropout(.)  (the layer's dropout_k + residual add).
    live (ops.LiveRows with .fwd): xq / resid / the result hold the compact query rows only (and xkv too for
    self-attention: the live rows of a sample are a prefix, so they are also the only keys a live query can see).
    fold ((ops.KvFold, layer), cross-attention only): xkv holds the rows of the latent z instead of the memory, and
    K | V are its image under the folded weights of that layer."""
    d, H = m.d_model, m.h
    dk = d // H
    self_attn = xkv is xq
    Mq = xq.shape[0]
    # Self-attention under a key-padding mask (the encoder): the K / V projections of masked rows are never read and
    # their dK / dV are exactly zero, so K | V run on the VISIBLE rows only (keys: ops.KeyRows of the mask; 56 % fewer
    # rows at MOSES-like lengths) while Q -- every row's output feeds the KL term -- runs on all of them.  From here on
    # it is the cross-attention path with xkv = the gathered visible rows of xq.
    self_split = self_attn and keys is not None and live is None and not want_probs
    if self_split:
        xkv = keys.gather(xq)
    if self_attn and not self_split:
        qkv = _empty(Mq, 3 * d, xq)
        ops.linear_fwd(xq, [m.q_linear.weight, m.k_linear.weight, m.v_linear.weight],
                       [m.q_linear.bias, m.k_linear.bias, m.v_linear.bias],
                       [qkv, qkv[:, d:], qkv[:, 2 * d:]], 3 * d)
        q, k, v, ldq, ldkv = qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, 3 * d
        qb, kvb = qkv, None
        if live is not None:
            keys = live                                 # K / V rows of sample b: cstart[b] .. + n_b[b]
    else:
        qb = _empty(Mq, d, xq)
        ops.linear_fwd(xq, [m.q_linear.weight], [m.q_linear.bias], [qb], d)
        # keys (ops.KeyRows): xkv holds the VISIBLE rows of the encoder memory only (quad-compacted)
        kvb = _empty(B * Lk, 2 * d, xkv) if keys is None else keys.empty(2 * d)
        if fold is not None:
            fold[0].fwd(fold[1], xkv, [kvb, kvb[:, d:]], 2 * d)
        else:
            ops.linear_fwd(xkv, [m.k_linear.weight, m.v_linear.weight],
                           [m.k_linear.bias, m.v_linear.bias], [kvb, kvb[:, d:]], 2 * d)
        q, k, v, ldq, ldkv = qb, kvb, kvb[:, d:], d, 2 * d
    site_p = run.site()
    o, lse, probs = ops.attn_fwd(q, k, v, ldq, ldkv, ldkv, mask_u8, B, H, Lq, Lk, dk, run.p,
                                 run.seed, site_p, want_probs=want_probs, keys=keys, live=live)
    y = _empty(Mq, d, xq)
    site_o = run.site()
    if resid is not None:
        ops.linear_fwd(o, [m.out.weight], [m.out.bias], [y], d, epi=ops.EPI_DROP_RESID,
                       resid=resid, p=run.p, seed=run.seed, site=site_o, live=live)
    else:
        ops.linear_fwd(o, [m.out.weight], [m.out.bias], [y], d)
    saved = MhaSaved(xq, xkv, qb, kvb, o, lse, mask_u8, B, Lq, Lk, site_p, site_o, resid is not None,
                     None if (self_attn and live is not None) else keys, self_split)
    return y, saved, probs


def mha_bwd(run: Run, m, sv: MhaSaved, dy, G: GradSink, dxq_out, depi_q, dxkv_out=None,
            depi_kv=ops.DEPI_STORE, live=None, gdrop=None, fold=None):
    """dy: gradient w.r.t. the block output (resid + dropout(out(o)) or out(o)); gdrop: dropout_bwd(dy) already
    computed by the producer of dy (ops.norm_bwd(drop=...)).
    Writes dW/db through G, d(xq) into dxq_out (epilogue depi_q) and, for cross-attention,
    d(xkv) into dxkv_out (epilogue depi_kv).  The identity path to `resid` is the caller's.
    live (ops.LiveRows): the QUERY-side rows (dy, dxq_out) are quad-compacted; saved forward tensors are
    gathered on the way in, key/value-side gradients of cross-attention stay in the encoder's row space.
    fold ((ops.KvFold, layer)): sv.xkv holds rows of the latent z; dxkv_out (nullable) is d(those rows), and the
    gradients of k_linear / v_linear are the caller's (KvFold.wgrad_layer, after the layer's slab reductions)."""
    B, Lq, Lk, keys = sv.B, sv.Lq, sv.Lk, sv.keys
    d, H = m.d_model, m.h
    dk = d // H
    Mq, Mk = B * Lq, sv.xkv.shape[0]
    kt = run.kt
    new = lambda cols: _empty(Mq, cols, dy)                                      # noqa: E731
    if live is not None:
        Mq, kt = live.Mc, None
        # rows of a live quad that belong to no sample's live prefix are never written by the attention kernel
        new = live.empty_zero_gaps
        # (a forward that ran on the compact rows saved compact activations: nothing to gather)
        o_in, xq_in = (sv.o, sv.xq) if live.fwd else (live.gather(sv.o), live.gather(sv.xq))
    else:
        o_in, xq_in = sv.o, sv.xq
    if gdrop is not None:
        g = gdrop
    else:
        g = ops.dropout_bwd(dy, run.p, run.seed, sv.site_o, live=live) if (sv.fused and run.p > 0) else dy
    do = _empty(Mq, d, dy) if live is None else live.empty(d)
    ops.linear_bwd([g], d, o_in, [m.out.weight], [G(m.out.weight)], [G(m.out.bias)], do, kt=kt, M=Mq)
    if sv.kvb is None:  # self-attention: fused [q|k|v]
        dqkv = new(3 * d)
        fwdc = live is not None and live.fwd             # q | k | v and o are compact too: address K / V like dK / dV
        ops.attn_bwd(sv.qb, sv.qb[:, d:], sv.qb[:, 2 * d:], 3 * d, 3 * d, 3 * d, sv.mask_u8, sv.o, do, sv.lse, dqkv,
                     dqkv[:, d:], dqkv[:, 2 * d:], 3 * d, 3 * d, 3 * d, B, H, Lq, Lk, dk, run.p,
                     run.seed, sv.site_p, live=live, kv_compact=live is not None and not fwdc,
                     keys=live if fwdc else None)
        segs = [dqkv, dqkv[:, d:], dqkv[:, 2 * d:]]
        ops.linear_bwd(segs, 3 * d, xq_in, [m.q_linear.weight, m.k_linear.weight, m.v_linear.weight],
                       [G(m.q_linear.weight), G(m.k_linear.weight), G(m.v_linear.weight)],
                       [G(m.q_linear.bias), G(m.k_linear.bias), G(m.v_linear.bias)], dxq_out, depi=depi_q, kt=kt, M=Mq)
    else:
        dq = new(d)
        if keys is None:
            dkv = _empty(Mk, 2 * d, dy)
        else:      # compacted keys: the rows that pad a quad belong to no sample and are never written
            dkv = keys.empty_zero_gaps(2 * d)
        ops.attn_bwd(sv.qb, sv.kvb, sv.kvb[:, d:], d, 2 * d, 2 * d, sv.mask_u8, sv.o, do, sv.lse, dq, dkv, dkv[:, d:],
                     d, 2 * d, 2 * d, B, H, Lq, Lk, dk, run.p, run.seed, sv.site_p, live=live, keys=keys)
        ops.linear_bwd([dq], d, xq_in, [m.q_linear.weight], [G(m.q_linear.weight)], [G(m.q_linear.bias)], dxq_out,
                       depi=depi_q, kt=kt, M=Mq)                                          # query rows
        if fold is not None:
            fold[0].bwd(fold[1], [dkv, dkv[:, d:]], 2 * d, sv.xkv, dxkv_out, depi_kv, Mk)
            return
        kv_w = [m.k_linear.weight, m.v_linear.weight]
        kv_g = ([G(m.k_linear.weight), G(m.v_linear.weight)], [G(m.k_linear.bias), G(m.v_linear.bias)])
        if sv.self_split:    # K | V came from the visible rows of xq itself: their input gradient goes back into d(xq)
            dxk = keys.empty(d)
            ops.linear_bwd([dkv, dkv[:, d:]], 2 * d, sv.xkv, kv_w, *kv_g, dxk, M=Mk)
            keys.scatter_add(dxk, dxq_out)
        elif dxkv_out is not None:
            ops.linear_bwd([dkv, dkv[:, d:]], 2 * d, sv.xkv, kv_w, *kv_g, dxkv_out, depi=depi_kv, M=Mk)
        else:
            ops.linear_wgrad([dkv, dkv[:, d:]], 2 * d, sv.xkv, *kv_g)


# ------------------------------------------------------------------------------------- FFN
def ffn_fwd(run: Run, ff, x, resid, live=None):
    M, d = x.shape
    dff = ff.linear_1.weight.shape[0]
    gelu_d = _empty(M, dff, x)     # the backward's elementwise factor: gelu'(pre-activation) where kept, 0 where dropped
    hdn = _empty(M, dff, x)
    site_h = run.site()
    ops.linear_fwd(x, [ff.linear_1.weight], [ff.linear_1.bias], [hdn], dff, epi=ops.EPI_GELU_DROP_SAVE,
                   pre=gelu_d, p=run.p, seed=run.seed, site=site_h, live=live)
    y = _empty(M, d, x)
    site_o = run.site()
    if resid is not None:
        ops.linear_fwd(hdn, [ff.linear_2.weight], [ff.linear_2.bias], [y], d,
                       epi=ops.EPI_DROP_RESID, resid=resid, p=run.p, seed=run.seed, site=site_o, live=live)
    else:
        ops.linear_fwd(hdn, [ff.linear_2.weight], [ff.linear_2.bias], [y], d)
    return y, FfnSaved(x, gelu_d, hdn, site_h, site_o, resid is not None)


def ffn_bwd(run: Run, ff, sv: FfnSaved, dy, G: GradSink, dx_out, depi, live=None, gdrop=None):
    x, gelu_d, hdn = sv.x, sv.gelu_d, sv.hdn
    M, d = x.shape
    dff = gelu_d.shape[1]
    kt = run.kt
    if live is not None:          # quad-compacted rows: gather what the forward saved
        M, kt = live.Mc, None
        if not live.fwd:                              # (a compact forward saved compact x / gelu_d / hdn)
            x, hdn = live.gather(x), live.gather(hdn)     # (gelu_d stays in place: the dgrad epilogue reads it
                                                          #  through the quad map)
    if gdrop is not None:
        g = gdrop
    else:
        g = ops.dropout_bwd(dy, run.p, run.seed, sv.site_o, live=live) if (sv.fused and run.p > 0) else dy
    dpre = _empty(M, dff, dy) if live is None else live.empty(dff)
    ops.linear_bwd([g], d, hdn, [ff.linear_2.weight], [G(ff.linear_2.weight)], [G(ff.linear_2.bias)], dpre,
                   depi=ops.DEPI_MUL_SAVED, pre=gelu_d, p=run.p, seed=run.seed, site=sv.site_h, kt=kt, live=live,
                   pre_full=live is not None and not live.fwd, M=M)
    ops.linear_bwd([dpre], dff, x, [ff.linear_1.weight], [G(ff.linear_1.weight)], [G(ff.linear_1.bias)], dx_out,
                   depi=depi, kt=kt, M=M)


# ---------------------------------------------------------------------------------- layers
def enc_layer_fwd(run: Run, layer, x_in, B, L, mask_u8, want_probs=False, keys=None):
    n1, m1, r1 = ops.norm_fwd(x_in, layer.norm_1.alpha, layer.norm_1.bias, layer.norm_1.eps)
    a, sv_a, probs = mha_fwd(run, layer.attn, n1, n1, B, L, L, mask_u8, n1, want_probs, keys=keys)
    n2, m2, r2 = ops.norm_fwd(a, layer.norm_2.alpha, layer.norm_2.bias, layer.norm_2.eps)
    out, sv_f = ffn_fwd(run, layer.ff, n2, n2)
    return out, EncLayerSaved(x_in, m1, r1, sv_a, a, m2, r2, sv_f), probs


def _mha_drop(run: Run, sv: MhaSaved, buf):
    """ops.norm_bwd(drop=...) request for the attention block saved in sv: the Norm backward that produces the
    gradient of that block's output also writes dropout_bwd of it (the block's own first step) into buf."""
    return (buf, run.p, run.seed, sv.site_o) if (buf is not None and sv.fused and run.p > 0) else None


def _ffn_drop(run: Run, sv: Optional[FfnSaved], buf):
    return (buf, run.p, run.seed, sv.site_o) if (buf is not None and sv is not None and sv.fused and run.p > 0) else None


def enc_layer_bwd(run: Run, layer, sv: EncLayerSaved, g, G: GradSink, gd=None, gdbuf=None, below=None):
    """g: mutable [M,d] gradient buffer w.r.t. the layer output; returns d(x_in) in g.
    gd: dropout_bwd(g) for this layer's FFN if the caller's Norm backward already produced it; gdbuf: scratch
    [M,d] for the fused dropout_bwd outputs; below: saved FFN state of the layer underneath (its dropout_bwd is
    written by this layer's last Norm backward) -- returns (g, that buffer or None)."""
    with ops.deferred_reductions():      # the layer's 6 weight / bias / Norm slab reductions: one launch at the end
        # out = n2 + drop(ffn(n2))  =>  d(n2) = g + ffn'(g): the W1 dgrad accumulates into g
        ffn_bwd(run, layer.ff, sv.ffn, g, G, g, ops.DEPI_ACCUM, gdrop=gd)
        dr = _mha_drop(run, sv.attn, gdbuf)
        ops.norm_bwd(g, sv.a, layer.norm_2.alpha, sv.m2, sv.r2, G(layer.norm_2.alpha), G(layer.norm_2.bias),
                     out=g, eps=layer.norm_2.eps, drop=dr)
        # a = n1 + drop(attn(n1))
        mha_bwd(run, layer.attn, sv.attn, g, G, g, ops.DEPI_ACCUM, gdrop=None if dr is None else gdbuf)
        dr = _ffn_drop(run, below, gdbuf)
        ops.norm_bwd(g, sv.x_in, layer.norm_1.alpha, sv.m1, sv.r1, G(layer.norm_1.alpha), G(layer.norm_1.bias),
                     out=g, eps=layer.norm_1.eps, drop=dr)
    _grads_done(layer, G)
    return g, (None if dr is None else gdbuf)


def dec_layer_fwd(run: Run, layer, x, e, B, T, Lk, src_mask_u8, trg_mask_u8, want_probs=False, keys=None, live=None,
                  fold=None):
    """live (ops.LiveRows with .fwd): x and everything row-wise of this layer hold the compact live rows only.
    fold ((ops.KvFold, layer)): e holds the rows of the latent z (mha_fwd)."""
    x2, m1, r1 = ops.norm_fwd(x, layer.norm_1.alpha, layer.norm_1.bias, layer.norm_1.eps)
    xa, sa1, p1 = mha_fwd(run, layer.attn_1, x2, x2, B, T, T, trg_mask_u8, x, want_probs, live=live)
    x2, m2, r2 = ops.norm_fwd(xa, layer.norm_2.alpha, layer.norm_2.bias, layer.norm_2.eps)
    xb, sa2, p2 = mha_fwd(run, layer.attn_2, x2, e, B, T, Lk, src_mask_u8, xa, want_probs, keys=keys, live=live,
                          fold=fold)
    x2, m3, r3 = ops.norm_fwd(xb, layer.norm_3.alpha, layer.norm_3.bias, layer.norm_3.eps)
    xc, sf = ffn_fwd(run, layer.ff, x2, xb, live=live)
    return xc, DecLayerSaved(x, m1, r1, sa1, xa, m2, r2, sa2, xb, m3, r3, sf), p1, p2


def dec_layer_bwd(run: Run, layer, sv: DecLayerSaved, g, de, first_de, G: GradSink, live=None, gd=None, gdbuf=None,
                  below=None, fold=None):
    """live (ops.LiveRows): g and every row-wise gradient of this layer are quad-compacted [live.Mc, d].
    fold ((ops.KvFold, layer)): de (nullable) is the gradient of the rows of z, not of the memory.
    gd / gdbuf / below as in enc_layer_bwd; returns (g, dropout_bwd(g) for the FFN of the layer underneath or None)."""
    t = torch.empty_like(g) if live is None else live.empty(g.shape[1])
    with ops.deferred_reductions():      # the layer's 9 weight / bias / Norm slab reductions: one launch at the end
        ffn_bwd(run, layer.ff, sv.ffn, g, G, t, ops.DEPI_STORE, live=live, gdrop=gd)
        dr = _mha_drop(run, sv.attn_2, gdbuf)
        ops.norm_bwd(t, sv.xb, layer.norm_3.alpha, sv.m3, sv.r3, G(layer.norm_3.alpha), G(layer.norm_3.bias),
                     dres=g, out=g, eps=layer.norm_3.eps, live=live, drop=dr)
        mha_bwd(run, layer.attn_2, sv.attn_2, g, G, t, ops.DEPI_STORE, de,
                ops.DEPI_STORE if first_de else ops.DEPI_ACCUM, live=live, gdrop=None if dr is None else gdbuf,
                fold=fold)
        dr = _mha_drop(run, sv.attn_1, gdbuf)
        ops.norm_bwd(t, sv.xa, layer.norm_2.alpha, sv.m2, sv.r2, G(layer.norm_2.alpha), G(layer.norm_2.bias),
                     dres=g, out=g, eps=layer.norm_2.eps, live=live, drop=dr)
        mha_bwd(run, layer.attn_1, sv.attn_1, g, G, t, ops.DEPI_STORE, live=live, gdrop=None if dr is None else gdbuf)
        dr = _ffn_drop(run, below, gdbuf)
        ops.norm_bwd(t, sv.x, layer.norm_1.alpha, sv.m1, sv.r1, G(layer.norm_1.alpha), G(layer.norm_1.bias),
                     dres=g, out=g, eps=layer.norm_1.eps, live=live, drop=dr)
    if fold is not None:                 # P_l and s_l are final now: the gradients of k_linear | v_linear from them
        a2 = layer.attn_2
        fold[0].wgrad_layer(fold[1], G(a2.k_linear.weight), G(a2.v_linear.weight), G(a2.k_linear.bias),
                            G(a2.v_linear.bias))
    _grads_done(layer, G)
    return g, (None if dr is None else gdbuf)


# ---------------------------------------------------------------------------------- trunks
def _pe2d(pe_mod, L):
    pe = pe_mod.pe
    if L > pe.shape[1]:
        raise ValueError(f"sequence length {L} exceeds the positional table ({pe.shape[1]})")
    return pe[0]


def encoder_trunk_fwd(enc, run: Run, src, mask_u8, econds, want_probs, plan: RowPlan):
    """Model/vaetf.py:32-54 (up to the final Norm).  Returns x [B, n_c+S, d] and saved state.
    plan.enc_keys (ops.KeyRows of the key-padding mask): the K | V projections of every layer run on the visible rows
    only (mha_fwd)."""
    keys = plan.enc_keys
    B, S = src.shape
    d, nc = enc.d_model, enc.nconds
    cond = None
    if nc > 0:
        if econds is None:
            raise ValueError("econds required when nconds > 0")          # vaetf.py:36
        cond = ops.small_linear_fwd(econds.contiguous(), enc.embed_cond2enc.weight,
                                    enc.embed_cond2enc.bias)
    L = S + nc
    mask_u8 = ops.pack_mask(mask_u8, B, L, L)           # bits: once per call, shared by all layers / heads / backward
    site_pe = run.site()
    x = ops.embed_pe_fwd(src, enc.embed_sentence.embed.weight, cond, _pe2d(enc.pe, L), nc,
                         math.sqrt(d), run.p, run.seed, site_pe)
    layers, probs = [], []
    for layer in enc.layers:
        x, sv, pr = enc_layer_fwd(run, layer, x, B, L, mask_u8, want_probs, keys=keys)
        layers.append(sv)
        probs.append(pr)
    y, mean, rstd = ops.norm_fwd(x, enc.norm.alpha, enc.norm.bias, enc.norm.eps)
    return y.view(B, L, d), EncoderSaved(src, econds, site_pe, layers, x, mean, rstd, B, L), probs


def encoder_trunk_bwd(enc, run: Run, sv: EncoderSaved, dy, G: GradSink):
    layers, B, L = sv.layers, sv.B, sv.L
    d, nc = enc.d_model, enc.nconds
    g = dy.reshape(B * L, d).clone()
    # every Norm backward also writes dropout_bwd of its result for the sub-layer that consumes it next (gdbuf)
    gdbuf = torch.empty_like(g) if (run.p > 0 and len(layers) > 0) else None
    dr = _ffn_drop(run, layers[-1].ffn if layers else None, gdbuf)
    ops.norm_bwd(g, sv.x_last, enc.norm.alpha, sv.mean, sv.rstd, G(enc.norm.alpha), G(enc.norm.bias), out=g,
                 eps=enc.norm.eps, drop=dr)
    gd = None if dr is None else gdbuf
    for i in range(len(layers) - 1, -1, -1):
        g, gd = enc_layer_bwd(run, enc.layers[i], layers[i], g, G, gd=gd, gdbuf=gdbuf,
                              below=layers[i - 1].ffn if i > 0 else None)
    dcond = torch.empty(B, nc * d, dtype=torch.float32, device=g.device) if nc > 0 else None
    ops.embed_pe_bwd(g, sv.src, G(enc.embed_sentence.embed.weight), dcond, nc, math.sqrt(d), run.p,
                     run.seed, sv.site_pe)
    if nc > 0:
        ops.small_linear_bwd(dcond, sv.econds.contiguous(), G(enc.embed_cond2enc.weight),
                             G(enc.embed_cond2enc.bias))


def decoder_trunk_fwd(dec, run: Run, trg, z, src_mask_u8, trg_mask_u8, dconds, want_probs, plan: RowPlan):
    """Model/vaetf.py:79-114.  z [B, L_e, latent].  The trunk takes the shortcuts of `plan` (RowPlan, finished):
      dec_keys  the visible rows of the encoder memory: padded rows are masked keys of every cross-attention, their
                K / V projections are never used and their dK / dV are zero, so the six K|V GEMMs, their weight
                gradients and the gradient w.r.t. the memory run on the visible rows only (quad-compacted, ops.KeyRows);
      live      the decoder rows whose output reaches the loss (the reference's cross-entropy ignores the rows of padded
                targets, Train/trainer1.py:21-22: 56 % of the rows at MOSES-like lengths).  A row outside the set
                influences a row inside it only as a KEY of self-attention, and the map was checked on the device
                against this call's trg_mask (no live query sees a dead row), so the whole trunk runs on the quad-
                compacted live rows: every GEMM, Norm and attention launch sees ~half the rows, every dropout site draws
                the bits of the original coordinates, the backward finds its activations compact already.  The trunk
                then RETURNS THE COMPACT ROWS [Mc, d]; whoever scatters them back (ScatterRowsFn: Decoder.forward for a
                caller of the decoder alone, Vaetf / Cvaetf.forward behind the vocabulary head) produces zeros on the
                skipped rows -- or, for the few padded rows that share an aligned group of four rows with a live one,
                finite values without meaning -- not the reference's values (nothing downstream of an ignore_index loss
                reads them), and reports a gradient that arrives on a skipped row as an error (ops.LiveRows.check_grad)."""
    B, T0 = trg.shape
    d, nc = dec.d_model, dec.nconds
    Le, lat = z.shape[1], z.shape[2]
    z2 = z.reshape(B * Le, lat)
    c2d = dec.use_cond2dec and nc > 0
    c2l = (not c2d) and dec.use_cond2lat and nc > 0
    cond_x = None
    if c2d:
        cond_x = ops.small_linear_fwd(dconds.contiguous(), dec.embed_cond2dec.weight,
                                      dec.embed_cond2dec.bias)
    T = T0 + (nc if c2d else 0)
    site_pe = run.site()
    x = ops.embed_pe_fwd(trg, dec.embed.embed.weight, cond_x, _pe2d(dec.pe, T), nc if c2d else 0,
                         math.sqrt(d), run.p, run.seed, site_pe)
    # Without cond2lat rows the memory e = fc_z(z) feeds nothing but the K | V projections of the layers: they run on
    # the rows of z itself, through weights folded once per call (ops.KvFold), and e is never formed
    kv = [(layer.attn_2.k_linear, layer.attn_2.v_linear) for layer in dec.layers]
    fold = ops.KvFold(kv, dec.fc_z) if (KV_FOLD and not c2l and ops.KvFold.usable(kv, dec.fc_z)) else None
    Lk = Le
    e = z2
    if fold is None:
        e = ez = _empty(B * Le, d, z2)
        ops.linear_fwd(z2, [dec.fc_z.weight], [dec.fc_z.bias], [ez], d)
    if c2l:
        Lk = Le + nc
        cl = ops.small_linear_fwd(dconds.contiguous(), dec.embed_cond2lat.weight,
                                  dec.embed_cond2lat.bias)                     # [B, nc*d]
        e = _empty(B * Lk, d, z2)
        ops.copy_rows(cl, nc, 0, e, Lk, 0, B * nc, nc, d)
        ops.copy_rows(ez, Le, 0, e, Lk, nc, B * Le, Le, d)
        if src_mask_u8 is not None:                                            # vaetf.py:95-98
            ones = torch.ones(B, nc, dtype=torch.uint8, device=src_mask_u8.device)
            src_mask_u8 = torch.cat([ones, src_mask_u8.view(B, Le)], dim=1).contiguous()
    layers, p1s, p2s = [], [], []
    live, keys = plan.live, plan.dec_keys
    if live is not None:
        x = live.gather(x)
    if keys is not None:
        e = keys.gather(e)
    src_m = ops.pack_mask(src_mask_u8, B, T, Lk)
    trg_m = ops.pack_mask(trg_mask_u8, B, T, T)
    for i, layer in enumerate(dec.layers):
        x, sv, p1, p2 = dec_layer_fwd(run, layer, x, e, B, T, Lk, src_m, trg_m, want_probs, keys=keys, live=live,
                                      fold=None if fold is None else (fold, i))
        layers.append(sv)
        p1s.append(p1)
        p2s.append(p2)
    y, mean, rstd = ops.norm_fwd(x, dec.norm.alpha, dec.norm.bias, dec.norm.eps)
    saved = DecoderSaved(trg, z2, dconds, site_pe, layers, x, mean, rstd, B, T, Le, Lk, c2d, c2l,
                         trg_mask_u8.u8 if isinstance(trg_mask_u8, ops.MaskBits) else trg_mask_u8, keys, live, fold)
    if live is not None:
        return y, saved, p1s, p2s        # [Mc, d] COMPACT rows: the caller holds the plan and scatters what it needs
    return y.view(B, T, d), saved, p1s, p2s


def decoder_trunk_bwd(dec, run: Run, sv: DecoderSaved, dy, G: GradSink, need_dz=True):
    layers, keys, live_fwd, fold = sv.layers, sv.keys, sv.live, sv.fold
    B, T, Le, Lk = sv.B, sv.T, sv.Le, sv.Lk
    d, nc = dec.d_model, dec.nconds
    dcols = d if fold is None else sv.z2.shape[1]          # d(memory), maybe compact -- with the fold d(rows of z)
    new_de = (lambda: _empty(B * Lk, dcols, dy)) if keys is None else (lambda: keys.empty(dcols))
    # A decoder row whose incoming gradient is zero (padded target positions under the ignore_index loss: 56 % of
    # the rows at MOSES-like lengths) keeps a zero gradient through every layer below -- norm, linear, GELU and
    # dropout backward map a zero row to a zero row, attention gives zero dQ rows for zero dO rows -- PROVIDED no live
    # query attends to it (a dead row that is a visible key receives dK / dV).  ops.LiveRows derives the live rows
    # from the gradient and checks that proviso on the device against the trg_mask this call used
    # (csrc/liverows.hip).  When it holds (and pays), the whole decoder backward runs on the QUAD-COMPACTED live
    # rows: every GEMM, norm and dropout backward sees ~half the rows; otherwise the dense path runs, with the
    # weight-gradient GEMMs reducing over the live token tiles (the list names every tile when the check fails).
    live, lr = live_fwd, None
    if live_fwd is None:
        lr = ops.LiveRows(dy.reshape(B * T, d), B, T, sv.trg_mask_u8) if (COMPACT_BWD or (B * T) % 32 == 0) else None
        if COMPACT_BWD and len(dec.layers) > 0 and not torch.cuda.is_current_stream_capturing():
            live = lr if RowPlan.usable_live(lr.host(), B * T) else None       # one 32-byte read-back per step
    if live_fwd is not None:
        # the forward ran on these rows only and handed out COMPACT rows: dy arrives compact (ScatterRowsFn gathers the
        # gradient of what it scattered and reports gradient rows that fell on skipped rows)
        g = dy.reshape(live.Mc, d).clone()
    elif live is not None:
        g = live.gather(dy.reshape(B * T, d))
    else:
        g = dy.reshape(B * T, d).clone()
        run.kt = lr.kt if (lr is not None and (B * T) % 32 == 0) else None
    gdbuf = None
    if run.p > 0 and len(layers) > 0:
        gdbuf = torch.empty_like(g) if live is None else live.empty(d)
    dr = _ffn_drop(run, layers[-1].ffn if layers else None, gdbuf)
    ops.norm_bwd(g, sv.x_last, dec.norm.alpha, sv.mean, sv.rstd, G(dec.norm.alpha), G(dec.norm.bias), out=g,
                 eps=dec.norm.eps, live=live, drop=dr)
    gd = None if dr is None else gdbuf
    de = new_de() if (fold is None or need_dz) else None
    for i in range(len(layers) - 1, -1, -1):
        g, gd = dec_layer_bwd(run, dec.layers[i], layers[i], g, de, i == len(layers) - 1, G, live=live, gd=gd,
                              gdbuf=gdbuf, below=layers[i - 1].ffn if i > 0 else None,
                              fold=None if fold is None else (fold, i))
    run.kt = None
    if live is not None:
        g = live.scatter(g)                             # back to [B*T, d]: zero rows where nothing was live
    if len(dec.layers) == 0:
        de.zero_()
    if keys is not None and de is not None:
        de = keys.scatter(de)                            # back to [B*Lk, d]: masked keys get no gradient
    # embedding side
    dcx = torch.empty(B, nc * d, dtype=torch.float32, device=g.device) if sv.c2d else None
    ops.embed_pe_bwd(g, sv.trg, G(dec.embed.embed.weight), dcx, nc if sv.c2d else 0, math.sqrt(d), run.p,
                     run.seed, sv.site_pe)
    if sv.c2d:
        ops.small_linear_bwd(dcx, sv.dconds.contiguous(), G(dec.embed_cond2dec.weight),
                             G(dec.embed_cond2dec.bias))
    # memory side
    if fold is not None:                 # de is d(z) already; fc_z's gradients from the layers' P_l and s_l
        fold.finish(G(dec.fc_z.weight), G(dec.fc_z.bias))
        return de.view(B, Le, -1) if need_dz else None
    dez = de
    if sv.c2l:
        dcl = torch.empty(B, nc * d, dtype=torch.float32, device=g.device)
        ops.copy_rows(de, Lk, 0, dcl, nc, 0, B * nc, nc, d)
        ops.small_linear_bwd(dcl, sv.dconds.contiguous(), G(dec.embed_cond2lat.weight),
                             G(dec.embed_cond2lat.bias))
        dez = _empty(B * Le, d, g)
        ops.copy_rows(de, Lk, nc, dez, Le, 0, B * Le, Le, d)
    ops.linear_wgrad([dez], d, sv.z2, [G(dec.fc_z.weight)], [G(dec.fc_z.bias)])
    dz = None
    if need_dz:
        dz = _empty(B * Le, sv.z2.shape[1], g)
        ops.linear_dgrad([dez], d, B * Le, [dec.fc_z.weight], dz)
        dz = dz.view(B, Le, -1)
    return dz


# ------------------------------------------------------------------------ autograd boundary
def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, run, src, mask_u8, econds, want_probs, plan, *params):
        y, saved, probs = encoder_trunk_fwd(enc, run, src, mask_u8, econds, want_probs, plan)
        ctx.enc, ctx.run, ctx.saved, ctx.params = enc, run, saved, params
        if want_probs:
            for p in probs:
                ctx.mark_non_differentiable(p)
            return (y, *probs)
        return y

    @staticmethod
    def backward(ctx, dy, *unused):
        G = GradSink()
        encoder_trunk_bwd(ctx.enc, ctx.run, ctx.saved, _f32c(dy), G)
        ctx.saved = None
        return (None,) * 7 + G.collect(ctx.params)


class DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dec, run, trg, z, src_mask_u8, trg_mask_u8, dconds, want_probs, plan, *params):
        y, saved, p1, p2 = decoder_trunk_fwd(dec, run, trg, _f32c(z), src_mask_u8, trg_mask_u8, dconds, want_probs,
                                             plan)      # plan.live: y holds the COMPACT live rows [Mc, d]
        ctx.dec, ctx.run, ctx.saved, ctx.params = dec, run, saved, params
        ctx.need_dz = z.requires_grad
        if want_probs:
            for p in p1 + p2:
                ctx.mark_non_differentiable(p)
            return (y, *p1, *p2)
        return y

    @staticmethod
    def backward(ctx, dy, *unused):
        G = GradSink()
        dz = decoder_trunk_bwd(ctx.dec, ctx.run, ctx.saved, _f32c(dy), G, ctx.need_dz)
        ctx.saved = None
        return (None, None, None, dz, None, None, None, None, None) + G.collect(ctx.params)


class ScatterRowsFn(torch.autograd.Function):
    """Compact rows [Mc, cols] of a decoder forward that ran on the loss rows only -> all [B, T, cols] rows (zeros where
    nothing was computed).  Backward: the gradient's compact rows; gradient rows that fall on SKIPPED rows cannot be
    honoured -- they are counted on the device and raised at the next read-back (ops.LiveRows.check_grad)."""

    @staticmethod
    def forward(ctx, xc, live, B, T):
        ctx.live, ctx.shape = live, xc.shape
        return live.scatter(_f32c(xc)).view(B, T, xc.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        live = ctx.live
        g = _f32c(dy).reshape(live.M, dy.shape[-1])
        live.check_grad(g)
        return live.gather(g).view(ctx.shape), None, None, None


class SamplerFn(torch.autograd.Function):
    """mu = fc_mu(x), log_var = fc_log_var(x) as ONE segmented GEMM, then the
    reparameterisation (Model/sublayers.py:22-26, Model/cvaetf.py:55-69)."""

    @staticmethod
    def forward(ctx, x, w_mu, b_mu, w_lv, b_lv, eps, variational):
        B, L, d = x.shape
        lat = w_mu.shape[0]
        x2 = _f32c(x).view(B * L, d)
        mu = _empty(B * L, lat, x2)
        lv = _empty(B * L, lat, x2)
        ops.linear_fwd(x2, [w_mu, w_lv], [b_mu, b_lv], [mu, lv], lat)
        if variational:
            z, eps_used = ops.reparam_fwd(mu, lv, None if eps is None else _f32c(eps).view(B * L, lat),
                                          next_seed(), 0)
        else:
            z, eps_used = mu, None
        ctx.save_for_backward(x2, w_mu, w_lv, lv, eps_used if eps_used is not None else lv)
        ctx.variational = variational
        ctx.shape = (B, L, d, lat)
        ctx.params = (w_mu, b_mu, w_lv, b_lv)
        shp = (B, L, lat)
        if variational:
            return z.view(shp), mu.view(shp), lv.view(shp)
        return mu.view(shp), mu.view(shp).clone(), lv.view(shp)

    @staticmethod
    def backward(ctx, dz, dmu, dlv):
        x2, w_mu, w_lv, lv, eps = ctx.saved_tensors
        B, L, d, lat = ctx.shape
        M = B * L
        zeros = None
        def flat(t):
            return None if t is None else _f32c(t).view(M, lat)
        dz, dmu, dlv = flat(dz), flat(dmu), flat(dlv)
        gmu = _empty(M, lat, x2)
        glv = _empty(M, lat, x2)
        if ctx.variational:
            if dz is None:
                dz = torch.zeros(M, lat, dtype=torch.float32, device=x2.device)
            ops.reparam_bwd(dz, lv, eps, dmu, dlv, gmu, glv)
        else:
            z0 = torch.zeros(M, lat, dtype=torch.float32, device=x2.device)
            a = dz if dz is not None else z0
            b = dmu if dmu is not None else z0
            ops.add(a, b, out=gmu)
            glv = dlv if dlv is not None else z0
        G = GradSink()
        w_mu_p, b_mu_p, w_lv_p, b_lv_p = ctx.params
        ops.linear_wgrad([gmu, glv], lat, x2, [G(w_mu_p), G(w_lv_p)], [G(b_mu_p), G(b_lv_p)])
        dx = _empty(M, d, x2)
        ops.linear_dgrad([gmu, glv], lat, M, [w_mu, w_lv], dx)
        return (dx.view(B, L, d),) + G.collect(ctx.params) + (None, None)


class LinearFn(torch.autograd.Function):
    """y = x W^T + b on the MFMA GEMM (Model/vaetf.py:169 `out`, :172 `prop_fc`)."""

    @staticmethod
    def forward(ctx, x, w, b):
        shp = x.shape
        x2 = _f32c(x).reshape(-1, shp[-1])
        y = _empty(x2.shape[0], w.shape[0], x2)
        ops.linear_fwd(x2, [w], [b], [y], w.shape[0])
        ctx.save_for_backward(x2, w)
        ctx.params = (w, b)
        ctx.shp = shp
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        N = w.shape[0]
        dy2 = _f32c(dy).reshape(-1, N)
        G = GradSink()
        wp, bp = ctx.params
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty(x2.shape[0], x2.shape[1], x2)
            ops.linear_bwd([dy2], N, x2, [w], [G(wp)], [G(bp) if bp is not None else None], dx)
            dx = dx.view(ctx.shp)
        else:
            ops.linear_wgrad([dy2], N, x2, [G(wp)], [G(bp) if bp is not None else None])
        ops.join_side()
        return dx, G.out.get(wp), G.out.get(bp) if bp is not None else None


class CrossEntropySumFn(torch.autograd.Function):
    """Train/trainer1.py:21-22."""

    @staticmethod
    def forward(ctx, logits, target, pad_id):
        l2 = _f32c(logits).reshape(-1, logits.shape[-1])
        t = target.reshape(-1).contiguous()
        ctx.save_for_backward(l2, t)
        ctx.pad_id, ctx.shp = int(pad_id), logits.shape
        return ops.ce_fwd(l2, t, int(pad_id))

    @staticmethod
    def backward(ctx, g):
        l2, t = ctx.saved_tensors
        return ops.ce_bwd(l2, t, _f32c(g), ctx.pad_id).view(ctx.shp), None, None


def _seq_rows2d(who, what, t, ys, row_shift):
    """Logits t [n, R, V] or [n * R, V] for the token rows ys [n, W], as the seq_* kernels take them: (fp32 [n * R, V]
    with unit column stride -- t itself where it already is one --, R).  `what` names t in the message."""
    n, V = ys.shape[0], t.shape[-1]
    if t.dim() == 3:
        if t.shape[0] != n:
            raise ValueError(f"{who}: {t.shape[0]} {what} blocks for {n} token rows")
        t2 = _f32c(t).view(-1, V)
    elif t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1:
        t2 = t
    else:
        t2 = _f32c(t).reshape(-1, V)
    return t2, t2.shape[0] // n if n else ys.shape[1] - 1 + int(row_shift)


def _seq_backward(shape, l2, grads, inputs, run):
    """What a seq_* Function's backward returns for its `inputs` inputs: dlogits = run(*grads as fp32 contiguous, None
    kept) in the shape the forward got -- zeros without a launch when every gradient is None --, then None for the
    rest."""
    gs = [None if g is None else _f32c(g) for g in grads]
    dl = torch.zeros(shape, device=l2.device) if all(g is None for g in gs) else run(*gs).view(shape)
    return (dl,) + (None,) * (inputs - 1)


class SeqLogpFn(torch.autograd.Function):
    """Per-sequence log-likelihoods with a gradient (decode.score_reference / seq_logp_grad_reference state the rules):
    apply(logits, ys, prefix_lens, pad_id, row_shift) -> (logp [n], token_logp [n, W], tokens [n], hits [n]).
    logits fp32 [n, R, V] or [n * R, V] (unit column stride; R >= row_shift + W - 1 logits rows per sequence), ys int64
    [n, W], prefix_lens int32 [n] on the device or None.  tokens / hits are counts: not differentiable.  The backward
    is gct_seq_logp_bwd: it writes every row of dlogits, exact zeros where nothing is scored or the weight is 0."""

    @staticmethod
    def forward(ctx, logits, ys, prefix_lens, pad_id, row_shift):
        l2, R = _seq_rows2d("SeqLogpFn", "logits", logits, ys, row_shift)
        ys = ys.contiguous()
        tl, lp, nt, nh = ops.seq_logp(l2, ys, prefix_lens, int(pad_id), row_shift=int(row_shift), rows_per_seq=R)
        ctx.save_for_backward(l2, ys, prefix_lens)
        ctx.geom = (int(pad_id), int(row_shift), R, logits.shape)
        ctx.set_materialize_grads(False)                 # an output nobody used arrives as None, not as zeros
        ctx.mark_non_differentiable(nt, nh)
        return lp, tl, nt, nh

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logp, g_token, *unused):
        l2, ys, prefix_lens = ctx.saved_tensors
        pad_id, row_shift, R, shape = ctx.geom
        return _seq_backward(shape, l2, (g_logp, g_token), 5, lambda gl, gt: ops.seq_logp_bwd(
            l2, ys, prefix_lens, pad_id, row_shift=row_shift, rows_per_seq=R, g_logp=gl, g_token=gt))


class SeqDistFn(torch.autograd.Function):
    """Entropy of the next-token distribution and its KL divergence from a frozen prior's, with a gradient into the
    agent's logits (decode.dist_reference / dist_grad_reference state the rules):
    apply(logits, prior_logits, ys, prefix_lens, pad_id, row_shift) -> (entropy [n], token_entropy [n, W], kl [n],
    token_kl [n, W]); kl / token_kl are None when prior_logits is.  logits, ys, prefix_lens as SeqLogpFn takes them;
    prior_logits fp32 in the shape of logits (or [n * R, V]): no gradient flows into it.  The backward is
    gct_seq_dist_bwd: it writes every row of dlogits, exact zeros where nothing is scored or the weights are 0, and
    autograd adds it to SeqLogpFn's on the same logits."""

    @staticmethod
    def forward(ctx, logits, prior_logits, ys, prefix_lens, pad_id, row_shift):
        l2, R = _seq_rows2d("SeqDistFn", "logits", logits, ys, row_shift)
        q2 = None if prior_logits is None else _seq_rows2d("SeqDistFn", "prior logits", prior_logits.detach(), ys,
                                                           row_shift)[0]
        ys = ys.contiguous()
        te, en, tk, kl = ops.seq_dist(l2, ys, prefix_lens, int(pad_id), row_shift=int(row_shift), rows_per_seq=R,
                                      prior_logits2d=q2)
        ctx.save_for_backward(l2, q2, ys, prefix_lens)
        ctx.geom = (int(pad_id), int(row_shift), R, logits.shape)
        ctx.set_materialize_grads(False)                 # an output nobody used arrives as None, not as zeros
        return en, te, kl, tk

    @staticmethod
    @once_differentiable
    def backward(ctx, g_entropy, g_token_entropy, g_kl, g_token_kl):
        l2, q2, ys, prefix_lens = ctx.saved_tensors
        pad_id, row_shift, R, shape = ctx.geom
        return _seq_backward(shape, l2, (g_entropy, g_token_entropy, g_kl, g_token_kl), 6,
                             lambda ge, gte, gk, gtk: ops.seq_dist_bwd(
                                 l2, ys, prefix_lens, pad_id, row_shift=row_shift, rows_per_seq=R, prior_logits2d=q2,
                                 g_entropy=ge, g_token_entropy=gte, g_kl=gk, g_token_kl=gtk))


class SeqPpoFn(torch.autograd.Function):
    """PPO's clipped surrogate of the scored tokens with a gradient into the logits (decode.ppo_reference /
    ppo_grad_reference state the rules):
    apply(logits, ys, prefix_lens, pad_id, row_shift, old_token_logp, advantage, clip_lo, clip_hi) -> (surrogate [n],
    token_surrogate [n, W], logp [n], token_logp [n, W], approx_kl [n], tokens [n], hits [n], clipped [n]).  logits, ys,
    prefix_lens as SeqLogpFn takes them; old_token_logp fp32 [n, W] and advantage fp32 [n] get no gradient.  Only
    surrogate and token_surrogate are differentiable (once); the other six are reports.  The backward is
    gct_seq_ppo_bwd: it writes every row of dlogits, exact zeros where nothing is scored, the token is clipped, or the
    advantage or the weight is 0."""

    @staticmethod
    def forward(ctx, logits, ys, prefix_lens, pad_id, row_shift, old_token_logp, advantage, clip_lo, clip_hi):
        l2, R = _seq_rows2d("SeqPpoFn", "logits", logits, ys, row_shift)
        ys = ys.contiguous()
        old = _f32c(old_token_logp.detach())
        adv = _f32c(advantage.detach()).view(-1)
        tl, ts, lp, su, kl, nt, nh, nc = ops.seq_ppo(l2, ys, old, adv, float(clip_lo), float(clip_hi), prefix_lens,
                                                 int(pad_id), row_shift=int(row_shift), rows_per_seq=R)
        ctx.save_for_backward(l2, ys, prefix_lens, old, adv)
        ctx.geom = (int(pad_id), int(row_shift), R, logits.shape, float(clip_lo), float(clip_hi))
        ctx.set_materialize_grads(False)                 # an output nobody used arrives as None, not as zeros
        ctx.mark_non_differentiable(lp, tl, kl, nt, nh, nc)
        return su, ts, lp, tl, kl, nt, nh, nc

    @staticmethod
    @once_differentiable
    def backward(ctx, g_surrogate, g_token_surrogate, *unused):
        l2, ys, prefix_lens, old, adv = ctx.saved_tensors
        pad_id, row_shift, R, shape, clip_lo, clip_hi = ctx.geom
        return _seq_backward(shape, l2, (g_surrogate, g_token_surrogate), 9, lambda gs, gts: ops.seq_ppo_bwd(
            l2, ys, old, adv, clip_lo, clip_hi, prefix_lens, pad_id, row_shift=row_shift, rows_per_seq=R,
            g_surrogate=gs, g_token_surrogate=gts))


class KldFn(torch.autograd.Function):
    """Train/trainer1.py:23."""

    @staticmethod
    def forward(ctx, mu, log_var):
        m, l = _f32c(mu), _f32c(log_var)
        ctx.save_for_backward(m, l)
        return ops.kld_fwd(m, l)

    @staticmethod
    def backward(ctx, g):
        m, l = ctx.saved_tensors
        dmu, dlv = ops.kld_bwd(m, l, _f32c(g))
        return dmu, dlv


def check_kl_controls(free_bits, mask_pad=False):
    """(free_bits as a float, mask_pad as a bool) of the trainer's KL controls, or ValueError: free_bits is in nats
    per latent dimension per molecule, a finite number >= 0 that fits fp32 (0: no floor)."""
    if isinstance(free_bits, bool) or not isinstance(free_bits, (int, float)):
        raise ValueError(f"kl_free_bits: expected a number, got {free_bits!r}")
    value = float(free_bits)
    if not (math.isfinite(value) and 0.0 <= value <= 3.4028234663852886e38):
        raise ValueError(f"kl_free_bits: {free_bits!r} is not a finite number >= 0")
    if not isinstance(mask_pad, (bool, int)) or mask_pad not in (0, 1):
        raise ValueError(f"kl_mask_pad: expected a bool, got {mask_pad!r}")
    return value, bool(mask_pad)


def _kl_host_rows(mu, log_var, live):
    """fp32 rows [R, D] of mu and log_var and the live rows as a bool [R], on the host."""
    m = torch.as_tensor(mu).detach().cpu().to(torch.float32)
    l = torch.as_tensor(log_var).detach().cpu().to(torch.float32)
    D = m.shape[-1]
    m, l = m.reshape(-1, D), l.reshape(-1, D)
    keep = torch.ones(m.shape[0], dtype=torch.bool) if live is None else (torch.as_tensor(live).cpu() != 0).reshape(-1)
    if l.shape != m.shape or keep.numel() != m.shape[0]:
        raise ValueError("kl_dims_reference: mu, log_var [..., D] and live [R] do not fit together")
    return m, l, keep


def kl_dims_reference(mu, log_var, live=None, free_bits=0.0, n_mol=1):
    """The rule of gct_kld_dims_fwd on the host: t = 1.0f + l - m*m - expf(l) in fp32 operation by operation, as the
    kernels form it (a kernel may fuse the product into the subtraction, which is inside the kernel tests' bound), then
    K_j = -0.5 * sum over the live rows of (double) t in fp64, floor = free_bits * n_mol, gate_j = K_j > floor.
    Returns a dict: objective, raw (floats), kl_dim fp64 [D], gate bool [D], n_floor, live_rows (ints)."""
    free_bits, _ = check_kl_controls(free_bits)
    if int(n_mol) < 1:
        raise ValueError("kl_dims_reference: n_mol must be >= 1")
    m, l, keep = _kl_host_rows(mu, log_var, live)
    t = ((1.0 + l) - m * m) - torch.exp(l)                                   # fp32, left to right
    K = -0.5 * t[keep].to(torch.float64).sum(dim=0)
    floor = torch.tensor(free_bits, dtype=torch.float32).item() * int(n_mol)      # (double) of the fp32 argument
    gate = K > floor
    return {"objective": float(torch.where(gate, K, torch.full_like(K, floor)).sum()), "raw": float(K.sum()),
            "kl_dim": K, "gate": gate, "n_floor": int((~gate).sum()), "live_rows": int(keep.sum()), "floor": floor}


def kl_dims_grad_reference(mu, log_var, live=None, free_bits=0.0, n_mol=1):
    """d objective / d mu = gate_j * live_r * mu and d objective / d log_var = gate_j * live_r * 0.5 * (exp(lv) - 1),
    fp64 [R, D] each, with the gate of kl_dims_reference."""
    gate = kl_dims_reference(mu, log_var, live, free_bits, n_mol)["gate"]
    m, l, keep = _kl_host_rows(mu, log_var, live)
    w = (keep[:, None] & gate[None, :]).to(torch.float64)
    return w * m.to(torch.float64), w * 0.5 * (torch.exp(l.to(torch.float64)) - 1.0)


class KldFreeBitsFn(torch.autograd.Function):
    """The KL term with free bits over the live latent rows (gct_kld_dims_fwd / gct_kld_dims_bwd; the rule:
    kl_dims_reference): apply(mu, log_var, live, free_bits, n_mol) -> (objective, raw, kl_dim [D], n_floor).
    live: bool/u8 [B, Le], [B, 1, Le] or [R], or None.  Only objective is differentiable (once); raw is the plain KL
    of the live rows, kl_dim its split over the dimensions and n_floor how many sit on the floor.  The backward reads
    the gate the forward wrote."""

    @staticmethod
    def forward(ctx, mu, log_var, live, free_bits, n_mol):
        m, l = _f32c(mu), _f32c(log_var)
        live = None if live is None else ops.to_mask_u8(live)
        out, kl_dim, gate = ops.kld_dims_fwd(m, l, live, free_bits, n_mol)
        ctx.save_for_backward(m, l, gate, *(() if live is None else (live,)))
        objective, raw, n_floor = out[0], out[1], out[2]
        ctx.mark_non_differentiable(raw, kl_dim, n_floor)
        return objective, raw, kl_dim, n_floor

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *unused):
        m, l, gate, *live = ctx.saved_tensors
        dmu, dlv = ops.kld_dims_bwd(m, l, live[0] if live else None, gate, _f32c(g))
        return dmu, dlv, None, None, None


class NormFn(torch.autograd.Function):
    """Standalone Norm module call (Model/modules.py:92-95)."""

    @staticmethod
    def forward(ctx, x, alpha, bias, eps):
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        y, mean, rstd = ops.norm_fwd(x2, alpha, bias, eps)
        ctx.save_for_backward(x2, alpha, mean, rstd)
        ctx.params, ctx.eps, ctx.shp = (alpha, bias), eps, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, alpha, mean, rstd = ctx.saved_tensors
        G = GradSink()
        a, b = ctx.params
        dx = ops.norm_bwd(_f32c(dy).reshape(x2.shape), x2, alpha, mean, rstd, G(a), G(b), eps=ctx.eps)
        return dx.view(ctx.shp), G.out[a], G.out[b], None


# ----------------------------------------------------- standalone sub-module calls (rare)
class EmbedFn(torch.autograd.Function):
    """Embeddings.forward alone: the K1 kernel with scale 1 and a zero positional table."""

    @staticmethod
    def forward(ctx, tok, table):
        B, S = tok.shape
        d = table.shape[1]
        zeros = torch.zeros(S, d, dtype=torch.float32, device=table.device)
        out = ops.embed_pe_fwd(tok.contiguous(), table, None, zeros, 0, 1.0, 0.0, 0, 0)
        ctx.tok, ctx.param = tok.contiguous(), table
        return out.view(B, S, d)

    @staticmethod
    def backward(ctx, dy):
        G = GradSink()
        d = ctx.param.shape[1]
        ops.embed_pe_bwd(_f32c(dy).reshape(-1, d), ctx.tok, G(ctx.param), None, 0, 1.0, 0.0, 0, 0)
        return None, G.out[ctx.param]


class PosEncFn(torch.autograd.Function):
    """PositionalEncoding.forward alone: x*sqrt(d) + pe[:L], dropout -- the K1 kernel with
    zero token columns (every row is a 'cond' row)."""

    @staticmethod
    def forward(ctx, x, pe, scale, run):
        B, L, d = x.shape
        x2 = _f32c(x).view(B, L * d)
        site = run.site()
        dummy_tok = torch.zeros(B, 0, dtype=torch.int64, device=x.device)
        out = ops.embed_pe_fwd(dummy_tok, None, x2, _pe2d_raw(pe, L), L, scale, run.p, run.seed,
                               site, d=d)
        ctx.cfg = (B, L, d, scale, run, site)
        return out.view(B, L, d)

    @staticmethod
    def backward(ctx, dy):
        B, L, d, scale, run, site = ctx.cfg
        dx = torch.empty(B, L * d, dtype=torch.float32, device=dy.device)
        dummy_tok = torch.zeros(B, 0, dtype=torch.int64, device=dy.device)
        ops.embed_pe_bwd(_f32c(dy).reshape(B * L, d), dummy_tok, None, dx, L, scale, run.p,
                         run.seed, site, d=d)
        return dx.view(B, L, d), None, None, None


def _pe2d_raw(pe, L):
    if L > pe.shape[1]:
        raise ValueError(f"sequence length {L} exceeds the positional table ({pe.shape[1]})")
    return pe[0]


def _flat3(x):
    B, L, d = x.shape
    return _f32c(x).view(B * L, d), B, L, d


class MhaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, run, q, kv, mask_u8, want_probs, *params):
        xq, B, Lq, d = _flat3(q)
        if kv is None:
            xkv, Lk = xq, Lq
        else:
            xkv, _, Lk, _ = _flat3(kv)
        y, saved, probs = mha_fwd(run, m, xq, xkv, B, Lq, Lk, mask_u8, None, want_probs)
        ctx.m, ctx.run, ctx.saved, ctx.params = m, run, saved, params
        ctx.shapes = (B, Lq, Lk, d, kv is not None)
        if want_probs:
            ctx.mark_non_differentiable(probs)
            return y.view(B, Lq, d), probs
        return (y.view(B, Lq, d),)

    @staticmethod
    def backward(ctx, dy, *unused):
        B, Lq, Lk, d, cross = ctx.shapes
        G = GradSink()
        dxq = torch.empty(B * Lq, d, dtype=torch.float32, device=dy.device)
        dxkv = torch.empty(B * Lk, d, dtype=torch.float32, device=dy.device) if cross else None
        mha_bwd(ctx.run, ctx.m, ctx.saved, _f32c(dy).reshape(B * Lq, d), G, dxq, ops.DEPI_STORE,
                dxkv, ops.DEPI_STORE)
        ctx.saved = None
        return (None, None, dxq.view(B, Lq, d), dxkv.view(B, Lk, d) if cross else None, None,
                None) + G.collect(ctx.params)


class FfnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ff, run, x, *params):
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        y, saved = ffn_fwd(run, ff, x2, None)
        ctx.ff, ctx.run, ctx.saved, ctx.params, ctx.shp = ff, run, saved, params, x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        G = GradSink()
        dy2 = _f32c(dy).reshape(-1, dy.shape[-1])
        dx = torch.empty_like(dy2)
        ffn_bwd(ctx.run, ctx.ff, ctx.saved, dy2, G, dx, ops.DEPI_STORE)
        ctx.saved = None
        return (None, None, dx.view(ctx.shp)) + G.collect(ctx.params)


class EncLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, run, x, mask_u8, want_probs, *params):
        x2, B, L, d = _flat3(x)
        y, saved, probs = enc_layer_fwd(run, layer, x2, B, L, mask_u8, want_probs)
        ctx.layer, ctx.run, ctx.saved, ctx.params, ctx.shp = layer, run, saved, params, (B, L, d)
        if want_probs:
            ctx.mark_non_differentiable(probs)
            return y.view(B, L, d), probs
        return (y.view(B, L, d),)

    @staticmethod
    def backward(ctx, dy, *unused):
        B, L, d = ctx.shp
        G = GradSink()
        g, _ = enc_layer_bwd(ctx.run, ctx.layer, ctx.saved, _f32c(dy).reshape(B * L, d).clone(), G)
        ctx.saved = None
        return (None, None, g.view(B, L, d), None, None) + G.collect(ctx.params)


class DecLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, run, x, e, src_mask_u8, trg_mask_u8, want_probs, *params):
        x2, B, T, d = _flat3(x)
        e2, _, Lk, _ = _flat3(e)
        y, saved, p1, p2 = dec_layer_fwd(run, layer, x2, e2, B, T, Lk, src_mask_u8, trg_mask_u8,
                                         want_probs)
        ctx.layer, ctx.run, ctx.saved, ctx.params = layer, run, saved, params
        ctx.shp = (B, T, Lk, d)
        if want_probs:
            ctx.mark_non_differentiable(p1, p2)
            return y.view(B, T, d), p1, p2
        return (y.view(B, T, d),)

    @staticmethod
    def backward(ctx, dy, *unused):
        B, T, Lk, d = ctx.shp
        G = GradSink()
        de = torch.empty(B * Lk, d, dtype=torch.float32, device=dy.device)
        g, _ = dec_layer_bwd(ctx.run, ctx.layer, ctx.saved, _f32c(dy).reshape(B * T, d).clone(), de,
                             True, G)
        ctx.saved = None
        return (None, None, g.view(B, T, d), de.view(B, Lk, d), None, None, None) + \
            G.collect(ctx.params)
