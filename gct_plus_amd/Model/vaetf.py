"""Vaetf: unconditioned Transformer-VAE (reference Model/vaetf.py:14-182) on the MI355X
engine.  Same constructor signature, sub-module names, registration order (=> identical RNG
consumption at init, identical state_dict keys and Adam state order) and call contract:

    forward(src, trg, src_mask, trg_mask, econds=None, dconds=None)
        -> (output_prop, output_mol, mu, log_var, z)        [+ attention lists with get_attn]
    encode(src, src_mask, econds=None) -> (z, mu, log_var)
    decode(trg, z, src_mask, trg_mask, dconds=None) -> logits
"""
import torch
import torch.nn as nn

from .. import engine, ops
from ..flat import FlatModelMixin, planes_scope
from .layers import DecoderLayer, EncoderLayer
from .modules import Embeddings, Norm, PositionalEncoding, get_clones
from .sublayers import Sampler


class _TrunkParams:
    """Caches the parameter tuple a trunk hands to its autograd.Function."""

    def trunk_params(self):
        ps = self.__dict__.get("_trunk_params_cache")
        if ps is None:
            ps = tuple(p for n, p in self.named_parameters() if not n.startswith(self._dead_prefixes))
            self.__dict__["_trunk_params_cache"] = ps
        return ps


class Encoder(nn.Module, _TrunkParams):
    _dead_prefixes = ("fc_mu", "fc_log_var")  # owned but never used by Vaetf (vaetf.py:26-27)

    def __init__(self, vocab_size, d_model, N, h, dff, latent_dim, nconds, dropout,
                 variational=True, get_attn=False):
        super().__init__()
        self.N, self.nconds, self.variational, self.get_attn = N, nconds, variational, get_attn
        self.d_model, self.p = d_model, dropout
        self.embed_sentence = Embeddings(d_model, vocab_size)
        self.norm = Norm(d_model)
        self.pe = PositionalEncoding(d_model, dropout=dropout)
        self.layers = get_clones(EncoderLayer(h, d_model, dff, dropout, get_attn), N)
        self.fc_mu = nn.Linear(d_model, latent_dim)
        self.fc_log_var = nn.Linear(d_model, latent_dim)
        if nconds > 0:
            self.embed_cond2enc = nn.Linear(nconds, d_model * nconds)

    def trunk(self, src, src_mask, econds, _plan=None):
        run = engine.Run(self.p, self.training)
        plan = engine.RowPlan.launch(engine.ENCODER).finish() if _plan is None else _plan
        outs = engine.EncoderFn.apply(self, run, src.contiguous(), ops.to_mask_u8(src_mask), econds,
                                      self.get_attn, plan, *self.trunk_params())
        if self.get_attn:
            return outs[0], list(outs[1:])
        return outs, None

    def forward(self, src, src_mask, econds):
        x, attn = self.trunk(src, src_mask, econds)
        return (x, attn) if self.get_attn else x


class _DecoderTrunk(_TrunkParams):
    """The decoder's forward, shared by Vaetf's and Cvaetf's Decoder (which differ in registration order only)."""
    _dead_prefixes = ("\0",)

    def forward(self, trg, z, src_mask, trg_mask, dconds=None, loss_rows=None, _plan=None):
        """loss_rows (bool / uint8 [B, T], optional -- an extension of this build): the rows whose output reaches the
        loss; the others are not computed: they come back as zeros, except the (at most 3 per sample) padded rows that
        share an aligned group of four rows with a live one, which hold arbitrary finite values (engine.decoder_trunk_fwd).
        _plan (engine.RowPlan, finished): the model forward's; that caller gets the COMPACT rows [Mc, d] when
        _plan.live is set and scatters them itself.  Without one the decoder plans its own rows and returns every row."""
        run = engine.Run(self.p, self.training)
        sm, tm = ops.to_mask_u8(src_mask), ops.to_mask_u8(trg_mask)
        plan = _plan
        if plan is None:
            plan = engine.RowPlan.launch(engine.DECODER, self, sm, tm, loss_rows, *trg.shape, z.shape[1]).finish()
        outs = engine.DecoderFn.apply(self, run, trg.contiguous(), z, sm, tm, dconds, self.get_attn, plan,
                                      *self.trunk_params())
        if plan.live is not None and _plan is None:
            outs = engine.ScatterRowsFn.apply(outs, plan.live, trg.size(0), trg.size(1))
        if self.get_attn:
            n = self.N
            return outs[0], list(outs[1:1 + n]), list(outs[1 + n:1 + 2 * n])
        return outs


class Decoder(_DecoderTrunk, nn.Module):   # (the mixin first: its forward, not Module's)
    def __init__(self, vocab_size, d_model, N, h, dff, latent_dim, nconds, dropout, use_cond2dec,
                 use_cond2lat, get_attn=False):
        super().__init__()
        self.N, self.nconds, self.d_model, self.get_attn = N, nconds, d_model, get_attn
        self.use_cond2dec, self.use_cond2lat, self.p = use_cond2dec, use_cond2lat, dropout
        self.embed = Embeddings(d_model, vocab_size)
        self.pe = PositionalEncoding(d_model, dropout=dropout)
        self.fc_z = nn.Linear(latent_dim, d_model)
        self.layers = get_clones(DecoderLayer(h, d_model, dff, dropout, get_attn), N)
        self.norm = Norm(d_model)
        if use_cond2dec and nconds > 0:
            self.embed_cond2dec = nn.Linear(nconds, d_model * nconds)
        if use_cond2lat and nconds > 0:
            self.embed_cond2lat = nn.Linear(nconds, d_model * nconds)


def _row_plan(model, src_mask, trg_mask, loss_rows, trg):
    """engine.RowPlan of a training-style forward (engine.MODEL): the row maps of both trunks, launched with one
    asynchronous read-back; .finish() gives the plan.  Works on the masks exactly as the caller passed them."""
    Le = 0 if src_mask is None else src_mask.shape[-1]
    return engine.RowPlan.launch(engine.MODEL, model.decoder, src_mask, trg_mask, loss_rows, *trg.shape, Le,
                                 n_enc=len(model.encoder.layers))


class Linear(nn.Linear):
    """nn.Linear parameter holder whose forward runs on the MFMA GEMM (`out`, `prop_fc`)."""

    def forward(self, x):
        return engine.LinearFn.apply(x, self.weight, self.bias)


class Vaetf(FlatModelMixin, nn.Module):
    def __init__(self, src_vocab, trg_vocab, N=6, d_model=256, dff=2048, h=8, latent_dim=64,
                 dropout=0.1, nconds=3, use_cond2dec=False, use_cond2lat=False, variational=True,
                 get_attn=False):
        super().__init__()
        self.nconds, self.get_attn = nconds, get_attn
        self.use_cond2dec, self.use_cond2lat = use_cond2dec, use_cond2lat
        self.encoder = Encoder(src_vocab, d_model, N, h, dff, latent_dim, nconds, dropout,
                               variational, get_attn)
        self.decoder = Decoder(trg_vocab, d_model, N, h, dff, latent_dim, nconds, dropout,
                               use_cond2dec, use_cond2lat, get_attn)
        self.sampler = Sampler(d_model, latent_dim, variational)
        self.out = Linear(d_model, trg_vocab)
        if use_cond2dec and nconds > 0:
            self.prop_fc = Linear(trg_vocab, 1)
        self.reset_parameters()

    def reset_parameters(self):
        for _, p in self.named_parameters():        # reference vaetf.py:140-143
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    @planes_scope
    def encode(self, src, src_mask, econds=None):
        x, _ = self.encoder.trunk(src, src_mask, econds)
        return self.sampler(x)

    @planes_scope
    def decode(self, trg, z, src_mask, trg_mask, dconds=None):
        x = self.decoder(trg, z, src_mask, trg_mask, dconds)
        if self.get_attn:
            x = x[0]
        return self.out(x)

    def plan_ahead(self, src_mask, trg_mask, loss_rows, trg):
        """Queue the row maps of a batch that a later forward(..., _plan_ahead=<the returned object>) will use (the
        trainer: the NEXT batch's, between this step's forward and its backward -- Model/forward_propagation1.prefetch)."""
        return _row_plan(self, src_mask, trg_mask, loss_rows, trg)

    @planes_scope
    def forward(self, src, trg, src_mask, trg_mask, econds=None, dconds=None, *, loss_rows=None, _plan_ahead=None):
        """Reference signature (Model/vaetf.py:154) plus one keyword-only extension: loss_rows (bool [B, T]) names the
        decoder rows whose logits reach the loss -- the trainer passes `ys != pad` (Model/forward_propagation1.py); the
        other rows are then not computed at all: their logits come back as zeros -- or, for the few padded rows that share an
        aligned group of four with a live row, as arbitrary finite values -- NOT as the reference's values.  Default (None): every row, as the reference."""
        plan = (_row_plan(self, src_mask, trg_mask, loss_rows, trg) if _plan_ahead is None else _plan_ahead).finish()
        x, enc_attn = self.encoder.trunk(src, src_mask, econds, _plan=plan)
        z, mu, log_var = self.sampler(x)
        d = self.decoder(trg, z, src_mask, trg_mask, dconds, _plan=plan)
        if self.get_attn:
            d, dec_attn_1, dec_attn_2 = d
        output = self.out(d)
        if plan.live is not None:       # the decoder ran on the loss rows only: d and the logits are compact [Mc, .]
            output = engine.ScatterRowsFn.apply(output, plan.live, trg.size(0), trg.size(1))
        if self.use_cond2dec:
            output_prop = self.prop_fc(output[:, :self.nconds, :])
            output_mol = output[:, self.nconds:, :]
        else:
            output_prop = torch.zeros(output.size(0), self.nconds, 1)   # CPU, as the reference
            output_mol = output
        if self.get_attn:
            return output_prop, output_mol, mu, log_var, z, enc_attn, dec_attn_1, dec_attn_2
        return output_prop, output_mol, mu, log_var, z
