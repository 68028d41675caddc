"""KV-cached autoregressive decoding (BASELINE config 5).

The reference's Sampling.decode (Inference/sampling_tool.py:140-184) re-runs the WHOLE decoder
on ys[:, :i+1] for every generated token -- fc_z(z), all six cross-attention K/V projections
and every earlier position are recomputed 79 times, with one device->host sync per step.
Because the decoder is causal, position j's hidden states depend only on tokens 0..j, so the
same token ids come out of
  * `start`:   once per sequence, the cross-attention operands: the key / value projections of the memory fc_z(z) are
               FOLDED into the query / output projections (`_fold_cross`), so a step attends over the latent rows z
               themselves (gct_attn_decode_z) and no per-layer K / V of the memory is built -- or, with a latent wider
               than 2 d_model / H, the K/V of all layers projected once;
  * `prefill`: the prefix (<sos>, or <sos> scaffold <sep>; with use_cond2dec the n_c condition tokens in
               front of it, which see each other and the first token -- Model/modules.py:19-26) through ONE ordinary
               decoder forward, whose per-layer self-attention K/V fill the caches;
  * `step`:    a single-token chain per generated token -- embedding row, 6 x [norm, fused QKV GEMM, single-query
               attention that APPENDS the new key/value to the cache, out-proj+residual, cross-attention, FFN],
               norm, vocabulary GEMM, fused softmax + argmax / multinomial that appends the token and updates the
               key-valid and finished flags on the device.
The step reads its position from a DEVICE-side counter (csrc/decode.hip), so one captured graph serves every step
(`use_graphs=True`): no host round trip, no per-position capture.  Work per generated token drops from O(T) decoder
passes to O(1).  What the unit of step + selection consists of in a given generate call -- the selection, the view of
the rows its kernels get, grammar mask, log-probabilities -- is one `StepPlan`, built by the call and passed down to the
step; the decoder keeps no per-call mode.  `StepPlan.key` states which captured graph (`KVDecoder.graphs`) a unit shares.

Beam search (`start(..., beams=k)` + `generate_beam`): sample s owns rows s*k .. s*k+k-1.  The rules are stated once,
in `beam_step_reference` / `beam_finalize`; gct_beam_select implements the step on the device.  The self-attention
caches, ys and valid stay PHYSICAL slots, each written once by the row that owns it, and an int32 map kv_src [n*k, T]
says where beam r's logical position j lives (row kv_src[r, j]): a selection copies the parent's map row instead of the
parent's caches (gct_attn_decode_beam reads through it).  Final ids: token t of beam b is ys[kv_src[b, off + t], t].

Stochastic beam search (`start(..., beams=k)` + `generate_sbs`; Kool, van Hoof and Welling 2019): the same unit with
another selection, gct_beam_select_gumbel, and one more float per row (`bgumbel`).  The rules are stated once, in
`sbs_step_reference`: beam search over Gumbel-perturbed log-probabilities, each child's Gumbel value conditioned on its
parent's.  The k beams are k DISTINCT sequences, an exact sample without replacement from the model's distribution; the
first is an ordinary sample; `sbs_importance_weights` turns them into an unbiased estimator.

Sequential Monte Carlo under the grammar (`start(..., beams=k)` + `generate_smc`; Lew et al. 2023, Loula et al. 2025):
the same rows and map again, as k weighted PARTICLES per sample.  The rules are stated once, in `smc_step_reference`:
every step multiplies a particle's weight by the mass A_t the grammar mask leaves of its next-token distribution,
resamples the ancestors (systematic) when the effective sample size falls below a threshold, and then draws from the
masked distribution -- gct_grammar_mask_anc reads the particle's history through kv_src, gct_smc_select does the rest.
The weighted particles converge to the model's own distribution restricted to well-formed strings, which the locally
renormalised draws of generate(grammar=) do not, and exp(log_z) is an unbiased estimate of that event's probability.

Mixed prefix lengths (`generate(..., prefix_lens=)`, e.g. one batch of many scaffolds): row r's prefix is ys0[r, :t0_r],
right-padded to t0_max.  The device counter stays shared (the token index of the longest prefix) and row r reads it
through its offset row_off[r] = t0_max - t0_r (gct_decode_embed / gct_attn_decode / gct_select_token), so each row keeps
its own token positions, positional rows, cache slots and multinomial keys (row, token position): it decodes exactly
what it would decode alone.  Row r's generated tokens start at column t0_r of the output (`generated_tokens`).

Top-k / nucleus / temperature sampling (`generate(algo="multinomial", top_k=, top_p=, temperature=)`): the rules are
stated once, in `sample_filter_reference`; gct_select_token applies them on the device between the softmax and the
inverse-CDF draw, reading the settings from a device buffer (`self.filt`), so one captured graph serves any settings and
mixed-prefix rows keep their own draws.

Continuous batching (`start_stream` + `generate_stream`): R decode rows work through a pool of N items.  The rule is
stated once, in `stream_schedule_reference`; gct_stream_refill implements it on the device at the end of every step:
a row whose item produced <eos> (or reached its cap) hands its tokens out and takes the next item of the pool -- latent
rows, masks, condition rows, prefix -- with row_off[r] = *pos + 1, so the row restarts at its own position 0 behind the
same shared counter.  Every item enters that way and consumes its prefix token by token through the step chain (no
prefill), so what an item decodes depends on nothing but the item; its multinomial key is (item, token position).

Log-likelihoods: the rule is stated once, in `score_reference`.  `score_tokens` scores given token rows teacher-forced --
one decoder forward over the rows up to each sequence's last scored token, then gct_seq_logp on the logits; and
`generate` / `generate_stream(return_logp=True)` return the log-probability of every token they pick: gct_chosen_logp
reads the step's logits right behind the selection, so a sampling run needs no second forward to know its likelihood.
`sequence_logp` is score_tokens with a gradient (the backward rule is stated once, in `seq_logp_grad_reference`;
gct_seq_logp_bwd through engine.SeqLogpFn): the per-molecule policy term of a fine-tuning step (Train/finetune.py).
`sequence_policy` adds, from the same one forward, the terms that need the whole next-token distribution: the policy's
entropy and its KL divergence from a frozen prior at every scored token (the rules: `dist_reference` /
`dist_grad_reference`; gct_seq_dist / gct_seq_dist_bwd through engine.SeqDistFn).
`sequence_ppo` is the objective of several updates on one scored batch: PPO's clipped surrogate of each scored token's
probability ratio against the log-probabilities it was sampled with (the rules: `ppo_reference` / `ppo_grad_reference`;
gct_seq_ppo / gct_seq_ppo_bwd through engine.SeqPpoFn), with sequence_policy's terms beside it when asked for.
`marginal_logp` integrates the latent out: the importance-weighted bound of log p(x) over K posterior draws per molecule
(the rules: `latent_iw_reference` / `marginal_reference`; gct_latent_iw writes each latent once with its
log p(z) - log q(z | x), score_tokens scores the block, gct_iw_combine forms the bound in fp64).

Grammar-constrained decoding (`generate` / `generate_stream(grammar=SmilesGrammar(...))`): the rules are stated once, in
`smiles.SmilesGrammar` (grammar_step, grammar_min_finish).  gct_grammar_mask runs in front of the selection: one wave per row
re-derives the row's grammar state from the tokens it has generated (nothing to save for graph capture, nothing to reset
at a stream refill) and writes a copy of the logits with -inf on every token that has no transition or would leave the
row unable to reach <eos> inside its length budget, which it reads from device memory.  Every row then ends with <eos>
and parses.  The guarantee is syntactic only: valence, aromaticity and ring-bond consistency are not part of it.

Chemical validity of FINISHED rows (`smiles.SmilesChemistry.check_rows`): the rules are stated once, in its `check`
-- the grammar's verdict with the position of the first offending token, then the molecular graph: valence caps per
atom, ring closures that double a bond or disagree on its order, aromatic atoms with fewer than two aromatic neighbours.
gct_smiles_check applies them to a batch of decoded rows in one launch (one wave per row; lane 0 walks the row with its
stack and per-atom sums in LDS).  A necessary condition, not a chemistry toolkit; it takes no part in the decode loop.

Per-step sampling statistics (`generate` / `generate_stream(return_stats=True)`): the rules are stated once, in
`step_stats_reference`.  return_logp is the MODEL's log-probability of a token; under a filter or the grammar the token
was drawn from another distribution, the behaviour distribution q.  gct_step_stats runs behind the selection, on the raw
logits and the normalised weights gct_select_token leaves in buf['probs'], and records per generated token the model's
entropy, log q(token), q's entropy and KL(q || model) -- the diagnostics of a collapsing policy without a second
forward, and, summed per row, the denominator of the importance weights Train/finetune.behaviour_weights forms.
"""
from __future__ import annotations

import dataclasses
import functools
import heapq
import math
import numbers
import os
from typing import NamedTuple, Optional

import torch

from . import engine, ops
from ._lib import check
from .flat import planes_scope
# the grammar and the chemistry check live in smiles.py.  Beyond _int_vector and check_grammar, which this module uses,
# the names below are the ones that code written against earlier versions takes from here (`from gct_plus_amd.decode
# import SmilesGrammar`): an import that stopped resolving would break every such caller at import time
from .smiles import (G_END, GRAMMAR_START, ChemReport, SmilesChemistry, SmilesGrammar, _int_vector,  # noqa: F401
                     check_grammar, chem_atom_entry, grammar_class, grammar_min_finish, grammar_step)


# rows per step below which the step's GEMMs take the skinny fp32 kernels (panel / 64x64 split-K) instead of the general
# path (bf16x6).  Measured on MI355X: n = 1100 / 1536 / 2048 / 3000 take 2.18 / 2.32 / 2.39 / 3.04 ms per token on the
# general path against 2.27 / 2.46 / 2.58 / 3.74 on the skinny kernels
SKINNY_BELOW = 1024
# cross-attention of a step over the latent rows themselves (gct_attn_decode_z) instead of per-layer K / V projections of
# the memory; False keeps the projected K / V (the tests compare the two; also taken when the latent is too wide)
ZATTN = True
# replay guard of use_graphs=True (KVDecoder._replay_is_fast): replay must not be slower than REPLAY_SLOW_FACTOR x the
# eager launches of the same step on this box; `GCT_DECODE_GRAPH_GUARD=0` switches the guard off (always replay)
REPLAY_GUARD = os.environ.get("GCT_DECODE_GRAPH_GUARD", "1") != "0"
REPLAY_SLOW_FACTOR = 1.3
# beam search: length penalty exponent of the final ranking score / length**alpha (reference generate_mols.py:182-185)
BEAM_ALPHA = 0.7
BEAM = "beam"                                       # StepPlan.select: the beam step (gct_beam_select)
SBEAM = "sbeam"                                     # StepPlan.select: the stochastic beam step (gct_beam_select_gumbel)
SMC = "smc"                                         # StepPlan.select: the sequential Monte Carlo step (gct_smc_select)
FILTERED = "filtered"                               # StepPlan.select: the filtered multinomial draw
UNIFORM, MIXED, STREAM = "uniform", "mixed", "stream"      # StepPlan.layout
LOGP = "logp"                                       # graph key suffix of a step unit that records log-probabilities
GRAMMAR = "grammar"                                 # graph key suffix of a step unit that masks the logits by a grammar
STATS = "stats"                                     # graph key suffix of a step unit that records the step statistics
STREAM_COND_CHUNK = 256                             # items per GEMM when the pool's condition rows are projected
TOP_K_FLOOR = 1e-6                                  # weight of a token outside the top k (the reference's top_k_logits)


@dataclasses.dataclass(frozen=True)
class StepPlan:
    """What one step unit is -- the decode step plus the selection, the unit a graph captures.  Each generate call
    builds one and passes it down; KVDecoder keeps no per-call mode of its own.
      select   0 greedy, 1 multinomial, FILTERED (the multinomial draw through self.filt), BEAM (gct_beam_select, the
               self-attention through the ancestry map kv_src), SBEAM (the same unit with gct_beam_select_gumbel) or SMC
               (the same rows again: gct_grammar_mask_anc through the map, then gct_smc_select);
      layout   UNIFORM: every row at the shared position.  MIXED: the kernels get row_off.  STREAM: row_off plus the
               rows' item and prefix_len, and the unit ends with the refill (KVDecoder._rows is the row view);
      grammar  gct_grammar_mask runs in front of the selection;
      logp     gct_chosen_logp runs behind it;
      stats    gct_step_stats runs behind it too, and a multinomial draw through a filter or a grammar leaves the
               distribution it drew from in buf['probs'] for it.
    ValueError for what the unit cannot do: beam rows keep their history behind kv_src and their scores are
    log-probabilities already, so BEAM and SBEAM go with UNIFORM and neither grammar, logp nor stats.  SMC is the unit
    whose mask reads that history through the map: UNIFORM rows, the grammar always (it is the potential the particles
    are weighted by), and neither logp nor stats (gct_smc_select accumulates the particles' log-probabilities itself)."""
    select: object = 0
    layout: str = UNIFORM
    grammar: bool = False
    logp: bool = False
    stats: bool = False

    def __post_init__(self):
        select, layout, grammar, logp, stats = dataclasses.astuple(self)
        if select not in (0, 1, FILTERED, BEAM, SBEAM, SMC) or layout not in (UNIFORM, MIXED, STREAM):
            raise ValueError(f"no step unit selects {select!r} over {layout!r} rows")
        if select in (BEAM, SBEAM) and (layout != UNIFORM or grammar or logp or stats):
            raise ValueError(f"the {'stochastic ' * (select == SBEAM)}beam step takes uniform rows, no grammar, no "
                             "log-probabilities and no step statistics")
        if select == SMC and (layout != UNIFORM or not grammar or logp or stats):
            raise ValueError("the sequential Monte Carlo step takes uniform rows and a grammar, no log-probabilities and "
                             "no step statistics")

    @functools.cached_property
    def key(self):
        """THE statement of the graph key (KVDecoder.graphs; bench.py, the tools and the tests read it): `select` alone
        for plain uniform rows -- the only rows BEAM ("beam") and SBEAM ("sbeam") have; (select, layout) for another
        layout; and with a grammar, log-probabilities and / or step statistics (select, layout[, GRAMMAR][, LOGP][,
        STATS]), uniform spelled out.  A stream unit has k[1] == STREAM; a unit without stats has logp k[-1] == LOGP."""
        select, layout, grammar, logp, stats = dataclasses.astuple(self)
        tail = (GRAMMAR,) * bool(grammar) + (LOGP,) * bool(logp) + (STATS,) * bool(stats)
        if layout == UNIFORM and not tail:
            return select
        return (select, layout) + tail


# ------------------------------------------------------------------------- top-k / nucleus / temperature sampling
def check_sample_filter(top_k=None, top_p=None, temperature=1.0, vocab=None):
    """Validate sampling settings: top_k None or an int in [1, vocab]; top_p None or a real in (0, 1]; temperature a
    finite real > 0 whose fp32 reciprocal is finite.  ValueError otherwise.  Returns True when the settings change the
    distribution (k < vocab, top_p < 1 or temperature != 1), False when they are neutral."""
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral):
            raise ValueError(f"top_k must be None or an int, got {top_k!r}")
        if top_k < 1 or (vocab is not None and top_k > vocab):
            raise ValueError(f"top_k {top_k} outside [1, {vocab if vocab is not None else 'V'}]")
    if top_p is not None:
        if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real) or not 0.0 < float(top_p) <= 1.0:
            raise ValueError(f"top_p must be None or a real in (0, 1], got {top_p!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real):
        raise ValueError(f"temperature must be a real number, got {temperature!r}")
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0 and 1.0 / t < 3.0e38):
        raise ValueError(f"temperature must be finite and > 0 (with a finite fp32 reciprocal), got {temperature!r}")
    return ((top_k is not None and (vocab is None or top_k < vocab)) or (top_p is not None and float(top_p) < 1.0)
            or t != 1.0)


def sample_filter_reference(logits, top_k=None, top_p=None, temperature=1.0):
    """THE statement of the sampling filter (gct_select_token's filtered draw implements it): logits [..., V] -> the
    normalised distribution [..., V] the multinomial draw uses.
      1. p = softmax(x / T) in fp32;
      2. top_k: token c is in when fewer than k tokens have a strictly larger LOGIT (ties at the k-th value stay in, the
         reference's p_c >= v_k); an out token gets the weight TOP_K_FLOOR = 1e-6, as the reference's top_k_logits gives
         it before torch.multinomial renormalises; k = V is a no-op; a token whose logit is -inf (one a grammar mask
         forbids) has the weight 0 at every stage and never gets the floor;
      3. top_p (nucleus) on s = w / sum w, w the result of 2: token c is kept when the mass of the tokens with a strictly
         larger s is < top_p (every token tied at the boundary is kept), otherwise its weight is 0; top_p = 1 is a no-op;
      4. the draw picks c with probability w_c / sum w (returned).  The top token is always kept, so greedy ignores all
         three settings."""
    V = logits.shape[-1]
    check_sample_filter(top_k, top_p, temperature, V)
    x = logits.float()
    w = torch.softmax(x / float(temperature), -1)
    if top_k is not None and top_k < V:
        asc = x.sort(-1).values
        larger = V - torch.searchsorted(asc, x.contiguous(), right=True)           # tokens with a strictly larger logit
        w = torch.where((larger < top_k) | (x == -math.inf), w, torch.full_like(w, TOP_K_FLOOR))
    if top_p is not None and top_p < 1:
        s = w / w.sum(-1, keepdim=True)
        asc = s.sort(-1).values
        larger = V - torch.searchsorted(asc, s.contiguous(), right=True)           # tokens with a strictly larger s
        top_mass = asc.flip(-1).double().cumsum(-1)                                  # mass of the j + 1 largest
        mass = torch.where(larger > 0, top_mass.gather(-1, (larger - 1).clamp(min=0)), torch.zeros_like(top_mass))
        w = torch.where(mass < float(top_p), w, torch.zeros_like(w))
    return w / w.sum(-1, keepdim=True)


# ------------------------------------------------------------------------------------------- log-likelihoods
def check_score_inputs(ys, prefix_lens, vocab):
    """Validate the inputs of a scoring call: ys an integer tensor [n, W >= 2] of token ids in [0, vocab); prefix_lens
    None or integers [n] in [1, W].  ValueError otherwise.  Returns the prefix lengths as an int64 CPU tensor [n] (all 1
    for None)."""
    ys = torch.as_tensor(ys)
    if ys.dim() != 2 or ys.shape[1] < 2:
        raise ValueError(f"ys must be [n, W >= 2] (full token rows), got {list(ys.shape)}")
    if ys.dtype.is_floating_point or ys.dtype.is_complex or ys.dtype == torch.bool:
        raise ValueError(f"ys must hold integer token ids, got {ys.dtype}")
    n, W = ys.shape
    lens = torch.ones(n, dtype=torch.int64) if prefix_lens is None else _int_vector(
        "prefix_lens", prefix_lens, n, 1, W, "the row width")
    if n and (int(ys.min()) < 0 or int(ys.max()) >= int(vocab)):
        raise ValueError(f"token ids must lie in [0, {int(vocab)}), got [{int(ys.min())}, {int(ys.max())}]")
    return lens


def score_reference(logits, ys, prefix_lens, pad_id):
    """THE statement of the scoring rule (gct_seq_logp implements it on teacher-forced logits, gct_chosen_logp on the
    logits of a decode step).  ys [n, W] int64: full token rows -- prefix, tokens, pad (generate(prefix_lens=)'s layout);
    logits [n, W - 1, V]: the teacher-forced logits of the inputs ys[:, :-1], row c - 1 predicts token c; prefix_lens
    ints [n], 1 <= t0_r <= W (None: 1, only <sos> is given).
    Column c of row r is SCORED when c >= t0_r and ys[r, c] != pad_id.  Returns, in the dtype of logits (fp32 at least):
      token_logp [n, W]  x[t] - m - log(sum exp(x - m)) at scored columns (beam_log_softmax's form, m the row maximum),
                         0 elsewhere;
      logp [n]           the sum of a row's scored columns in ascending column order;
      tokens [n] int32   the number of scored columns;
      hits [n] int32     the scored columns whose target is the FIRST maximum of its logits row (torch.argmax).
    A row without a scored column gives 0, 0, 0."""
    ys, x, tgt, scored = _scored_rows(logits, ys, prefix_lens, pad_id)
    y = x - x.max(-1, keepdim=True).values
    lsm = y - torch.log(torch.exp(y).sum(-1, keepdim=True))
    token_logp, logp = _column_sums(scored, lsm.gather(-1, tgt.unsqueeze(-1)).squeeze(-1))
    hit = scored & (x.argmax(-1) == tgt)
    return token_logp, logp, scored.sum(1).to(ys.device, torch.int32), hit.sum(1).to(torch.int32)


class StepStats(NamedTuple):
    """What generate / generate_stream(return_stats=True) return behind their other results (step_stats_reference states
    the per-step rules): four fp32 tables [n, L] laid out like ys -- kept on a row's generated span up to its first
    <eos> (return_logp's span), 0 elsewhere -- and behaviour_logp_sum [n], the row sum of behaviour_logp: the
    log-probability of the row under the distribution it was actually sampled from."""
    model_entropy: torch.Tensor
    behaviour_logp: torch.Tensor
    behaviour_entropy: torch.Tensor
    behaviour_kl: torch.Tensor
    behaviour_logp_sum: torch.Tensor


def step_stats_reference(logits, probs, tok, pad_id, greedy=False):
    """THE statement of the per-step sampling statistics (gct_step_stats implements it behind the selection), in fp64
    on the host.  logits [n, V]: the step's RAW logits; tok [n]: the token each row received; probs [n, V] or None:
    the normalised weights the draw used (gct_select_token's probs_out), taken as given.
      pi = softmax(logits) at temperature 1, in log-sum-exp form (score_reference's);
      q  = the BEHAVIOUR distribution the token was drawn from: probs; pi itself when probs is None; the one-hot at tok
           when greedy (probs is ignored).
    Returns fp64 [n] each:
      model_entropy     -sum pi log pi                       behaviour_logp  log q(tok)
      behaviour_entropy -sum_{q > 0} q log q                 behaviour_kl    sum_{q > 0} q (log q - log pi)
    A term with q == 0 (pi == 0) adds exactly 0.  A row whose token is pad_id (a finished row; or no token of the
    vocabulary) gives four zeros.  With probs None and not greedy log q IS log pi: behaviour_logp is the model's
    log-probability (score_reference's), behaviour_entropy is model_entropy and behaviour_kl is exactly 0."""
    x = torch.as_tensor(logits).double()
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"logits must be [n, V >= 1], got {list(x.shape)}")
    n, V = x.shape
    tok = torch.as_tensor(tok).long().reshape(-1)
    if tok.numel() != n:
        raise ValueError(f"tok must hold {n} tokens, got {tok.numel()}")
    live = (tok != pad_id) & (tok >= 0) & (tok < V)
    at = tok.clamp(0, V - 1).view(n, 1)
    y = x - x.max(-1, keepdim=True).values
    lpi = y - torch.log(torch.exp(y).sum(-1, keepdim=True))
    pi, zero = torch.exp(lpi), torch.zeros((), dtype=torch.float64)
    if greedy:
        q = torch.zeros_like(pi).scatter_(1, at, 1.0)
        lq = torch.zeros_like(pi)
    elif probs is None:
        q, lq = pi, lpi
    else:
        q = torch.as_tensor(probs).double()
        if q.shape != x.shape:
            raise ValueError(f"probs must have the shape of logits {list(x.shape)}, got {list(q.shape)}")
        lq = torch.log(torch.where(q > 0, q, torch.ones_like(q)))
    model_entropy = -torch.where(pi > 0, pi * lpi, zero).sum(-1)
    qt = q.gather(1, at).view(n)
    behaviour_logp = torch.where(qt > 0, lq.gather(1, at).view(n), torch.full((), -math.inf, dtype=torch.float64))
    behaviour_entropy = -torch.where(q > 0, q * lq, zero).sum(-1)
    behaviour_kl = torch.where(q > 0, q * (lq - lpi), zero).sum(-1)
    return tuple(torch.where(live, v, zero) for v in (model_entropy, behaviour_logp, behaviour_entropy, behaviour_kl))


def _scored_rows(logits, ys, prefix_lens, pad_id):
    """Shared front of the six rules below: check_score_inputs and the shape check, then (ys as a tensor, x = the logits
    [n, W - 1, V] in fp64 or fp32, the targets ys[:, 1:] int64 [n, W - 1], score_reference's SCORED predicate bool
    [n, W - 1]), the last two on the device of x."""
    ys = torch.as_tensor(ys)
    lens = check_score_inputs(ys, prefix_lens, logits.shape[-1])
    n, W = ys.shape
    x = logits if logits.dtype == torch.float64 else logits.float()
    if tuple(x.shape[:2]) != (n, W - 1):
        raise ValueError(f"logits must be [{n}, {W - 1}, V], got {list(logits.shape)}")
    tgt = ys[:, 1:].long().to(x.device)
    scored = (torch.arange(1, W).view(1, -1) >= lens.view(-1, 1)).to(x.device) & (tgt != pad_id)
    return ys, x, tgt, scored


def _column_sums(scored, per_row):
    """per_row [n, W - 1], a value per logits row -> the token table [n, W] (per_row at the scored columns, 0 elsewhere
    and in column 0) and its row sums [n], added in ascending column order."""
    n, W = per_row.shape[0], per_row.shape[1] + 1
    zero = torch.zeros((), dtype=per_row.dtype, device=per_row.device)
    table = torch.cat([zero.expand(n, 1), torch.where(scored, per_row, zero)], dim=1)
    total = torch.zeros(n, dtype=per_row.dtype, device=per_row.device)
    for c in range(1, W):                                # ascending column order
        total = total + table[:, c]
    return table, total


def _grad_weight(g_row, g_table, like, n, W):
    """The weight of every logits row [n, W - 1] under incoming gradients g_row [n] and g_table [n, W] (None: 0), in the
    dtype and on the device of `like`: (g_row[r] + g_table[r, c]) for row c - 1."""
    g = torch.zeros(n, W, dtype=like.dtype, device=like.device)
    if g_row is not None:
        g = g + torch.as_tensor(g_row).to(like.device, like.dtype).view(n, 1)
    if g_table is not None:
        g = g + torch.as_tensor(g_table).to(like.device, like.dtype).view(n, W)
    return g[:, 1:]


@planes_scope
def _teacher_forced_logits(model, trg, z, src_mask, trg_mask, dconds, loss_rows):
    """model.decode with loss_rows: the decoder rows that are not marked are not computed (when the row planner accepts
    them), under the weight-plane scope model.decode runs in."""
    x = model.decoder(trg, z, src_mask, trg_mask, dconds, loss_rows=loss_rows)
    if model.get_attn:
        x = x[0]
    return model.out(x)


def seq_logp_grad_reference(logits, ys, prefix_lens, pad_id, g_logp=None, g_token=None):
    """THE statement of the backward rule of score_reference (gct_seq_logp_bwd implements it): the gradient with respect
    to the logits [n, W - 1, V] of  sum_r g_logp[r] * logp[r] + sum_{r, c} g_token[r, c] * token_logp[r, c]  (g_logp [n],
    g_token [n, W]; None: 0).  With g[r, c] = g_logp[r] + g_token[r, c], row c - 1 of sequence r gets
      g[r, c] * ([v == ys[r, c]] - softmax(logits[r, c - 1])[v])   where column c is scored (score_reference's predicate),
      exact zeros                                                   where it is not, or where g[r, c] == 0 -- whatever
    the logits row holds, NaN included: such a row is never looked at.
    Closed form, in the dtype of logits (fp32 at least), on the device of logits."""
    ys, x, tgt, scored = _scored_rows(logits, ys, prefix_lens, pad_id)
    n, W = ys.shape
    g = _grad_weight(g_logp, g_token, x, n, W)
    live = scored & (g != 0)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    grad = -(e / e.sum(-1, keepdim=True))
    grad.scatter_add_(-1, tgt.unsqueeze(-1), torch.ones(n, W - 1, 1, dtype=x.dtype, device=x.device))
    return torch.where(live.unsqueeze(-1), g.unsqueeze(-1) * grad, torch.zeros((), dtype=x.dtype, device=x.device))


def _dist_rows(logits, prior_logits, ys, prefix_lens, pad_id):
    """Shared front of dist_reference / dist_grad_reference: _scored_rows' (ys, x, scored) and the prior's logits in the
    dtype and on the device of x (None without a prior)."""
    ys, x, _, scored = _scored_rows(logits, ys, prefix_lens, pad_id)
    y = None
    if prior_logits is not None:
        if prior_logits.shape != logits.shape:
            raise ValueError(f"prior_logits must have the shape of logits {list(logits.shape)}, got "
                             f"{list(prior_logits.shape)}")
        y = prior_logits.to(x.device, x.dtype)
    return ys, x, y, scored


def _log_softmax_rows(x, live):
    """log-softmax, in log-sum-exp form, of the rows marked in live [n, W - 1]; a row that is not marked is replaced by
    zeros BEFORE any arithmetic, so nothing it holds (NaN included) reaches a value or a gradient."""
    x = torch.where(live.unsqueeze(-1), x, torch.zeros((), dtype=x.dtype, device=x.device))
    s = x - x.max(-1, keepdim=True).values
    return s - torch.log(torch.exp(s).sum(-1, keepdim=True))


def _p_logp(x, live):
    """(p, log p) of the marked rows; where p == 0 (a -inf logit) log p is replaced by 0, so that p * log p is exactly
    0 there, also under autograd."""
    logp = _log_softmax_rows(x, live)
    p = torch.exp(logp)
    return p, torch.where(p > 0, logp, torch.zeros((), dtype=x.dtype, device=x.device))


def dist_reference(logits, ys, prefix_lens, pad_id, prior_logits=None):
    """THE statement of the distribution terms of a policy (gct_seq_dist implements it): the entropy of the next-token
    distribution and its KL divergence from a second model's (the "prior"), at score_reference's geometry and under its
    SCORED predicate (ys [n, W] full token rows, logits [n, W - 1, V], row c - 1 predicts token c, column c of row r is
    scored when c >= t0_r and ys[r, c] != pad_id).  prior_logits: None, or the prior's logits in the shape of logits.
    At a scored column, with p = softmax(logits[r, c - 1]) and q = softmax(prior_logits[r, c - 1]), both in log-sum-exp
    form (log p_v = x_v - m - log sum exp(x - m), m the row maximum):
      token_entropy [n, W]  -sum_v p_v log p_v
      token_kl [n, W]       sum_v p_v (log p_v - log q_v)        = KL(agent || prior)
    A term with p_v == 0 (a -inf logit) contributes exactly 0; p_v > 0 where q_v == 0 gives +inf (the prior forbids a
    token the agent still draws).  Columns that are not scored hold 0 -- whatever their logits rows hold, NaN included:
    such a row is never looked at.
      entropy [n], kl [n]   the sums of a row's scored columns in ascending column order; 0 for a row with none.
    Returns (token_entropy, entropy, token_kl, kl), the last two None without prior_logits, in the dtype of logits (fp32
    at least) on the device of logits."""
    ys, x, y, scored = _dist_rows(logits, prior_logits, ys, prefix_lens, pad_id)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    p, logp = _p_logp(x, scored)
    token_entropy, entropy = _column_sums(scored, -(p * logp).sum(-1))
    if y is None:
        return token_entropy, entropy, None, None
    logq = torch.where(p > 0, _log_softmax_rows(y, scored), zero)   # q_v plays no part where p_v == 0
    token_kl, kl = _column_sums(scored, (p * (logp - logq)).sum(-1))
    return token_entropy, entropy, token_kl, kl


def dist_grad_reference(logits, ys, prefix_lens, pad_id, prior_logits=None, g_entropy=None, g_token_entropy=None,
                        g_kl=None, g_token_kl=None):
    """THE statement of the backward rule of dist_reference (gct_seq_dist_bwd implements it): the gradient with respect
    to the AGENT's logits [n, W - 1, V] of  sum_r g_entropy[r] * entropy[r] + sum_{r, c} g_token_entropy[r, c] *
    token_entropy[r, c] + sum_r g_kl[r] * kl[r] + sum_{r, c} g_token_kl[r, c] * token_kl[r, c]  (tables [n] and [n, W];
    None: 0; the kl pair needs prior_logits).  The prior gets no gradient.  With a = g_entropy[r] + g_token_entropy[r, c]
    and b = g_kl[r] + g_token_kl[r, c], and H, KL the column's token_entropy and token_kl, row c - 1 of sequence r gets
      a * (-p_v (log p_v + H)) + b * (p_v ((log p_v - log q_v) - KL))   where column c is scored,
      exact zeros                                                      where it is not, or where a == 0 and b == 0 --
    whatever the agent's and the prior's logits rows hold, NaN included: such rows are never looked at.  Entries with
    p_v == 0 get exact zeros.  Closed form, in the dtype of logits (fp32 at least), on the device of logits."""
    if prior_logits is None and (g_kl is not None or g_token_kl is not None):
        raise ValueError("dist_grad_reference: g_kl / g_token_kl need prior_logits")
    ys, x, y, scored = _dist_rows(logits, prior_logits, ys, prefix_lens, pad_id)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    a, b = _grad_weight(g_entropy, g_token_entropy, x, *ys.shape), _grad_weight(g_kl, g_token_kl, x, *ys.shape)
    live = scored & ((a != 0) | (b != 0))
    p, logp = _p_logp(x, live)
    H = -(p * logp).sum(-1, keepdim=True)
    grad = a.unsqueeze(-1) * (-p * (logp + H))
    if y is not None:
        logq = torch.where(p > 0, _log_softmax_rows(y, live & (b != 0)), zero)
        d = logp - logq
        KL = (p * d).sum(-1, keepdim=True)
        grad = grad + torch.where((b != 0).unsqueeze(-1), b.unsqueeze(-1) * (p * (d - KL)), zero)
    return torch.where(live.unsqueeze(-1) & (p > 0), grad, zero)


def clip_pair(clip):
    """PPO's clip argument as (clip_lo, clip_hi) floats: a number e means (e, e), a pair (lo, hi) itself.  ValueError for
    anything else; the ranges are check_ppo_inputs' business."""
    if isinstance(clip, numbers.Real) and not isinstance(clip, bool):
        return float(clip), float(clip)
    try:
        lo, hi = clip
        if any(isinstance(v, bool) or not isinstance(v, numbers.Real) for v in (lo, hi)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"clip must be a number or a pair (clip_lo, clip_hi) of numbers, got {clip!r}") from None
    return float(lo), float(hi)


def check_ppo_inputs(old_token_logp, advantage, clip_lo, clip_hi, n, W):
    """Validate what PPO's surrogate takes beside a scoring call's inputs, for n token rows of W columns: old_token_logp
    a floating-point tensor [n, W]; advantage [n] finite numbers; 0 <= clip_lo < 1 (the lower bound 1 - clip_lo of the
    ratio stays positive); clip_hi >= 0.  ValueError otherwise, before any device work of the caller.
    The VALUES of old_token_logp are not looked at -- the table lives on the device, and a check would wait for it: a
    non-finite entry on a scored column is not refused, IEEE arithmetic decides the result there (NaN gives a NaN
    surrogate and gradient row, +inf a ratio of 0, -inf an infinite one).  Returns advantage as a tensor."""
    if not isinstance(old_token_logp, torch.Tensor) or not old_token_logp.dtype.is_floating_point:
        raise ValueError("old_token_logp must be a floating-point tensor")
    if tuple(old_token_logp.shape) != (n, W):
        raise ValueError(f"old_token_logp must be [{n}, {W}], got {list(old_token_logp.shape)}")
    adv = torch.as_tensor(advantage)
    if adv.dtype == torch.bool or adv.dtype.is_complex:
        raise ValueError(f"advantage must hold real numbers, got {adv.dtype}")
    if adv.dim() != 1 or adv.numel() != n:
        raise ValueError(f"advantage must have shape [{n}], got {list(adv.shape)}")
    if not bool(torch.isfinite(adv.double()).all()):
        raise ValueError("advantage must be finite")
    for name, v in (("clip_lo", clip_lo), ("clip_hi", clip_hi)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"{name} must be a number, got {v!r}")
    if not 0 <= clip_lo < 1:
        raise ValueError(f"clip_lo must lie in [0, 1), got {clip_lo!r}")
    if not clip_hi >= 0:
        raise ValueError(f"clip_hi must be >= 0, got {clip_hi!r}")
    return adv


def _ppo_rows(logits, ys, prefix_lens, pad_id, old_token_logp, advantage, clip_lo, clip_hi):
    """Shared front of ppo_reference / ppo_grad_reference: (ys, x, n, W, scored [n, W - 1], targets [n, W - 1], old
    [n, W - 1], A [n, 1], lo, hi) in the dtype and on the device of x; lo = 1 - clip_lo and hi = 1 + clip_hi are formed
    in that dtype."""
    ys, x, tgt, scored = _scored_rows(logits, ys, prefix_lens, pad_id)
    n, W = ys.shape
    adv = check_ppo_inputs(torch.as_tensor(old_token_logp), advantage, clip_lo, clip_hi, n, W)
    dev = x.device
    old = torch.as_tensor(old_token_logp).to(dev, x.dtype)[:, 1:]
    A = adv.to(dev, x.dtype).view(n, 1)
    one = torch.ones((), dtype=x.dtype, device=dev)
    return ys, x, n, W, scored, tgt, old, A, one - clip_lo, one + clip_hi


def ppo_reference(logits, ys, prefix_lens, pad_id, old_token_logp, advantage, clip_lo, clip_hi):
    """THE statement of PPO's clipped surrogate over the scored tokens (gct_seq_ppo implements it), at score_reference's
    geometry and under its SCORED predicate (ys [n, W] full token rows, logits [n, W - 1, V], row c - 1 predicts token
    c).  old_token_logp [n, W]: the log-probabilities the tokens were sampled with (score_reference's token_logp under
    the sampling-time policy); advantage [n]: one number per sequence; 0 <= clip_lo < 1, clip_hi >= 0
    (check_ppo_inputs).  At a scored column (r, c), with lp = score_reference's token_logp[r, c], A = advantage[r] and
      rho = exp(lp - old_token_logp[r, c]):
    the token is CLIPPED when (A > 0 and rho > 1 + clip_hi) or (A < 0 and rho < 1 - clip_lo) -- strict comparisons, so
    rho == 1 is never clipped, even with a clip of 0 --, and
      token_surrogate [n, W]  A * (1 + clip_hi) clipped high, A * (1 - clip_lo) clipped low, A * rho otherwise
                              (= min(rho A, clamp(rho, 1 - clip_lo, 1 + clip_hi) A) in value);
      the k3 term             (rho - 1) - (lp - old): an estimator of KL(old || new), >= 0.
    Columns that are not scored hold 0, whatever their logits rows and old_token_logp hold.  Per sequence, sums of the
    scored columns in ascending column order: logp [n], surrogate [n], approx_kl [n] (the k3 terms); counts: tokens [n],
    hits [n], clipped [n] int32.  token_logp, logp, tokens and hits are score_reference's.
    Returns (token_logp, token_surrogate, logp, surrogate, approx_kl, tokens, hits, clipped), in the dtype of logits
    (fp32 at least) on the device of logits.  A non-finite old_token_logp on a scored column is not an error: IEEE
    arithmetic decides."""
    ys, x, n, W, scored, tgt, old, A, lo, hi = _ppo_rows(logits, ys, prefix_lens, pad_id, old_token_logp, advantage,
                                                         clip_lo, clip_hi)
    token_logp, logp, tokens, hits = score_reference(x, ys, prefix_lens, pad_id)
    d = torch.where(scored, token_logp[:, 1:] - old, torch.zeros((), dtype=x.dtype, device=x.device))
    rho = torch.exp(d)
    up = scored & (A > 0) & (rho > hi)
    down = scored & (A < 0) & (rho < lo)
    token_surrogate, surrogate = _column_sums(scored, torch.where(up, A * hi, torch.where(down, A * lo, A * rho)))
    _, approx_kl = _column_sums(scored, (rho - 1) - d)
    return (token_logp, token_surrogate, logp, surrogate, approx_kl, tokens, hits,
            (up | down).sum(1).to(torch.int32))


def ppo_grad_reference(logits, ys, prefix_lens, pad_id, old_token_logp, advantage, clip_lo, clip_hi, g_surrogate=None,
                       g_token_surrogate=None):
    """THE statement of the backward rule of ppo_reference (gct_seq_ppo_bwd implements it): the gradient with respect to
    the logits [n, W - 1, V] of  sum_r g_surrogate[r] * surrogate[r] + sum_{r, c} g_token_surrogate[r, c] *
    token_surrogate[r, c]  (g_surrogate [n], g_token_surrogate [n, W]; None: 0).  With g = g_surrogate[r] +
    g_token_surrogate[r, c], A = advantage[r] and rho as in ppo_reference, row c - 1 of sequence r gets
      ((g * A) * rho) * ([v == ys[r, c]] - softmax(logits[r, c - 1])[v])   where column c is scored and not clipped,
      exact zeros   where the column is not scored, the token is clipped, A == 0 or g == 0 -- whatever the logits row
    holds, NaN included.  For a column that is not scored, or with A == 0 or g == 0, the row is never looked at; a
    clipped token's row is, to decide that it is clipped.  old_token_logp and advantage get no gradient.
    Closed form, in the dtype of logits (fp32 at least), on the device of logits."""
    ys, x, n, W, scored, tgt, old, A, lo, hi = _ppo_rows(logits, ys, prefix_lens, pad_id, old_token_logp, advantage,
                                                         clip_lo, clip_hi)
    dev = x.device
    zero = torch.zeros((), dtype=x.dtype, device=dev)
    g = _grad_weight(g_surrogate, g_token_surrogate, x, n, W)
    looked = scored & (g != 0) & (A != 0)
    lsm = _log_softmax_rows(x, looked)                   # the other rows: zeros before any arithmetic
    d = torch.where(looked, lsm.gather(-1, tgt.unsqueeze(-1)).squeeze(-1) - old, zero)
    rho = torch.exp(d)
    live = looked & ~(((A > 0) & (rho > hi)) | ((A < 0) & (rho < lo)))
    grad = -torch.exp(lsm)
    grad.scatter_add_(-1, tgt.unsqueeze(-1), torch.ones(n, W - 1, 1, dtype=x.dtype, device=dev))
    w = (g * A) * rho
    return torch.where(live.unsqueeze(-1), w.unsqueeze(-1) * grad, zero)


def _score_geometry(model, ys, prefix_lens):
    """What every teacher-forced scoring call validates before any device work: (ys as a tensor, prefix lengths int64
    [n] on the CPU, use_cond2dec, row_shift = the condition rows in front of a sequence's logits, V).  ValueError for
    malformed inputs (check_score_inputs) and for rows beyond the positional table."""
    dec = model.decoder
    V = model.out.weight.shape[0]
    ys = torch.as_tensor(ys)
    lens = check_score_inputs(ys, prefix_lens, V)
    W = ys.shape[1]
    c2d = bool(dec.use_cond2dec and dec.nconds > 0)
    off = dec.nconds if c2d else 0
    pe_rows = dec.pe.pe.shape[1]
    if off + W - 1 > pe_rows or W > 256:
        raise ValueError(f"{W - 1} input tokens + {off} condition rows exceed the {pe_rows}-row positional table")
    return ys, lens, c2d, off, V


def _scoring_logits(model, z, src_mask, dconds, y, t0, pad_id, c2d):
    """The teacher-forced logits of the token rows y int64 [m, W] (on the device, prefix lengths t0 int64 [m] there too)
    as gct_seq_logp / gct_seq_logp_bwd take them: (logits [m * rows_per_seq, V], rows_per_seq), or None when no column of
    the batch is scored (no forward then).  The decoder gets loss_rows = every input row up to the sequence's last
    scored token (prefix rows included, so that the live rows stay a prefix): the rows behind it are not computed when
    the row planner accepts the map; a use_cond2dec model runs every row."""
    from .Model.modules import get_trg_mask
    dec = model.decoder
    W = y.shape[1]
    cols = torch.arange(W, device=y.device).view(1, -1)
    scored = (cols >= t0.view(-1, 1)) & (y != pad_id)
    last = (scored * cols).amax(1)                                  # a row's last scored column (0: none)
    if not bool(last.any()):
        return None
    trg = y[:, :-1].contiguous()
    trg_mask = get_trg_mask(trg, pad_id, c2d, dconds if dec.nconds > 0 else None)
    loss_rows = cols[:, :W - 1] < last.view(-1, 1)                  # input row c - 1 predicts token c
    logits = _teacher_forced_logits(model, trg, z, src_mask, trg_mask, dconds, loss_rows)
    rows = logits.shape[1]                                          # W - 1 (+ the condition rows of use_cond2dec)
    return logits.reshape(y.shape[0] * rows, logits.shape[-1]), rows


@torch.no_grad()
def score_tokens(model, z, src_mask, dconds, ys, prefix_lens=None, pad_id=1, chunk=512):
    """Teacher-forced log-likelihood of the token rows ys [n, W] (score_reference's layout and rule) under
    model.decode(ys[:, :-1], z, src_mask, ., dconds): z [n, L_e, latent], src_mask bool [n, 1, L_e], dconds [n, n_c] or
    None, as model.decode takes them.  Returns (logp [n] fp32, tokens [n] int32, hits [n] int32, token_logp [n, W] fp32)
    on the device.
    One decoder forward per `chunk` sequences, then gct_seq_logp straight on its logits.  The decoder gets loss_rows =
    every input row up to the sequence's last scored token (prefix rows included, so that the live rows stay a prefix):
    the rows behind it are not computed when the row planner accepts the map; a use_cond2dec model runs every row.
    ValueError before any device work for malformed inputs (check_score_inputs) and for rows beyond the positional
    table.  sequence_logp is the same computation with a gradient."""
    ys, lens, c2d, off, V = _score_geometry(model, ys, prefix_lens)
    if isinstance(chunk, bool) or not isinstance(chunk, numbers.Integral) or chunk < 1:
        raise ValueError(f"chunk must be an int >= 1, got {chunk!r}")
    n, W = ys.shape
    dev = z.device
    token_logp = torch.empty(n, W, device=dev)
    logp = torch.empty(n, device=dev)
    tokens = torch.empty(n, dtype=torch.int32, device=dev)
    hits = torch.empty(n, dtype=torch.int32, device=dev)
    for lo in range(0, n, int(chunk)):
        hi = min(n, lo + int(chunk))
        y = ys[lo:hi].to(dev, torch.int64).contiguous()
        t0 = lens[lo:hi].to(dev)
        out = (token_logp[lo:hi], logp[lo:hi], tokens[lo:hi], hits[lo:hi])
        dc = None if dconds is None else dconds[lo:hi].to(dev)
        sm = None if src_mask is None else src_mask[lo:hi].to(dev)
        got = _scoring_logits(model, z[lo:hi], sm, dc, y, t0, pad_id, c2d)
        if got is None:                                             # nothing to score: no forward
            for t in out:
                t.zero_()
            continue
        logits2d, rows = got
        ops.seq_logp(logits2d, y, None if prefix_lens is None else t0.to(torch.int32), pad_id, row_shift=off,
                     rows_per_seq=rows, out=out)
    return logp, tokens, hits, token_logp


def sequence_logp(model, z, src_mask, dconds, ys, prefix_lens=None, pad_id=1):
    """score_tokens with a gradient: the same inputs, the same rule, the same values bit for bit, and logp [n] /
    token_logp [n, W] attached to the autograd graph of the decoder's parameters, of model.out and -- when it requires
    grad -- of z.  Returns (logp, tokens, hits, token_logp) on the device; tokens / hits are counts and carry no
    gradient.  A per-molecule objective (REINFORCE, reward-weighted likelihood, the best k of a batch) is any function
    of logp; Train/finetune.py builds the policy-gradient step on it.
    ONE decoder forward over all n rows, no chunks -- the caller sizes n -- in the model's current train / eval mode
    (dropout is live under model.train()).  loss_rows is score_tokens' rule, so the rows behind a sequence's last scored
    token are computed neither forward nor backward when the row planner accepts the map; the backward
    (gct_seq_logp_bwd through engine.SeqLogpFn) writes exact zeros on every logits row that is not scored, so no
    gradient ever falls on a skipped row (ops.assert_no_skipped_row_gradients stays silent).  The encoder is not part of
    the graph: z is an input.
    ValueError before any device work for whatever check_score_inputs refuses, for rows beyond the positional table, and
    for a batch without a single scored column.  A single row with nothing scored is fine: value 0, gradient 0."""
    r = _policy_rows("sequence_logp", model, z, src_mask, dconds, ys, prefix_lens, pad_id, prior=None)
    logp, token_logp, tokens, hits = engine.SeqLogpFn.apply(r.logits2d, r.y, r.t0_dev, pad_id, r.off)
    return logp, tokens, hits, token_logp


class PolicyTerms(NamedTuple):
    """What sequence_policy returns, on the device: sequence_logp's four (logp [n], tokens [n] int32, hits [n] int32,
    token_logp [n, W]); entropy [n] / token_entropy [n, W] of the agent's next-token distributions at the scored columns
    (None with entropy=False); and with a prior kl [n] / token_kl [n, W] = KL(agent || prior) there and prior_logp [n],
    the prior's log-likelihood of the same tokens (None without one).  logp, token_logp, entropy, token_entropy, kl and
    token_kl carry the agent's graph; prior_logp carries none.  dist_reference states the rule of the new terms."""
    logp: torch.Tensor
    tokens: torch.Tensor
    hits: torch.Tensor
    token_logp: torch.Tensor
    entropy: Optional[torch.Tensor]
    token_entropy: Optional[torch.Tensor]
    kl: Optional[torch.Tensor]
    token_kl: Optional[torch.Tensor]
    prior_logp: Optional[torch.Tensor]


def _check_prior(model, prior, name="sequence_policy"):
    """A prior scores the agent's rows with the agent's geometry: the same vocabulary, condition count and
    use_cond2dec.  ValueError otherwise."""
    for what, a, b in (("vocabulary", model.out.weight.shape[0], prior.out.weight.shape[0]),
                       ("nconds", model.decoder.nconds, prior.decoder.nconds),
                       ("use_cond2dec", bool(model.decoder.use_cond2dec), bool(prior.decoder.use_cond2dec))):
        if a != b:
            raise ValueError(f"{name}: the prior's {what} ({b}) is not the model's ({a})")


class _PolicyRows(NamedTuple):
    """What sequence_policy and sequence_ppo share once the inputs are accepted and the agent's ONE forward has run, on
    the device: the token rows y, prefix lengths t0 (int64) / t0_dev (int32, None when the caller gave none), mask and
    conditions, use_cond2dec and the condition rows in front of a sequence's logits, the logits [n * rows, V]."""
    y: torch.Tensor
    t0: torch.Tensor
    t0_dev: Optional[torch.Tensor]
    sm: Optional[torch.Tensor]
    dc: Optional[torch.Tensor]
    c2d: bool
    off: int
    logits2d: torch.Tensor
    rows: int


def _policy_rows(name, model, z, src_mask, dconds, ys, prefix_lens, pad_id, prior, check=None):
    """sequence_policy's validation (ValueError before any device work; `check(n, W)` adds the caller's own), then the
    agent's one forward through _scoring_logits."""
    ys, lens, c2d, off, V = _score_geometry(model, ys, prefix_lens)
    if prior is not None:
        _check_prior(model, prior, name)
    n, W = ys.shape
    if check is not None:
        check(n, W)
    host = ys.detach().cpu()
    if not bool(((torch.arange(W).view(1, -1) >= lens.view(-1, 1)) & (host != pad_id))[:, 1:].any()):
        raise ValueError(f"{name}: no column of the batch is scored (every row is prefix or pad)")
    dev = z.device
    y = ys.to(dev, torch.int64).contiguous()
    t0 = lens.to(dev)
    dc = None if dconds is None else dconds.to(dev)
    sm = None if src_mask is None else src_mask.to(dev)
    t0_dev = None if prefix_lens is None else t0.to(torch.int32)
    logits2d, rows = _scoring_logits(model, z, sm, dc, y, t0, pad_id, c2d)
    return _PolicyRows(y, t0, t0_dev, sm, dc, c2d, off, logits2d, rows)


def _dist_terms(name, r, z, pad_id, prior, entropy):
    """The terms of sequence_policy beyond logp, on the rows r of _policy_rows: the prior's one forward under no_grad and
    its log-likelihood (gct_seq_logp), then engine.SeqDistFn on the agent's logits.  Returns (entropy, token_entropy, kl,
    token_kl, prior_logp), each None when not asked for."""
    prior2d = prior_logp = None
    if prior is not None:
        with torch.no_grad():
            prior2d, prior_rows = _scoring_logits(prior, z.detach(), r.sm, r.dc, r.y, r.t0, pad_id, r.c2d)
            if prior_rows != r.rows:
                raise ValueError(f"{name}: the prior gives {prior_rows} logits rows per sequence, the model {r.rows}")
            prior_logp = ops.seq_logp(prior2d, r.y, r.t0_dev, pad_id, row_shift=r.off, rows_per_seq=r.rows)[1]
    ent = tent = kl = tkl = None
    if entropy or prior is not None:
        ent, tent, kl, tkl = engine.SeqDistFn.apply(r.logits2d, prior2d, r.y, r.t0_dev, pad_id, r.off)
        if not entropy:
            ent = tent = None
    return ent, tent, kl, tkl, prior_logp


def sequence_policy(model, z, src_mask, dconds, ys, prefix_lens=None, pad_id=1, prior=None, entropy=True):
    """sequence_logp plus the terms that need the whole next-token distribution, from ONE agent forward: the entropy of
    the policy at every scored token and -- with `prior`, a second model of the same architecture (finetune.frozen_prior)
    -- KL(agent || prior) there and the prior's log-likelihood of the same tokens.  Returns a PolicyTerms; logp, tokens,
    hits and token_logp are sequence_logp's bit for bit (same inputs, same train / eval mode).
    The prior runs ONE forward under torch.no_grad(), in whatever mode it is in (the caller keeps it in eval()), with the
    agent's loss_rows, so the rows it skips are the agent's; prior_logp is gct_seq_logp on its logits.  entropy=False
    without a prior launches nothing beyond sequence_logp.  The backward of the new terms is gct_seq_dist_bwd through
    engine.SeqDistFn: exact zeros on every logits row that is not scored, as SeqLogpFn's, and autograd adds the two.
    ValueError before any device work for what sequence_logp refuses and for a prior whose vocabulary, nconds or
    use_cond2dec differ from the model's."""
    r = _policy_rows("sequence_policy", model, z, src_mask, dconds, ys, prefix_lens, pad_id, prior)
    logp, token_logp, tokens, hits = engine.SeqLogpFn.apply(r.logits2d, r.y, r.t0_dev, pad_id, r.off)
    ent, tent, kl, tkl, prior_logp = _dist_terms("sequence_policy", r, z, pad_id, prior, entropy)
    return PolicyTerms(logp, tokens, hits, token_logp, ent, tent, kl, tkl, prior_logp)


class PpoTerms(NamedTuple):
    """What sequence_ppo returns, on the device: PolicyTerms' nine fields -- logp [n], tokens [n] int32, hits [n] int32,
    token_logp [n, W] of the CURRENT policy; entropy / token_entropy (None with entropy=False); kl / token_kl /
    prior_logp (None without a prior) -- and PPO's: surrogate [n] / token_surrogate [n, W], the clipped surrogate of the
    probability ratios against old_token_logp; approx_kl [n], the k3 estimate of KL(old || new) summed over a row's
    scored tokens; clipped [n] int32, the row's clipped tokens.  surrogate, token_surrogate, entropy, token_entropy, kl
    and token_kl carry the agent's graph; logp, token_logp, approx_kl and the counts are reports and carry none (an
    objective in logp is sequence_logp's business).  ppo_reference states the rule of the new terms."""
    logp: torch.Tensor
    tokens: torch.Tensor
    hits: torch.Tensor
    token_logp: torch.Tensor
    entropy: Optional[torch.Tensor]
    token_entropy: Optional[torch.Tensor]
    kl: Optional[torch.Tensor]
    token_kl: Optional[torch.Tensor]
    prior_logp: Optional[torch.Tensor]
    surrogate: torch.Tensor
    token_surrogate: torch.Tensor
    approx_kl: torch.Tensor
    clipped: torch.Tensor


def sequence_ppo(model, z, src_mask, dconds, ys, old_token_logp, advantage, clip=0.2, prefix_lens=None, pad_id=1,
                 prior=None, entropy=False):
    """PPO's clipped surrogate of the token rows ys under the model, against the log-probabilities old_token_logp [n, W]
    the rows were sampled with (sequence_logp's / Sampling.score's token_logp of the sampling-time policy) and one
    advantage per row; clip: a number e (the ratio's trust region is [1 - e, 1 + e]) or a pair (clip_lo, clip_hi).
    Returns a PpoTerms from ONE agent forward: gct_seq_ppo on the teacher-forced logits gives the surrogate and, in the
    same launch, logp / tokens / hits / token_logp -- sequence_logp's bit for bit, but without a gradient --; with
    entropy=True or a prior, the entropy / KL terms exactly as sequence_policy computes them (same values bit for bit).
    old_token_logp and advantage get no gradient.  The backward is gct_seq_ppo_bwd through engine.SeqPpoFn: exact zeros on
    every logits row that is not scored (ops.assert_no_skipped_row_gradients stays silent) and on the rows of clipped
    tokens.  The model runs in its current train / eval mode; a ratio against a deterministic old policy wants eval()
    (Train/finetune.ppo_update).
    ValueError before any device work for what sequence_policy refuses and for what check_ppo_inputs does."""
    clip_lo, clip_hi = clip_pair(clip)
    adv = []
    r = _policy_rows("sequence_ppo", model, z, src_mask, dconds, ys, prefix_lens, pad_id, prior,
                     check=lambda n, W: adv.append(check_ppo_inputs(old_token_logp, advantage, clip_lo, clip_hi, n, W)))
    dev = z.device
    old = old_token_logp.detach().to(dev, torch.float32)
    a = adv[0].detach().to(dev, torch.float32)
    surrogate, token_surrogate, logp, token_logp, approx_kl, tokens, hits, clipped = engine.SeqPpoFn.apply(
        r.logits2d, r.y, r.t0_dev, pad_id, r.off, old, a, clip_lo, clip_hi)
    ent, tent, kl, tkl, prior_logp = _dist_terms("sequence_ppo", r, z, pad_id, prior, entropy)
    return PpoTerms(logp, tokens, hits, token_logp, ent, tent, kl, tkl, prior_logp, surrogate, token_surrogate,
                    approx_kl, clipped)


# ------------------------------------------------------------------------ importance-weighted marginal likelihoods
class Marginal(NamedTuple):
    """What marginal_logp returns, one entry per molecule: iwae [n] fp32 = logsumexp_k(log w_k) - log K, the
    importance-weighted lower bound of log p(x) (Burda et al.; the ELBO at K = 1, log p(x) as K grows), with
    log w_k = log p(x | z_k) + log p(z_k) - log q(z_k | x), z_k ~ q(z | x); elbo [n] = mean_k log w_k, the K-sample
    estimate of the ELBO; recon [n] = mean_k log p(x | z_k); ess [n] = (sum w)^2 / sum w^2, the effective sample size in
    [1, K] (near 1: one draw carries the estimate, raise K); tokens [n] int32 the scored tokens (score_tokens').
    With return_weights: log_w fp64 [n, K] = logp + logw, and its two parts logp [n, K] (the decoder's) and logw [n, K]
    (gct_latent_iw's log p(z) - log q(z | x)), both fp32."""
    iwae: torch.Tensor
    elbo: torch.Tensor
    recon: torch.Tensor
    ess: torch.Tensor
    tokens: Optional[torch.Tensor] = None
    log_w: Optional[torch.Tensor] = None
    logp: Optional[torch.Tensor] = None
    logw: Optional[torch.Tensor] = None


def _int_at_least_one(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError(f"{name} must be an int >= 1, got {v!r}")
    return int(v)


def latent_rows(src_mask, n, Le):
    """The latent rows each molecule owns, int64 [n] on the CPU, from src_mask bool [n, 1, Le] as the encoder and
    latent_setup_rows build it: the marked rows must be a non-empty prefix (condition rows, scaffold, <sep>, tokens).
    ValueError otherwise."""
    m = torch.as_tensor(src_mask)
    if tuple(m.shape) != (n, 1, Le):
        raise ValueError(f"src_mask must be [{n}, 1, {Le}], got {list(m.shape)}")
    m = m[:, 0].to("cpu").bool()
    rows = m.sum(1)
    if n and (int(rows.min()) < 1 or not torch.equal(m, torch.arange(Le).view(1, -1) < rows.view(-1, 1))):
        raise ValueError("src_mask must mark a non-empty prefix of every molecule's latent rows")
    return rows


def check_marginal_inputs(mu, log_var, src_mask, ys, K, chunk):
    """Validate a marginal-likelihood call: K and chunk ints >= 1; mu, log_var [n, Le, D] of one shape; src_mask
    [n, 1, Le] marking a non-empty prefix; ys [n, W].  ValueError otherwise.  Returns (K, chunk, rows int64 [n])."""
    K, chunk = _int_at_least_one("K", K), _int_at_least_one("chunk", chunk)
    if mu.dim() != 3 or tuple(log_var.shape) != tuple(mu.shape):
        raise ValueError(f"mu and log_var must be [n, Le, D] of one shape, got {list(mu.shape)} and {list(log_var.shape)}")
    n, Le, _ = mu.shape
    ys = torch.as_tensor(ys)
    if ys.dim() != 2 or ys.shape[0] != n:
        raise ValueError(f"ys must be [{n}, W], got {list(ys.shape)}")
    return K, chunk, latent_rows(src_mask, n, Le)


def marginal_blocks(n, K, chunk):
    """The blocks marginal_logp walks the n x K (molecule, draw) rows in, each of at most `chunk` rows:
    [(i0, i1, k0, k1)] = molecules i0 .. i1 - 1 x draws k0 .. k1 - 1.  Whole molecules x all K draws while K <= chunk;
    one molecule x ranges of k otherwise."""
    if K > chunk:
        return [(i, i + 1, k, min(K, k + chunk)) for i in range(n) for k in range(0, K, chunk)]
    m = chunk // K
    return [(i, min(n, i + m), 0, K) for i in range(0, n, m)]


def latent_iw_reference(mu, log_var, rows, eps):
    """THE statement of gct_latent_iw's arithmetic given the draws, in fp64: mu, log_var [n, Le, D], rows ints [n],
    eps [n, K, Le, D] standard normals -> (z [n, K, Le, D], logw [n, K]).  On a molecule's own rows t < rows[i]:
    z = mu + eps exp(log_var / 2) and logw = the sum of 0.5 ((eps - z)(eps + z) + log_var) = log N(z; 0, I) -
    log N(z; mu, exp(log_var)) (the log 2 pi terms cancel); beyond them z = 0 and nothing is added."""
    mu, lv = torch.as_tensor(mu).double().cpu(), torch.as_tensor(log_var).double().cpu()
    eps = torch.as_tensor(eps).double().cpu()
    n, Le, D = mu.shape
    if eps.dim() != 4 or eps.shape[0] != n or tuple(eps.shape[2:]) != (Le, D) or tuple(lv.shape) != (n, Le, D):
        raise ValueError(f"eps must be [{n}, K, {Le}, {D}] and log_var [{n}, {Le}, {D}], got {list(eps.shape)}, {list(lv.shape)}")
    rows = _int_vector("rows", rows, n, 1, Le, "the latent rows")
    own = (torch.arange(Le).view(1, -1) < rows.view(-1, 1)).view(n, 1, Le, 1)
    z = mu.unsqueeze(1) + eps * torch.exp(0.5 * lv).unsqueeze(1)
    term = 0.5 * ((eps - z) * (eps + z) + lv.unsqueeze(1))
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(own, z, zero), torch.where(own, term, zero).sum((2, 3))


def marginal_reference(logp, logw=None, mu=None, log_var=None, rows=None, eps=None):
    """THE statement of the importance-weighted estimate (gct_iw_combine implements it), in fp64 on the CPU.
    logp [n, K >= 1]: log p(x | z_k) of every draw; logw [n, K]: log p(z_k) - log q(z_k | x) -- or, with logw None,
    computed from the draws themselves: latent_iw_reference(mu, log_var, rows, eps), eps [n, K, Le, D].
    Returns Marginal(iwae, elbo, recon, ess, None, log_w) with a = logp + logw, m = max_k a:
      iwae = m + log(sum_k exp(a_k - m)) - log K      elbo = mean_k a_k      recon = mean_k logp_k
      ess  = (sum_k exp(a_k - m))^2 / sum_k exp(a_k - m)^2
    Jensen: elbo <= iwae <= max_k a_k for every molecule.  ValueError for K < 1 and mismatched shapes."""
    logp = torch.as_tensor(logp).double().cpu()
    if logp.dim() != 2 or logp.shape[1] < 1:
        raise ValueError(f"logp must be [n, K >= 1], got {list(logp.shape)}")
    if logw is None:
        if mu is None or log_var is None or rows is None or eps is None:
            raise ValueError("marginal_reference: logw, or (mu, log_var, rows, eps) to compute it from")
        logw = latent_iw_reference(mu, log_var, rows, eps)[1]
    logw = torch.as_tensor(logw).double().cpu()
    if tuple(logw.shape) != tuple(logp.shape):
        raise ValueError(f"logw must be {list(logp.shape)} like logp, got {list(logw.shape)}")
    K = logp.shape[1]
    a = logp + logw
    m = a.max(1, keepdim=True).values
    e = torch.exp(a - m)
    s1, s2 = e.sum(1), (e * e).sum(1)
    return Marginal(m.squeeze(1) + torch.log(s1) - math.log(K), a.sum(1) / K, logp.sum(1) / K, s1 * s1 / s2, None, a)


@torch.no_grad()
def marginal_logp(model, mu, log_var, src_mask, dconds, ys, prefix_lens=None, K=64, seed=0, items=None, chunk=4096,
                  pad_id=1, return_weights=False):
    """Importance-weighted estimate of log p(x) of the token rows ys [n, W] (score_tokens' layout and rule) under the
    VAE: K draws z_k ~ q(z | x) = N(mu, exp(log_var)) per molecule, mu / log_var [n, L_e, latent] the encoder's and
    src_mask bool [n, 1, L_e] its mask (a non-empty prefix of every molecule's rows), dconds [n, n_c] or None and
    prefix_lens as score_tokens takes them.  Returns a Marginal on the device (its docstring says what the numbers are).
    The number is log p(scored tokens | latent length, prefix, conditions): the prior is N(0, I) over the molecule's own
    latent rows, whose count is held at the encoder's; no term for the token length is added.
    The n x K rows are walked in marginal_blocks of at most `chunk` rows: per block ONE gct_latent_iw launch (the
    latents, written once, with log p(z) - log q(z | x) of each) and score_tokens on the block with the mask, conditions
    and token rows repeated per draw; at the end one gct_iw_combine.  The draws are keyed by (seed, items[i], k) --
    items ints [n] >= 0, default arange(n) --: a molecule's latents and logw are bit-identical whatever chunk, n or the
    order of the molecules.  ValueError before any device work for what check_marginal_inputs and score_tokens refuse."""
    K, chunk, rows = check_marginal_inputs(mu, log_var, src_mask, ys, K, chunk)
    ys, lens, _, _, _ = _score_geometry(model, ys, prefix_lens)
    n = mu.shape[0]
    items = torch.arange(n) if items is None else _int_vector("items", items, n, 0, 2 ** 31 - 1, "int32")
    if dconds is not None and dconds.shape[0] != n:
        raise ValueError(f"dconds must have {n} rows, got {list(dconds.shape)}")
    dev = mu.device
    mu, log_var = mu.float().contiguous(), log_var.float().contiguous()
    src_mask = torch.as_tensor(src_mask).to(dev)
    logp = torch.empty(n, K, device=dev)
    logw = torch.empty(n, K, device=dev)
    tokens = torch.empty(n, dtype=torch.int32, device=dev)
    for i0, i1, k0, k1 in marginal_blocks(n, K, chunk):
        Kc = k1 - k0
        z, lw, _ = ops.latent_iw(mu[i0:i1], log_var[i0:i1], rows[i0:i1], items[i0:i1], k0, Kc, seed)
        rep = lambda x: None if x is None else x[i0:i1].repeat_interleave(Kc, 0)       # noqa: E731
        lp, tk, _, _ = score_tokens(model, z, rep(src_mask), rep(dconds), rep(ys),
                                    None if prefix_lens is None else rep(lens), pad_id=pad_id)
        logp[i0:i1, k0:k1] = lp.view(-1, Kc)
        logw[i0:i1, k0:k1] = lw.view(-1, Kc)
        tokens[i0:i1] = tk.view(-1, Kc)[:, 0]
    iwae, elbo, recon, ess = ops.iw_combine(logp.view(-1), logw.view(-1), n, K)
    if not return_weights:
        return Marginal(iwae, elbo, recon, ess, tokens)
    return Marginal(iwae, elbo, recon, ess, tokens, logp.double() + logw.double(), logp, logw)


# ------------------------------------------------------------------------------------- continuous batching
def stream_schedule_reference(steps_needed, rows):
    """THE statement of the continuous-batching schedule (gct_stream_refill implements it on the device).
    steps_needed [N] ints >= 1: shared steps item i occupies a row; rows >= 1 decode rows.
      * shared step 0 starts with items 0 .. min(rows, N) - 1 in the rows of the same index;
      * after every shared step the rows whose item finished IN that step take the next unstarted items in ascending
        row order; a row that finds the pool empty is parked for good.
    Returns (row_of [N] int64, start_step [N] int64, makespan): item i runs in row row_of[i] during the shared steps
    start_step[i] .. start_step[i] + steps_needed[i] - 1; makespan = the number of shared steps until the last item
    is done.  An item with a prefix of t0 tokens that generates g tokens needs t0 + g - 1 steps (the step that
    consumes token j writes token j + 1)."""
    need = [int(x) for x in torch.as_tensor(steps_needed).view(-1).tolist()]
    rows = int(rows)
    if rows < 1:
        raise ValueError(f"rows must be at least 1, got {rows}")
    if need and min(need) < 1:
        raise ValueError("every item needs at least one step")
    n = len(need)
    row_of, start = torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)
    first = min(rows, n)
    row_of[:first] = torch.arange(first)
    busy = [(need[i], i) for i in range(first)]         # (steps run when the row's item is done, row): a heap pops the
    heapq.heapify(busy)                                 # rows in the order of the rule -- earlier step, then lower row
    nxt, makespan = first, 0
    while busy:
        end, r = heapq.heappop(busy)
        makespan = max(makespan, end)
        if nxt < n:
            row_of[nxt], start[nxt] = r, end
            heapq.heappush(busy, (end + need[nxt], r))
            nxt += 1
    return row_of, start, makespan


def check_stream_rows(rows):
    """1 <= rows <= ops.STREAM_MAX_ROWS (gct_stream_refill's scan is one workgroup); ValueError otherwise."""
    if isinstance(rows, bool) or not isinstance(rows, numbers.Integral):
        raise ValueError(f"rows must be an int, got {rows!r}")
    if not 1 <= rows <= ops.STREAM_MAX_ROWS:
        raise ValueError(f"rows {rows} outside [1, {ops.STREAM_MAX_ROWS}]")
    return int(rows)


def zattn_latent_ok(model, lat):
    """A latent of this width lets a step's cross-attention run over the latent rows themselves (gct_attn_decode_z)."""
    dec = model.decoder
    return bool(ZATTN and lat % 4 == 0 and lat <= 128 and dec.layers[0].attn_1.h * lat <= 2 * dec.d_model)


def check_stream_model(model, latent_dim=None):
    """Continuous batching needs a decoder whose condition rows do not live in the self-attention caches (they would
    come from prefill) and whose cross-attention reads the latent rows: ValueError for use_cond2dec models, for more
    layers than gct_stream_refill takes and, with latent_dim given, for a latent width gct_attn_decode_z does not take."""
    dec = model.decoder
    if latent_dim is not None and not zattn_latent_ok(model, int(latent_dim)):
        raise ValueError(f"continuous batching needs the cross-attention over the latent rows (gct_attn_decode_z): a "
                         f"latent of {latent_dim} keeps per-sequence K / V projections")
    if dec.use_cond2dec and dec.nconds > 0:
        raise ValueError("continuous batching does not support use_cond2dec models (their condition rows are written "
                         "into the caches by prefill)")
    if len(dec.layers) > ops.STREAM_MAX_LAYERS:
        raise ValueError(f"continuous batching supports up to {ops.STREAM_MAX_LAYERS} decoder layers")


def check_max_new_tokens(max_new_tokens, n, steps):
    """Per-item caps (ints [n], 1 <= cap <= steps) as an int64 CPU tensor; None: every item may generate `steps`
    tokens.  ValueError otherwise."""
    if max_new_tokens is None:
        return torch.full((n,), steps, dtype=torch.int64)
    return _int_vector("max_new_tokens", max_new_tokens, n, 1, steps, "max_strlen - 1")


def memory_masks(src_mask, n_cond_rows, Le):
    """Key flags of the cross-attention memory, sv uint8 [n, Lk] (n_cond_rows always-visible condition rows in front of
    the Le latent rows), and klen int32 [n]: the rows a step reads.  Visible rows that form a non-empty prefix (the padding
    masks of Inference/*_sampling.py) hide rows that weigh exactly 0, which gct_attn_decode does not read; any other
    mask keeps all Lk rows."""
    n = src_mask.shape[0]
    sv = ops.to_mask_u8(src_mask).view(n, Le)
    if n_cond_rows:
        sv = torch.cat([torch.ones(n, n_cond_rows, dtype=torch.uint8, device=sv.device), sv], dim=1)
    Lk = sv.shape[1]
    cnt = sv.sum(1, dtype=torch.int32)
    prefix = (sv[:, :-1] >= sv[:, 1:]).all(1) if Lk > 1 else torch.ones(n, dtype=torch.bool, device=sv.device)
    return sv, torch.where(prefix & (cnt > 0), cnt, torch.full_like(cnt, Lk))


# ------------------------------------------------------------------------------------- beam-search semantics
def check_beam_size(beam_size, vocab):
    """1 <= beam_size <= ops.BEAM_MAX_K and beam_size <= vocab (gct_beam_select's limits); ValueError otherwise."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int):
        raise ValueError(f"beam_size must be an int, got {beam_size!r}")
    if not 1 <= beam_size <= ops.BEAM_MAX_K:
        raise ValueError(f"beam_size {beam_size} outside [1, {ops.BEAM_MAX_K}]")
    if beam_size > vocab:
        raise ValueError(f"beam_size {beam_size} exceeds the vocabulary ({vocab} tokens)")
    if vocab > ops.BEAM_MAX_VOCAB:
        raise ValueError(f"beam search supports vocabularies up to {ops.BEAM_MAX_VOCAB} tokens, not {vocab}")


# --------------------------------------------------------------------------------- mixed prefix lengths
def check_prefix_lens(prefix_lens, n, width):
    """prefix_lens (ints [n], 1 <= t0_r <= width) as an int64 CPU tensor, or None when every row uses the full width
    (the uniform path); ValueError otherwise."""
    if prefix_lens is None:
        return None
    lens = _int_vector("prefix_lens", prefix_lens, n, 1, width, "the prefix width")
    return None if bool((lens == width).all()) else lens


def row_prefix_lens(lens, n, width):
    """check_prefix_lens' result with the uniform path spelled out: int64 [n] on the CPU, `width` for every row when
    lens is None."""
    return torch.full((n,), width, dtype=torch.int64) if lens is None else lens


def pad_behind_prefix(ys0, lens, pad_id):
    """ys0 [n, t0] with pad_id in the columns behind each row's prefix ys0[r, :lens[r]] (lens int64 [n] on the device
    of ys0): what a mixed-prefix decode reads, whatever the caller left there."""
    cols = torch.arange(ys0.shape[1], device=ys0.device).view(1, -1)
    return torch.where(cols < lens.view(-1, 1), ys0, torch.full_like(ys0, pad_id))


def generated_tokens(ys, prefix_lens):
    """The generated part of a mixed-prefix output ys [n, t0_max + G]: [n, G], row r = ys[r, t0_r : t0_r + G] (pad
    after the row's last step).  prefix_lens=None: ys[:, t0:] is the caller's slice."""
    lens = torch.as_tensor(prefix_lens, device=ys.device).long().view(-1, 1)
    g = ys.shape[1] - int(lens.max())
    return ys.gather(1, lens + torch.arange(g, device=ys.device).view(1, -1))


def beam_init(n, k, device=None):
    """State after the prefill: scores [n, k] = [0, -inf, ...] (the first expansion uses beam 0 only: every beam holds
    the same prefix), finished [n, k] False, lengths [n, k] 0 (generated tokens, <eos> included)."""
    scores = torch.full((n, k), -math.inf, dtype=torch.float32, device=device)
    scores[:, 0] = 0.0
    return scores, torch.zeros(n, k, dtype=torch.bool, device=device), torch.zeros(n, k, dtype=torch.int64, device=device)


def beam_log_softmax(logits):
    """fp32 log-softmax of the step's logits, x - m - log sum exp(x - m)."""
    y = logits.float() - logits.float().max(-1, keepdim=True).values
    return y - torch.log(torch.exp(y).sum(-1, keepdim=True))


def beam_candidates(scores, finished, logp, k, pad_id):
    """[n, k*V] candidate scores at flat index beam * V + token (-inf: not offered); see beam_step_reference."""
    n = scores.shape[0]
    V = logp.shape[-1]
    cand = scores.float().unsqueeze(-1) + logp.reshape(n, k, V).float()
    frozen = torch.full_like(cand, -math.inf)
    frozen[:, :, pad_id] = scores.float()
    return torch.where(finished.unsqueeze(-1), frozen, cand).reshape(n, k * V)


def beam_step_reference(scores, finished, lengths, logp, k, pad_id, eos_id):
    """One beam-search step, THE statement of the rules (gct_beam_select implements them on the device).
    scores [n, k] fp32, finished [n, k] bool, lengths [n, k] int, logp [n*k, V] (beam_log_softmax of the step's logits).
      * a live beam b offers score_b + logp_b(v) for every token v;
      * a finished beam offers exactly one candidate, itself with token pad_id and its score unchanged (frozen);
      * the k best candidates by score become the children, ties to the lower flat index b*V + token;
      * child: finished = parent.finished or token == eos_id; length = parent's + 1 while the parent was live.
    Returns (parent [n, k], token [n, k], scores, finished, lengths) of the children, best first."""
    V = logp.shape[-1]
    cand = beam_candidates(scores, finished, logp, k, pad_id)
    order = torch.sort(cand, dim=1, descending=True, stable=True).indices[:, :k]
    parent, token = order // V, order % V
    pfin = finished.gather(1, parent)
    return (parent, token, cand.gather(1, order), pfin | (token == eos_id),
            lengths.gather(1, parent) + (~pfin).to(lengths.dtype))


def beam_finalize(ys, scores, lengths, t0, alpha=BEAM_ALPHA):
    """Final ranking: beams sorted by score / length**alpha (ties to the lower beam), also when the length limit ended
    the search.  ys [n, k, L] (prefix of t0 tokens, pad after each beam's end) is cut to t0 + the longest beam.
    Returns (ys, scores, lengths) in that order."""
    norm = scores / lengths.clamp(min=1).to(scores.dtype) ** alpha
    order = torch.sort(norm, dim=1, descending=True, stable=True).indices
    ys = ys.gather(1, order.unsqueeze(-1).expand_as(ys))
    lengths = lengths.gather(1, order)
    return ys[:, :, :t0 + int(lengths.max())].contiguous(), scores.gather(1, order), lengths


# ------------------------------------------------------------------------------ stochastic beam search semantics
class SbsSamples(NamedTuple):
    """What a stochastic beam decode returns: ys int64 [n, k, L] (prefix, tokens, pad after each beam's end), logp
    [n, k] fp32 = log p(beam's tokens | latent, conditions, prefix), gumbel [n, k] fp32 the perturbed log-probabilities
    the beams were drawn by, lengths [n, k] int64 generated tokens (<eos> included).  The k beams of a sample are
    distinct and in drawing order (descending gumbel): beam 0 alone is an ordinary sample of the model."""
    ys: torch.Tensor
    logp: torch.Tensor
    gumbel: torch.Tensor
    lengths: torch.Tensor


def sbs_init(n, k, device=None, root=None):
    """State after the prefill: (scores, gumbels, finished, lengths), scores and gumbels [n, k] = [0, -inf, ...] (the
    first expansion uses beam 0 only: the root of the tree), the rest as in beam_init.
    root ([n], optional): the root's Gumbel value, gumbels[:, 0].  WHICH sequences are drawn, and in which order, does
    not depend on it (the order of an exponential race is independent of its first arrival time), so 0 samples
    correctly; but every other Gumbel value is conditioned on it, and sbs_importance_weights is unbiased only when the
    root is a Gumbel(0) variate itself (sbs_root_gumbels; with the root fixed at 0 the toy model of tests/test_sbs_host.py
    gives E[sum w] = 0.970 instead of 1).  generate_sbs draws it."""
    scores, finished, lengths = beam_init(n, k, device)
    gumbels = scores.clone()
    if root is not None:
        gumbels[:, 0] = root.to(gumbels)
    return scores, gumbels, finished, lengths


def sbs_root_gumbels(n, seed, device=None):
    """The root's Gumbel(0) variate of each of n samples under `seed`, fp32 [n]: -log(-log(u)) of torch's CPU generator
    seeded with seed (u in float64, clamped inside (0, 1)); sample s's value does not depend on n."""
    u = torch.rand(n, generator=torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF), dtype=torch.float64)
    return (-torch.log(-torch.log(u.clamp(1e-300, 1.0 - 2.0 ** -53)))).float().to(device)


def log1mexp(d):
    """log(1 - exp(d)) for d <= 0: log(-expm1(d)) above -ln 2, log1p(-exp(d)) below (Maechler 2012)."""
    return torch.where(d > -math.log(2.0), torch.log(-torch.expm1(d)), torch.log1p(-torch.exp(d)))


def sbs_candidates(scores, gumbels, finished, logp, noise, k, pad_id):
    """(value, phi), each [n, k*V] at flat index beam * V + token: the candidate's conditioned Gumbel value g~ (-inf: not
    offered) and its score; see sbs_step_reference.  Computed in the promoted dtype of the inputs."""
    n, V = scores.shape[0], logp.shape[-1]
    dt = functools.reduce(torch.promote_types, (gumbels.dtype, logp.dtype, noise.dtype), scores.dtype)
    sc, G = scores.to(dt).unsqueeze(-1), gumbels.to(dt).unsqueeze(-1)
    at = sc > -math.inf                                          # a beam at -inf offers nothing
    live = at & ~finished.unsqueeze(-1)
    phi = sc + logp.reshape(n, k, V).to(dt)
    offered = live & (phi > -math.inf)
    zero, ninf = torch.zeros((), dtype=dt, device=phi.device), torch.full((), -math.inf, dtype=dt, device=phi.device)
    g = torch.where(offered, phi + noise.reshape(n, k, V).to(dt), ninf)
    Z = g.max(-1, keepdim=True).values
    tok = torch.arange(V, device=phi.device).expand_as(g)
    vstar = torch.where((g == Z) & offered, tok, V).min(-1, keepdim=True).values       # FIRST argmax; V: nothing offered
    gs, Zs, Gs = torch.where(offered, g, zero), torch.where(Z > -math.inf, Z, zero), torch.where(at, G, zero)
    w = Gs - gs + log1mexp((gs - Zs).clamp(max=0.0))
    val = Gs - w.clamp(min=0.0) - torch.log1p(torch.exp(-w.abs()))
    val = torch.where(tok == vstar, Gs.expand_as(val), val)      # by index, exactly
    val = torch.where(offered, val, ninf)
    frozen = at & finished.unsqueeze(-1) & (tok == pad_id)       # a finished beam: itself, once
    val = torch.where(frozen, G.expand_as(val), val)
    phi = torch.where(frozen, sc.expand_as(phi), phi)
    return val.reshape(n, k * V), phi.reshape(n, k * V)


def sbs_step_reference(scores, gumbels, finished, lengths, logp, noise, k, pad_id, eos_id):
    """One step of stochastic beam search (Kool, van Hoof and Welling 2019), THE statement of the rules
    (gct_beam_select_gumbel implements them on the device).  scores / gumbels [n, k] (log-probability and Gumbel value
    of each beam), finished [n, k] bool, lengths [n, k] int, logp [n*k, V] (beam_log_softmax of the step's logits),
    noise [n*k, V] standard Gumbel variates.
      * a live beam b with finite scores[b] offers every token v with finite phi_bv = scores[b] + logp_b(v); its
        perturbed value is g_bv = phi_bv + noise_bv; Z_b = max_v g_bv and v*_b is its first argmax;
      * the candidate's value is g~_bv = -log(exp(-G_b) - exp(-Z_b) + exp(-g_bv)), G_b = gumbels[b] -- the g_bv
        conditioned on their maximum being G_b -- evaluated as d = min(g - Z, 0), l = log1mexp(d), w = G - g + l,
        g~ = G - max(w, 0) - log1p(exp(-|w|)); token v*_b gets g~ = G_b exactly, by its index;
      * a token with phi = -inf is not offered; a finished beam offers itself once, token pad_id, score and Gumbel value
        unchanged; a beam at -inf offers nothing;
      * the k candidates of largest g~ become the children in that order, ties to the lower flat index b*V + token;
      * child: scores = phi, gumbels = g~, finished and lengths by beam_step_reference's rule.  A slot c that no candidate
        is left for (fewer than k offered) becomes a finished beam at -inf: parent c, token pad_id.
    Returns (parent [n, k], token [n, k], scores, gumbels, finished, lengths) of the children, in drawing order."""
    V = logp.shape[-1]
    val, phi = sbs_candidates(scores, gumbels, finished, logp, noise, k, pad_id)
    order = torch.sort(val, dim=1, descending=True, stable=True).indices[:, :k]
    gum = val.gather(1, order)
    empty = gum == -math.inf
    slot = torch.arange(k, device=order.device).expand_as(order)
    parent = torch.where(empty, slot, order // V)
    token = torch.where(empty, torch.full_like(order, pad_id), order % V)
    pfin = finished.gather(1, parent)
    sc = torch.where(empty, gum, phi.gather(1, order))
    return (parent, token, sc, gum, pfin | (token == eos_id) | empty, lengths.gather(1, parent) + (~pfin).to(lengths.dtype))


def sbs_importance_weights(scores, gumbels):
    """Importance weights of a stochastic beam sample: scores / gumbels [n, k], sorted by Gumbel value as the decode
    returns them.  kappa = the k-th (smallest) Gumbel value of the sample; w_i = p_i / q_i(kappa) with p_i = exp(scores_i)
    and q_i = 1 - exp(-exp(scores_i - kappa)) (through expm1) for the first k - 1 beams, 0 for the last.
    Returns (w, w_normalised), each [n, k].  The FIRST is the unbiased one: E[sum_i w_i f(y_i)] = E_p[f] exactly; the second,
    w / sum w per sample, is biased but of lower variance (the paper's normalised estimator).  k = 1 has no estimator
    (no threshold is left): ValueError."""
    if scores.dim() != 2 or scores.shape != gumbels.shape:
        raise ValueError(f"sbs_importance_weights: scores {list(scores.shape)} and gumbels {list(gumbels.shape)} must be "
                         "the same [n, k]")
    if scores.shape[1] < 2:
        raise ValueError("sbs_importance_weights: k = 1 has no estimator (the k-th Gumbel value is the threshold)")
    kappa = gumbels[:, -1:]
    ok = scores > -math.inf                                      # (a slot at -inf: the sample ran out of sequences)
    q = -torch.expm1(-torch.exp(torch.where(ok, scores, torch.zeros_like(scores)) - kappa))
    w = torch.where(ok, torch.exp(scores) / q, torch.zeros_like(scores))
    w = torch.cat([w[:, :-1], torch.zeros_like(w[:, -1:])], dim=1)
    return w, w / w.sum(1, keepdim=True)


# ------------------------------------------------------------------------------ sequential Monte Carlo semantics
class SmcSamples(NamedTuple):
    """What a sequential Monte Carlo decode returns, k weighted particles per sample: ys int64 [n, k, L] (prefix, tokens,
    pad after each particle's end); logw [n, k] fp32 the particles' log-weights, normalised (logsumexp over k is 0);
    logp [n, k] fp32 = log p(particle's tokens | latent, conditions, prefix) under the model; log_z [n] fp64 = log Z^,
    the final log mean weight included -- exp(log_z) is an unbiased estimate of P(well formed within the budget);
    lengths [n, k] int64 generated tokens (<eos> included); ess [n] fp32 the effective sample size of the final weights;
    resamples [n] int64 how often the sample resampled.  The weighted particles sum_i exp(logw_i) delta(ys_i) converge to
    the model's own distribution restricted to well-formed strings as k grows; they are NOT distinct."""
    ys: torch.Tensor
    logw: torch.Tensor
    logp: torch.Tensor
    log_z: torch.Tensor
    lengths: torch.Tensor
    ess: torch.Tensor
    resamples: torch.Tensor


def check_ess_threshold(ess_threshold):
    """A real in [0, 1] (0: never resample, 1: always); ValueError otherwise.  Returns it as a float."""
    if isinstance(ess_threshold, bool) or not isinstance(ess_threshold, numbers.Real) or \
            not 0.0 <= float(ess_threshold) <= 1.0:
        raise ValueError(f"ess_threshold must be a real in [0, 1], got {ess_threshold!r}")
    return float(ess_threshold)


def check_particles(k, who="generate_smc"):
    """1 <= k <= ops.BEAM_MAX_K particles per sample (gct_smc_select's limit); ValueError otherwise."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= ops.BEAM_MAX_K:
        raise ValueError(f"{who}: k must be an int in [1, {ops.BEAM_MAX_K}] particles per sample, got {k!r}")
    return int(k)


def smc_init(n, k, device=None):
    """State after the prefill: (logw [n, k] fp32 0, logp [n, k] fp32 0, finished [n, k] False, lengths [n, k] int64 0,
    log_z [n] fp64 0, resamples [n] int64 0).  Every particle is live from the start -- there is no [0, -inf, ...] root:
    the k copies of the prefix draw their first tokens independently."""
    z = lambda *sh, dt: torch.zeros(*sh, dtype=dt, device=device)          # noqa: E731
    return (z(n, k, dt=torch.float32), z(n, k, dt=torch.float32), z(n, k, dt=torch.bool), z(n, k, dt=torch.int64),
            z(n, dt=torch.float64), z(n, dt=torch.int64))


def _systematic(w, u):
    """(ancestors [n, k], cum [n, k], thr [n, k], S1 [n]) of systematic_resample_reference."""
    n, k = w.shape
    S1, cums = torch.zeros(n, dtype=w.dtype, device=w.device), []
    for b in range(k):                                           # the fixed order b = 0 .. k-1
        S1 = S1 + w[:, b]
        cums.append(S1)
    cum = torch.stack(cums, 1)
    idx = torch.arange(k, device=w.device)
    thr = (u.to(w.dtype).view(n, 1) + idx.to(w.dtype).view(1, k)) * (S1 / k).view(n, 1)
    pos = w > 0
    hit = (cum.view(n, 1, k) > thr.view(n, k, 1)) & pos.view(n, 1, k)           # [sample, child, ancestor]
    last = torch.where(pos, idx.view(1, k), torch.zeros_like(idx).view(1, k)).max(1).values
    anc = torch.where(hit.any(-1), hit.int().argmax(-1), last.view(n, 1).expand(n, k))
    return anc, cum, thr, S1


def systematic_resample_reference(w, u):
    """Systematic resampling, THE statement of the rule (gct_smc_select implements it): w [n, k] weights >= 0 (not
    normalised, at least one positive per sample), u [n] one uniform in (0, 1] per sample.  cum_b = w_0 + .. + w_b summed
    in the order b = 0 .. k-1; child c takes the first b with cum_b > (u + c) * (S1 / k) and w_b > 0, otherwise the last
    b with w_b > 0.  Ancestor b gets floor or ceil of k w_b / S1 children, a particle of weight 0 none, and the ancestors
    come out in ascending order.  Returns ancestors int64 [n, k].  Computed in w's dtype."""
    return _systematic(w, u)[0]


def smc_step_reference(logw, logp, finished, lengths, logits, masked, u, k, pad_id, eos_id, tau, log_z, resamples,
                       info=None):
    """One step of sequential Monte Carlo under the grammar, THE statement of the rules (gct_smc_select implements them
    on the device).  Per sample k particles: logw [n, k] log-weights since the last resampling, logp [n, k]
    log-probabilities of their tokens under the model, finished [n, k] bool, lengths [n, k] int; logits [n*k, V] the raw
    rows of the step and masked [n*k, V] the same with -inf where the grammar or the length budget forbids the token;
    u [n, k + 1] uniforms in (0, 1] -- column c < k child c's draw, column k the resampling; tau the ESS threshold in
    [0, 1]; log_z [n] fp64 and resamples [n] int the sample's accumulators.
      0. a sample whose particles are all finished on entry is idle: a_c = c, pad tokens, nothing else changes;
      1. weight: a live particle b gets logw_b += (my - mx) + (log sy - log sx), (m, s) = (max, sum exp(. - max)) of its
         raw (x) and masked (y) row -- the log of the model's mass A on the allowed tokens; a finished one keeps logw_b;
         a masked row with no finite entry gives -inf: the particle is dead -- never an ancestor, it writes pad and is
         finished from then on;
      2. resample: M = max_b logw_b.  M = -inf (every particle dead): log_z = -inf, a_c = c.  Otherwise w_b =
         exp(logw_b - M), S1 = sum w, S2 = sum w^2 (b ascending), ESS = S1^2 / S2, and the sample resamples iff tau >= 1
         or ESS < tau * k: ancestors a_c by systematic_resample_reference(w, u[:, k]), log_z += M + log(S1 / k), every
         child's logw = 0, resamples += 1.  Without resampling a_c = c and the child keeps logw_c;
      3. draw: child c of a live parent a takes the first token v with softmax(y_a)_v > 0 whose inclusive cumulative sum
         exceeds u[:, c] (none: the last token of nonzero probability) -- gct_select_token's multinomial draw;
         logp_c = logp_a + ((x_a[v] - mx_a) - log sx_a), finished = v == eos_id, lengths = lengths_a + 1.  A finished or
         dead parent hands down pad_id and its state (a dead one: logw = -inf, finished).
    The weight does not depend on the token drawn, so weighting and resampling come before the draw (the fully adapted
    particle filter): copies of one ancestor diverge at this very step.  With gamma_t(x_<=t) = pi(x_<=t) 1[the prefix
    can still finish], gamma_t / (gamma_{t-1} q_t) = A_t, hence E[exp(log_z) * mean_b exp(logw_b)] = Z for every k and tau.
    Computed in the promoted dtype of logw and logits.  info (a dict, optional) receives ess [n], resampled [n],
    ess_margin [n] = |ESS - tau k|, sys_gap [n] (distance of the nearest systematic position to a cumulative boundary of
    a positive weight; inf without resampling), probs [n, k, V] the children's draw distributions (0 rows where no draw
    is made) and drew [n, k].
    Returns (ancestor [n, k], token [n, k], logw, logp, finished, lengths, log_z, resamples) of the children."""
    n, V = logw.shape[0], logits.shape[-1]
    dt, dev = torch.promote_types(logw.dtype, logits.dtype), logits.device
    ninf, zero = torch.full((), -math.inf, dtype=dt, device=dev), torch.zeros((), dtype=dt, device=dev)
    x, y = logits.reshape(n, k, V).to(dt), masked.reshape(n, k, V).to(dt)
    mx, my = x.max(-1).values, y.max(-1).values
    sx = torch.exp(x - mx.unsqueeze(-1)).sum(-1)
    some = my > -math.inf                                        # the masked row allows a token
    mys = torch.where(some, my, zero)
    sy = torch.where(some, torch.exp(torch.where(some.unsqueeze(-1), y, zero) - mys.unsqueeze(-1)).sum(-1), zero + 1)
    live = ~finished
    lw = logw.to(dt)
    lw = torch.where(live & some, lw + ((mys - mx) + (torch.log(sy) - torch.log(sx))), lw)
    lw = torch.where(live & ~some, ninf, lw)
    idle = finished.all(1)
    M = lw.max(1).values
    all_dead = (M == -math.inf) & ~idle
    w = torch.where((M > -math.inf).view(n, 1), torch.exp(lw - torch.where(M > -math.inf, M, zero).view(n, 1)), zero)
    S2 = torch.zeros(n, dtype=dt, device=dev)
    for b in range(k):
        S2 = S2 + w[:, b] * w[:, b]
    anc_sys, cum, thr, S1 = _systematic(w, u[:, k])
    weighted = ~idle & ~all_dead
    ess = torch.where(weighted, S1 * S1 / torch.where(weighted, S2, zero + 1), zero)
    res = weighted & ((ess < float(tau) * k) | (float(tau) >= 1.0))
    own = torch.arange(k, device=dev).view(1, k).expand(n, k)
    anc = torch.where(res.view(n, 1), anc_sys, own)
    gain = M.double() + torch.log(torch.where(weighted, S1, zero + 1).double() / k)
    log_z = torch.where(res, log_z.double() + gain, log_z.double())
    log_z = torch.where(all_dead, torch.full_like(log_z, -math.inf), log_z)
    resamples = resamples + res.to(resamples.dtype)
    cw = torch.where(res.view(n, 1), zero, lw)
    pfin, plw = finished.gather(1, anc), lw.gather(1, anc)
    dead = ~pfin & (plw == -math.inf)
    drew = ~pfin & ~dead
    row = anc.unsqueeze(-1).expand(n, k, V)
    xa, ya = x.gather(1, row), y.gather(1, row)
    prob = torch.exp(torch.where(drew.unsqueeze(-1), ya, ninf) - mys.gather(1, anc).unsqueeze(-1)) / \
        sy.gather(1, anc).unsqueeze(-1)
    nz = prob > 0
    tokens = torch.arange(V, device=dev)
    hit = nz & (prob.cumsum(-1) > u[:, :k].to(dt).unsqueeze(-1))
    lastnz = torch.where(nz, tokens, torch.zeros_like(tokens)).max(-1).values
    tok = torch.where(hit.any(-1), hit.int().argmax(-1), lastnz)
    tok = torch.where(drew, tok, torch.full_like(tok, pad_id))
    step_lp = (xa.gather(2, tok.unsqueeze(-1)).squeeze(-1) - mx.gather(1, anc)) - torch.log(sx.gather(1, anc))
    lp = logp.to(dt).gather(1, anc) + torch.where(drew, step_lp, zero)
    if info is not None:
        edge = torch.where((w > 0).view(n, 1, k), (cum.view(n, 1, k) - thr.view(n, k, 1)).abs(), zero + math.inf)
        info.update(ess=ess, resampled=res, ess_margin=(ess - float(tau) * k).abs(), probs=prob, drew=drew,
                    sys_gap=torch.where(res, edge.reshape(n, -1).min(1).values, zero + math.inf))
    return (anc, tok, torch.where(dead, ninf, cw), lp, torch.where(drew, tok == eos_id, torch.ones_like(drew)),
            lengths.gather(1, anc) + drew.to(lengths.dtype), log_z, resamples)


def smc_finalize(logw, log_z):
    """(normalised logw [n, k], log_z [n] fp64 with the final log mean weight, ess [n]) of the weights a decode ends
    with: logw - logsumexp(logw), log_z + logsumexp(logw) - log k, and (sum w)^2 / sum w^2.  A sample whose particles all
    died (log_z = -inf) keeps logw = -inf and has ess 0."""
    k = logw.shape[1]
    lse = torch.logsumexp(logw.double(), 1)
    ok = lse > -math.inf
    norm = torch.where(ok.view(-1, 1), logw.double() - torch.where(ok, lse, torch.zeros_like(lse)).view(-1, 1),
                       logw.double())
    ess = torch.where(ok, 1.0 / torch.exp(2.0 * norm).sum(1).clamp(min=1e-300), torch.zeros_like(lse))
    return norm.to(logw.dtype), log_z.double() + lse - math.log(k), ess.float()


def smc_row_weights(samples):
    """The particles' weights as per-row factors of a policy-gradient step: k * exp(logw) flattened to [n*k] in the
    sample-major row order of DecodedRows (mean 1 per sample), for Train/finetune.reinforce_step(..., weight=) /
    ppo_update(..., weight=)."""
    k = samples.logw.shape[1]
    return (k * torch.exp(samples.logw.float())).reshape(-1)


class KVDecoder:
    def __init__(self, model, pad_id: int, sos_id: int, eos_id: int):
        dec = model.decoder
        self.model, self.dec = model, dec
        self.pad_id, self.sos_id, self.eos_id = int(pad_id), int(sos_id), int(eos_id)
        self.d = dec.d_model
        self.H = dec.layers[0].attn_1.h
        self.dk = self.d // self.H
        self.c2d = bool(dec.use_cond2dec and dec.nconds > 0)
        self.off = dec.nconds if self.c2d else 0          # cache / positional index of token 0
        self.graphs = {}
        self.graph_replay = True
        self.replay_probe = None                          # numbers of the replay guard (after the first capture)
        self._fold_key = None                             # what the cached folded projections were computed from
        self._shape = None
        self.stream = None                                # continuous batching: pool + StreamState (start_stream)

    # -------------------------------------------------------------------------------------
    @torch.no_grad()
    def start(self, z, src_mask, dconds=None, max_total_len=208, refold=False, beams=1):
        """z [n, L_e, latent]; src_mask bool [n,1,L_e] (as the reference builds it); max_total_len = longest
        token sequence (prefix + generated) this call may reach.
        beams=k > 1 (for generate_beam): latent, masks and dconds are replicated per beam, the decode runs n*k rows.
        refold=True recomputes the folded cross-attention projections even if `model.weights_token()` has not changed:
        the token follows torch in-place operations on the parameters / the flat buffer and FusedAdam's kernel, but NOT
        writes through `p.data` (p.data.copy_ / mul_: a separate version counter) or raw kernels of the caller's own --
        such writers call model.invalidate_weight_planes() (which bumps the token) or pass refold=True here."""
        if refold:
            self._fold_key = None
        dec, d = self.dec, self.d
        beams = int(beams)
        if beams != 1:
            check_beam_size(beams, self.model.out.weight.shape[0])
            z, src_mask = z.repeat_interleave(beams, 0), src_mask.repeat_interleave(beams, 0)
            dconds = None if dconds is None else dconds.repeat_interleave(beams, 0)
        dev = z.device
        n, Le, lat = z.shape
        if hasattr(self.model, "refresh_weight_planes"):
            self.model.refresh_weight_planes()         # the prefill GEMMs may take the bf16x6 path
        nc = dec.nconds
        c2l = (not self.c2d) and dec.use_cond2lat and nc > 0
        self.z, self.src_mask_in, self.dconds = z, src_mask, dconds
        self.zattn = self._zattn_ok(lat, Le)
        z2 = z.reshape(n * Le, lat).float().contiguous()
        Lk, e = Le, None
        if not self.zattn:
            e = ez = torch.empty(n * Le, d, device=dev)
            ops.linear_fwd(z2, [dec.fc_z.weight], [dec.fc_z.bias], [ez], d)
        sv, klen = memory_masks(src_mask, nc if c2l else 0, Le)
        if c2l:
            Lk = Le + nc
            cl = ops.small_linear_fwd(dconds.float().contiguous(), dec.embed_cond2lat.weight,
                                      dec.embed_cond2lat.bias)
            if not self.zattn:
                e = torch.empty(n * Lk, d, device=dev)
                ops.copy_rows(cl, nc, 0, e, Lk, 0, n * nc, nc, d)
                ops.copy_rows(ez, Le, 0, e, Lk, nc, n * Le, Le, d)
        T = int(max_total_len) + self.off              # cache rows: condition tokens (cond2dec) + tokens
        if T > 256 or Lk > 256:
            raise ValueError("decode lengths above 256 are not supported by gct_attn_decode")
        pe_rows = dec.pe.pe.shape[1]
        if T > pe_rows:
            # the positional table has pe_rows rows (Model/modules.py:116-144: 200); the reference fails loudly past it
            raise ValueError(f"decode: {max_total_len} tokens + {self.off} condition rows exceed the {pe_rows}-row "
                             "positional table")
        shape = (n, Lk, T, str(dev), self.zattn, lat, beams)
        if shape != self._shape:
            # new geometry: new buffers, and the graphs captured against the old ones are dropped with them
            # (they hold raw pointers: replaying them after a reallocation would write freed memory)
            self.graphs = {}
            self.graph_replay = True
            self._shape = shape
            self.n, self.Lk, self.T = n, Lk, T
            self.nz = self.H * lat                     # width of the folded query / latent context (zattn)
            self.nq = (d if c2l else 0) + self.nz
            if self.zattn:
                # folded projections of all layers in ONE flat buffer (its bf16 planes serve the bf16x6 GEMMs)
                per = 2 * self.nq * d
                self.zflat = torch.empty(len(dec.layers) * per, device=dev)
                self._fold_key = None                      # new buffers: nothing folded in them yet
                self.zq_w = [self.zflat[i * per:i * per + self.nq * d].view(self.nq, d) for i in range(len(dec.layers))]
                self.zo_w = [self.zflat[i * per + self.nq * d:(i + 1) * per].view(d, self.nq) for i in range(len(dec.layers))]
                self.zq_b = [torch.empty(self.nq, device=dev) for _ in dec.layers]
                self.zo_b = [torch.empty(d, device=dev) for _ in dec.layers]
                self.ckv = [torch.empty(n * nc, 2 * d, device=dev) if c2l else None for _ in dec.layers]
                self.z3 = torch.empty(n, Le, lat, device=dev)     # captured graphs read the latent rows from here
                self.zplanes = None
                self.cross_kv = None
            else:
                self.cross_kv = [torch.empty(n * Lk, 2 * d, device=dev) for _ in dec.layers]
            self.kc = [torch.empty(n, T, d, device=dev) for _ in dec.layers]
            self.vc = [torch.empty(n, T, d, device=dev) for _ in dec.layers]
            self.valid = torch.zeros(n, T, dtype=torch.uint8, device=dev)
            self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.ys = torch.full((n, T), self.pad_id, dtype=torch.int64, device=dev)
            self.tok_logp = torch.zeros(n, T, device=dev)                  # return_logp: laid out like ys
            self.src_valid = torch.empty(n, Lk, dtype=torch.uint8, device=dev)
            self.src_klen = torch.empty(n, dtype=torch.int32, device=dev)  # leading memory rows the cross-attention reads
            self.pos = torch.zeros(1, dtype=torch.int32, device=dev)       # token index the next step consumes
            self.row_off = torch.zeros(n, dtype=torch.int32, device=dev)   # mixed prefixes: row r is at pos - row_off[r]
            self.seed = torch.zeros(1, dtype=torch.int64, device=dev)      # multinomial seed of this generate()
            self.filt = torch.zeros(4, dtype=torch.int32, device=dev)      # GctSampleFilter of this generate()
            self.gram = self.gtable = None                                 # grammar buffers: the first _set_sampling with one
            self.stats_tab = None                                          # return_stats: the first call that asks for them
            # beam search state (generate_beam), per row: score, finished, length, parent; the ancestry map; done [n/k]
            self.beams = beams
            self.bscores = torch.zeros(n, device=dev)
            self.bgumbel = torch.zeros(n, device=dev)                      # generate_sbs: the rows' Gumbel values
            self.bfin = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.blen = torch.zeros(n, dtype=torch.int32, device=dev)
            self.bparent = torch.zeros(n, dtype=torch.int32, device=dev)
            self.kv_src = torch.zeros(n, T, dtype=torch.int32, device=dev)
            self.bdone = torch.zeros(n // beams, dtype=torch.uint8, device=dev)
            # generate_smc: bscores holds the particles' log-weights; their log-probabilities, and per sample log Z^,
            # the resampling count and (one word, read by the kernel) the ESS threshold
            self.blogp = torch.zeros(n, device=dev)
            self.blogz = torch.zeros(n // beams, dtype=torch.float64, device=dev)
            self.bres = torch.zeros(n // beams, dtype=torch.int32, device=dev)
            self.btau = torch.zeros(1, device=dev)
            dff =dec.layers[0].ff.linear_1.weight.shape[0]
            V = self.model.out.weight.shape[0]
            need = ops._L().gct_linear_fwd_ws_bytes
            shapes = [(dff, d), (d, 3 * d), (d, dff), (d, d), (d, V)]           # (K, N) of every GEMM of a step
            if self.zattn:
                shapes += [(d, self.nq), (self.nq, d)]                         # the folded cross-attention projections
            wsb = max(need(n, k_, n_) for k_, n_ in shapes)
            self.ws = torch.empty(wsb // 4 + 64, device=dev)           # split-K / tail slabs of the step's GEMMs
            # few rows: the skinny split-K kernels; many rows (n >= 1024): the general path, i.e. the bf16x6 kernels
            self.gemm_kw = dict(splitk_ws=self.ws) if n < SKINNY_BELOW else dict(ws=self.ws)
            f = lambda *sh: torch.empty(*sh, device=dev)                # noqa: E731
            qw = self.nq if self.zattn else d
            self.buf = dict(x=f(n, d), x2=f(n, d), qkv=f(n, 3 * d), o=f(n, d), xa=f(n, d), q2=f(n, qw), o2=f(n, qw),
                            xb=f(n, d), pre=f(n, dff), hdn=f(n, dff), xc=[f(n, d), f(n, d)], y=f(n, d),
                            logits=f(n, V))
        self.src_valid.copy_(sv)
        self.src_klen.copy_(klen)
        if self.zattn:
            self.z3.copy_(z2.view(n, Le, lat))
            self._fold_cross(cl.view(n * nc, d) if c2l else None)
            return
        for li, layer in enumerate(dec.layers):                    # cross K/V: once per sequence
            kv, a = self.cross_kv[li], layer.attn_2
            ops.linear_fwd(e, [a.k_linear.weight, a.v_linear.weight], [a.k_linear.bias, a.v_linear.bias],
                           [kv, kv[:, d:]], 2 * d)

    def _zattn_ok(self, lat, Le):
        """The cross-attention of a step runs over the latent rows themselves (gct_attn_decode_z)."""
        return zattn_latent_ok(self.model, lat) and Le <= 256

    def _fold_cross(self, cl):
        """Once per sequence (the n_c condition rows) on top of a weights-only part that is CACHED across start()
        calls while the weights stay the same (`model.weights_token()`): the cross-attention of layer l over the memory
        e = fc_z(z) is rewritten over z itself (gct_attn_decode_z).  With G = W_k W_z, Hm = W_v W_z (d x latent) and
        the block-diagonal BD[h*lat + c, h*dk + r] = G[h*dk + r, c]:
            folded query    q' = BD (W_q x + b_q)            -> zq_w = [W_q ; BD W_q], zq_b = [b_q ; BD b_q]
            folded output   y  = W_o (o_cond + BDH ctx) + b_o + W_o d   with d = W_v b_z + b_v
        (the key-side constant c = W_k b_z + b_k shifts every score of a row equally and drops out of the softmax; the
        condition rows keep explicit keys / values, shifted by -c / -d so that they share the softmax and the bias)."""
        dec, d = self.dec, self.d
        token = self.model.weights_token() if hasattr(self.model, "weights_token") else None
        key = (token, ops.gemm_get_mode(), self.nq, self.nz, self.zflat.data_ptr())
        if token is None or self._fold_key != key:
            self._fold_weights()
            self._fold_key = key
        off = self.nq - self.nz
        if off:                                                     # condition rows: k - c | v - d
            for li in range(len(dec.layers)):
                self._shifted_cond_kv(li, cl, self.ckv[li])

    def _shifted_cond_kv(self, li, cl, kv):
        """Layer li's keys | values of the condition rows cl [rows, d] into kv [rows, 2 d], shifted by -c | -d."""
        a, d = self.dec.layers[li].attn_2, self.d
        ops.linear_fwd(cl, [a.k_linear.weight, a.v_linear.weight], [a.k_linear.bias, a.v_linear.bias],
                       [kv, kv[:, d:]], 2 * d)
        kv.view(-1, 2, d).sub_(self.zcv[li].view(1, 2, d))

    def _fold_weights(self):
        """The weights-only part of _fold_cross (43 ms of small GEMMs and index fills for six layers: 15 % of a whole
        n = 4096 decode before it was cached)."""
        dec, d, H, dk, dev = self.dec, self.d, self.H, self.dk, self.zflat.device
        lat = self.nz // H
        Wz, bz = dec.fc_z.weight, dec.fc_z.bias
        WzT = Wz.t().contiguous()                                  # [lat, d]
        hh = torch.arange(H, device=dev)
        off = self.nq - self.nz                                    # d with condition rows, else 0

        def blockdiag(M):                                          # M [d, lat] -> [H*lat, d]
            bd = torch.zeros(H, lat, H, dk, device=dev)
            bd[hh, :, hh, :] = M.view(H, dk, lat).transpose(1, 2)
            return bd.view(H * lat, d)

        self.zcv = []
        for li, layer in enumerate(dec.layers):
            a = layer.attn_2
            G, Hm = torch.empty(d, lat, device=dev), torch.empty(d, lat, device=dev)
            ops.linear_fwd(a.k_linear.weight, [WzT], [None], [G], lat)             # W_k W_z
            ops.linear_fwd(a.v_linear.weight, [WzT], [None], [Hm], lat)            # W_v W_z
            cv = torch.empty(2, d, device=dev)                                      # c = W_k b_z + b_k ; d = W_v b_z + b_v
            ops.linear_fwd(bz.view(1, d), [a.k_linear.weight], [a.k_linear.bias], [cv[0:1]], d)
            ops.linear_fwd(bz.view(1, d), [a.v_linear.weight], [a.v_linear.bias], [cv[1:2]], d)
            self.zcv.append(cv)
            BD, BDH = blockdiag(G), blockdiag(Hm)
            qw, ow = self.zq_w[li], self.zo_w[li]
            ops.linear_fwd(BD, [a.q_linear.weight.t().contiguous()], [None], [qw[off:]], d)          # BD W_q
            ops.linear_fwd(BD, [a.q_linear.bias.view(1, d)], [None], [self.zq_b[li][off:].view(-1, 1)], 1)
            ops.linear_fwd(a.out.weight, [BDH], [None], [ow[:, off:]], self.nq)    # W_o BDH^T^T: rows of BDH are its N
            ops.linear_fwd(cv[1:2], [a.out.weight], [a.out.bias], [self.zo_b[li].view(1, d)], d)     # W_o d + b_o
            if off:
                qw[:off].copy_(a.q_linear.weight)
                self.zq_b[li][:off].copy_(a.q_linear.bias)
                ow[:, :off].copy_(a.out.weight)
        if ops.gemm_get_mode() != ops.GEMM_F32:          # bf16x6 / bf16x3
            self.zplanes = ops.split_planes(self.zflat, self.zplanes)
            ops.register_planes(self.zflat, self.zplanes)

    # -------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill(self, ys0, prefix_lens=None):
        """The prefix ys0 [n, t0] (and, with use_cond2dec, the condition tokens in front of it) through one decoder
        forward; fills the caches for positions < off + t0 and returns the logits of the last prefix position.
        prefix_lens (int64 [n], from check_prefix_lens; None = all t0): row r's prefix is ys0[r, :t0_r]; the columns
        behind it become pad (invalid cache slots until generation overwrites them), the returned logits are those of
        position t0_r - 1, and row_off holds the offsets t0 - t0_r a MIXED step unit runs with."""
        from .Model.modules import get_trg_mask
        dec, d, n = self.dec, self.d, self.n
        t0 = ys0.shape[1]
        ys0 = ys0.to(self.ys.device)
        if prefix_lens is not None:
            lens = prefix_lens.to(self.ys.device, torch.int64)
            ys0 = pad_behind_prefix(ys0, lens, self.pad_id)
            self.row_off.copy_(t0 - lens)
        self.ys.fill_(self.pad_id)
        self.ys[:, :t0] = ys0
        self.valid.zero_()
        self.valid[:, :self.off] = 1
        self.valid[:, self.off:self.off + t0] = (ys0 != self.pad_id).to(torch.uint8)
        self.done.zero_()
        trg_mask = get_trg_mask(ys0, self.pad_id, self.c2d, self.dconds if dec.nconds > 0 else None)
        run = engine.Run(0.0, False)
        sm, tm = ops.to_mask_u8(self.src_mask_in), ops.to_mask_u8(trg_mask)
        plan = engine.RowPlan.launch(engine.PREFILL, dec, sm, tm, None, *ys0.shape, self.z.shape[1]).finish()
        y, saved, _, _ = engine.decoder_trunk_fwd(dec, run, ys0.contiguous(), engine._f32c(self.z), sm, tm,
                                                  self.dconds, False, plan)
        Tp = self.off + t0
        for li, layer in enumerate(saved.layers):                   # the self-attention's q | k | v fills the caches
            qkv = layer.attn_1.qkv.view(n, Tp, 3 * d)
            self.kc[li][:, :Tp].copy_(qkv[:, :, d:2 * d])
            self.vc[li][:, :Tp].copy_(qkv[:, :, 2 * d:])
        out = self.model.out
        last = y[:, -1] if prefix_lens is None else y[torch.arange(n, device=y.device), self.off + lens - 1]
        ops.linear_fwd(last.contiguous(), [out.weight], [out.bias], [self.buf["logits"]], out.weight.shape[0])
        self.pos.fill_(t0 - 1)                                      # "token t0-1 has been consumed" (row r: t0_r - 1)
        return self.buf["logits"]

    # -------------------------------------------------------------------------------------
    def _rows(self, plan, mask=False):
        """The row view of a plan, as the keyword arguments the step's kernels take it in: row_off (MIXED and STREAM:
        row r is at *pos - row_off[r]), item and prefix_len (STREAM: the item a row works on and the items' prefix
        lengths), None each where the layout has none.  mask=True: what gct_grammar_mask reads besides -- gram, and
        the items' limit (STREAM)."""
        st = self.stream if plan.layout == STREAM else {}
        view = dict(row_off=None if plan.layout == UNIFORM else self.row_off, item=st.get("item"),
                    prefix_len=st.get("prefix_len"))
        return dict(view, gram=self.gram, limit=st.get("limit")) if mask else view

    @torch.no_grad()
    def step(self, plan=StepPlan()):
        """Consume token ys[:, p] with p = *pos + 1 ... see _chain: ONE generated token, position on the device.
        select BEAM / SBEAM / SMC: the self-attention reads the caches through the ancestry map kv_src
        (gct_attn_decode_beam)."""
        dec, d, n, T, B = self.dec, self.d, self.n, self.T, self.buf
        beam, row_off = plan.select in (BEAM, SBEAM, SMC), self._rows(plan)["row_off"]
        check(ops._L().gct_decode_advance(self.pos.data_ptr(), ops._st()), "gct_decode_advance")   # pos = the token consumed now
        ops.decode_embed(self.ys, self.pos, self.off, dec.embed.embed.weight, dec.pe.pe, B["x"], math.sqrt(d),
                         row_off=row_off)
        x = B["x"]
        for li, layer in enumerate(dec.layers):
            a1, a2, ff = layer.attn_1, layer.attn_2, layer.ff
            ops.norm_fwd(x, layer.norm_1.alpha, layer.norm_1.bias, layer.norm_1.eps, out=B["x2"])
            qkv = B["qkv"]
            ops.linear_fwd(B["x2"], [a1.q_linear.weight, a1.k_linear.weight, a1.v_linear.weight],
                           [a1.q_linear.bias, a1.k_linear.bias, a1.v_linear.bias],
                           [qkv, qkv[:, d:], qkv[:, 2 * d:]], 3 * d, **self.gemm_kw)
            if beam:
                ops.attn_decode_beam(qkv, 3 * d, self.kc[li], self.vc[li], d, T * d, self.valid, T, B["o"], n,
                                     self.H, T, self.dk, self.pos, self.off, qkv[:, d:], qkv[:, 2 * d:], 3 * d,
                                     self.kv_src)
            else:
                ops.attn_decode(qkv, 3 * d, self.kc[li], self.vc[li], d, T * d, self.valid, T, B["o"], n,
                                self.H, 0, self.dk, pos=self.pos, cache_off=self.off, knew=qkv[:, d:],
                                vnew=qkv[:, 2 * d:], ldn=3 * d, row_off=row_off)
            ops.linear_fwd(B["o"], [a1.out.weight], [a1.out.bias], [B["xa"]], d,
                           epi=ops.EPI_DROP_RESID, resid=x, **self.gemm_kw)
            ops.norm_fwd(B["xa"], layer.norm_2.alpha, layer.norm_2.bias, layer.norm_2.eps, out=B["x2"])
            if self.zattn:
                off = self.nq - self.nz
                ops.linear_fwd(B["x2"], [self.zq_w[li]], [self.zq_b[li]], [B["q2"]], self.nq, **self.gemm_kw)
                ops.attn_decode_z(B["q2"], off, self.z3, self.ckv[li], self.Lk - self.z3.shape[1], self.src_valid,
                                  B["o2"], off, n, self.H, self.dk, klen=self.src_klen)
                ops.linear_fwd(B["o2"], [self.zo_w[li]], [self.zo_b[li]], [B["xb"]], d,
                               epi=ops.EPI_DROP_RESID, resid=B["xa"], **self.gemm_kw)
            else:
                ops.linear_fwd(B["x2"], [a2.q_linear.weight], [a2.q_linear.bias], [B["q2"]], d, **self.gemm_kw)
                kv = self.cross_kv[li]
                ops.attn_decode(B["q2"], d, kv, kv[:, d:], 2 * d, self.Lk * 2 * d, self.src_valid, self.Lk,
                                B["o2"], n, self.H, self.Lk, self.dk, klen=self.src_klen)
                ops.linear_fwd(B["o2"], [a2.out.weight], [a2.out.bias], [B["xb"]], d,
                               epi=ops.EPI_DROP_RESID, resid=B["xa"], **self.gemm_kw)
            ops.norm_fwd(B["xb"], layer.norm_3.alpha, layer.norm_3.bias, layer.norm_3.eps, out=B["x2"])
            ops.linear_fwd(B["x2"], [ff.linear_1.weight], [ff.linear_1.bias], [B["hdn"]],
                           B["hdn"].shape[1], epi=ops.EPI_GELU_DROP, pre=B["pre"], **self.gemm_kw)
            xc = B["xc"][li & 1]
            ops.linear_fwd(B["hdn"], [ff.linear_2.weight], [ff.linear_2.bias], [xc], d,
                           epi=ops.EPI_DROP_RESID, resid=B["xb"], **self.gemm_kw)
            x = xc
        ops.norm_fwd(x, dec.norm.alpha, dec.norm.bias, dec.norm.eps, out=B["y"])
        out = self.model.out
        ops.linear_fwd(B["y"], [out.weight], [out.bias], [B["logits"]], out.weight.shape[0], ws=self.ws)
        return B["logits"]

    def _select(self, plan):
        """softmax + choice of the next token from buf['logits']; written at ys[:, *pos + 1] (device position).
        BEAM: gct_beam_select (beam state, the kv_src map and bdone in place); SBEAM: gct_beam_select_gumbel.  FILTERED: the multinomial draw through the
        top-k / nucleus / temperature settings in self.filt.  With a grammar the choice is made from a masked copy of
        the logits (gct_grammar_mask, one launch more); buf['logits'] stays raw for _chosen_logp and _step_stats.  A
        unit with stats has a multinomial draw through a filter or a grammar write the distribution it drew from to
        buf['probs'] (_behaviour_probs)."""
        if plan.select == BEAM:
            ops.beam_select(self.buf["logits"], self.beams, self.bscores, self.bfin, self.blen, self.ys, self.valid,
                            self.off, self.kv_src, self.bdone, self.pos, self.pad_id, self.eos_id,
                            parent_i32=self.bparent)
            return
        if plan.select == SBEAM:                         # the same state plus bgumbel; the draw's seed from self.seed
            ops.beam_select_gumbel(self.buf["logits"], self.beams, self.bscores, self.bgumbel, self.bfin, self.blen,
                                   self.ys, self.valid, self.off, self.kv_src, self.bdone, self.pos, self.pad_id,
                                   self.eos_id, seed_dev=self.seed, parent_i32=self.bparent)
            return
        logits = self.buf["logits"]
        if plan.select == SMC:                           # the mask through the ancestry, then weight / resample / draw:
            ops.grammar_mask(logits, self.buf["masked"], self.gtable, self.ys, self.pos, width=self.T - self.off,
                             gram=self.gram, kv_src=self.kv_src, valid_off=self.off)       # bscores holds the log-weights
            ops.smc_select(logits, self.buf["masked"], self.beams, self.bscores, self.blogp, self.bfin, self.blen, self.ys,
                           self.valid, self.off, self.kv_src, self.bdone, self.pos, self.pad_id, self.eos_id, self.blogz,
                           self.bres, self.btau, seed_dev=self.seed, parent_i32=self.bparent)
            return
        if plan.grammar:                                 # the selection sees -inf on what the grammar / the budget forbid
            ops.grammar_mask(logits, self.buf["masked"], self.gtable, self.ys, self.pos, width=self.T - self.off,
                             **self._rows(plan, mask=True))
            logits = self.buf["masked"]
        filtered = plan.select == FILTERED
        ops.select_token(logits, self.ys, 0, self.valid, self.done, 1 if filtered else plan.select,
                         self.pad_id, self.eos_id, pos_dev=self.pos, valid_off=self.off, seed_dev=self.seed,
                         filt_dev=self.filt if filtered else None, probs_out=self._behaviour_probs(plan),
                         item_base=self.stream["item_base"] if plan.layout == STREAM else 0, **self._rows(plan))

    def _advance(self, plan):
        """One step and its selection: the unit a graph captures.  Continuous batching: then the refill."""
        self.step(plan)
        self._select(plan)
        if plan.logp:
            self._chosen_logp(plan)                      # before the refill, which reassigns the rows' items
        if plan.stats:
            self._step_stats(plan)
        if plan.layout == STREAM:
            self.stream["state"].refill()

    def _chosen_logp(self, plan):
        """The model's log-probability of the token _select has just written (gct_chosen_logp): into tok_logp at the
        row's own column, or, streamed, into the pool's table at (item, column)."""
        out = self.stream["out_logp"] if plan.layout == STREAM else self.tok_logp
        ops.chosen_logp(self.buf["logits"], self.ys, self.pos, out, self.pad_id, **self._rows(plan))

    def _behaviour_probs(self, plan):
        """buf['probs'] [n, V] where a unit with stats draws from another distribution than the model's softmax -- a
        multinomial draw through a filter or a grammar -- and None otherwise (greedy: the one-hot at the token; the
        plain multinomial draw: the softmax itself).  A function of the plan alone, as a captured graph needs it;
        allocated with the rows' first such unit, like buf['masked']."""
        if not plan.stats or plan.select == 0 or not (plan.select == FILTERED or plan.grammar):
            return None
        if "probs" not in self.buf:
            self.buf["probs"] = torch.empty_like(self.buf["logits"])
        return self.buf["probs"]

    def _stats_tables(self, plan, zero=False):
        """The four tables gct_step_stats writes, [4, rows, T]: the decoder's own, laid out like ys, or, streamed, the
        pool's, per (item, column).  Allocated with the first call that asks for statistics."""
        st = self.stream if plan.layout == STREAM else None
        tab = self.stats_tab if st is None else st.get("out_stats")
        if tab is None:
            tab = torch.zeros(len(ops.STEP_STATS), self.n if st is None else st["items"], self.T, device=self.ys.device)
            if st is None:
                self.stats_tab = tab
            else:
                st["out_stats"] = tab
        elif zero:
            tab.zero_()
        return tab

    def _step_stats(self, plan):
        """The statistics of the draw _select has just made (gct_step_stats), at _chosen_logp's (row, column)."""
        ops.step_stats(self.buf["logits"], self._behaviour_probs(plan), self.ys, self.pos, self.pad_id,
                       greedy=plan.select == 0, **dict(zip(ops.STEP_STATS, self._stats_tables(plan))),
                       **self._rows(plan))

    def _span_stats(self, plan, ys, lens, n_gen):
        """StepStats of return_stats: the four tables through _span_logp, and behaviour_logp's row sum."""
        kept = [self._span_logp(t, ys, lens, n_gen) for t in self._stats_tables(plan)]
        return StepStats(*[t for t, _ in kept], kept[ops.STEP_STATS.index("behaviour_logp")][1])

    # ------------------------------------------------------------- what generate and generate_stream share
    def _check_sampling(self, algo, top_k, top_p, temperature):
        """The sampling settings of a generate call, the half that can raise: ValueError for bad values and for a
        filtered draw over too large a vocabulary.  Returns the GctSampleFilter record (CPU) when the draws go through
        the filter, None when they do not (neutral settings, or greedy: the filters always keep the top token)."""
        V = self.model.out.weight.shape[0]
        filtered = check_sample_filter(top_k, top_p, temperature, V) and algo == "multinomial"
        if filtered and V > ops.SAMPLE_FILTER_MAX_VOCAB:
            raise ValueError(f"top-k / nucleus / temperature sampling supports vocabularies up to "
                             f"{ops.SAMPLE_FILTER_MAX_VOCAB} tokens, not {V}")
        return ops.sample_filter_settings(top_k, top_p, temperature, V) if filtered else None

    def _set_sampling(self, algo, filt, seed, grammar, budget, t0):
        """The other half, after every check of the call has passed: seed, filter record and grammar go to the device
        buffers the captured graphs read -- the grammar as its class table and (budget G, prefix width), allocated with
        the masked copy of the logits when a decoder's rows first see a grammar.  Returns StepPlan.select."""
        select = {"greedy": 0, "multinomial": 1}[algo]
        self.seed.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        if filt is not None:
            select = FILTERED
            self.filt.copy_(filt)
        if grammar is not None:
            if self.gram is None:                        # first grammar on these rows (they live as long as the rows do,
                dev, (n, V) = self.ys.device, self.buf["logits"].shape     # like the graphs captured against them)
                self.gram = torch.zeros(2, dtype=torch.int32, device=dev)
                self.gtable = torch.zeros(V, dtype=torch.int32, device=dev)
                self.buf["masked"] = torch.empty(n, V, device=dev)
            self.gtable.copy_(grammar.device_table(self.gtable.device))
            self.gram.copy_(torch.tensor([int(budget), int(t0)], dtype=torch.int32))
        return select

    def _cut_at_eos(self, ys, lens, t0):
        """The reference's break point: when every row has produced <eos>, ys [n, t0 + G] (rows' tokens from column
        lens[r]) is cut after the longest row's first one.  Returns (ys, is_eos [n, G] of the uncut generated part)."""
        is_eos = generated_tokens(ys, lens) == self.eos_id
        if ys.size(0) and bool(is_eos.any(dim=1).all()):
            ys = ys[:, :t0 + int(is_eos.int().argmax(dim=1).max().item()) + 1]
        return ys, is_eos

    def _span_logp(self, table, ys, lens, n_gen):
        """(token_logp, logp) of return_logp: table [n, >= L] laid out like ys [n, L], kept on row r's generated span --
        its columns lens[r] .. lens[r] + n_gen[r] - 1 that are not pad -- and 0 elsewhere: a finished or held row decodes
        on, and the capture warm-up and the replay guard run real steps past the position they restore."""
        dev = ys.device
        start, cols = lens.to(dev).view(-1, 1), torch.arange(ys.size(1), device=dev).view(1, -1)
        span = (cols >= start) & (cols < start + n_gen.to(dev).view(-1, 1)) & (ys != self.pad_id)
        token_logp = torch.where(span, table[:, :ys.size(1)], torch.zeros((), device=dev))
        return token_logp, token_logp.sum(1)

    def _check_room(self, who, t0, steps):
        """A prefix of t0 tokens + `steps` steps (+ the `off` condition rows) fit the positional table, then the cache
        rows start() laid out; ValueError otherwise.  Before the first start() there are no cache rows to ask about:
        only the table is checked, and that the rows are missing is the caller's refusal (generate_stream: no pool)."""
        pe_rows = self.dec.pe.pe.shape[1]
        if self.off + t0 + steps > pe_rows:
            raise ValueError(f"{who}: prefix {t0} + {steps} steps + {self.off} condition rows exceed the {pe_rows}-row "
                             "positional table")
        if self._shape is not None and self.off + t0 + steps > self.T:
            raise ValueError(f"{who}: prefix {t0} + {steps} steps exceeds the cache length {self.T - self.off}")

    def _lockstep(self, plan, ys0, lens, steps, done, check_every, use_graphs):
        """THE driver of the decodes whose rows move in step (generate, generate_beam, generate_sbs): the prefill of
        the prefix rows ys0 [n, t0] (lens: prefill's prefix_lens), the first selection from the prefill's logits, then
        steps - 1 units of `plan`.  Every check_every steps (0: never) the host reads the device flags `done` and stops
        once all are set.  The caller has written the per-call device state the unit reads -- the prefill touches none
        of it.  Returns last: the decode wrote the token columns ys[:, :last]."""
        t0 = ys0.shape[1]
        self.prefill(ys0, lens)
        self._select(plan)                                         # token t0 from the prefill's last position
        if plan.logp:
            self._chosen_logp(plan)
        if plan.stats:
            self._step_stats(plan)
        for i in range(1, steps):
            self._run_step(plan, use_graphs)                       # consumes token t0+i-1, writes token t0+i
            if check_every and (i + 1) % check_every == 0 and bool(done.all()):
                return t0 + i + 1
        return t0 + steps

    def _beam_entry(self, who, ys0, k, max_strlen, prefix_lens, root=None):
        """What generate_beam and generate_sbs (`who`) do before the decode: the refusals (ValueError), then the beam
        state of start(..., beams=k)'s rows back to sbs_init's -- bscores [0, -inf, ...] per sample, bgumbel the same
        with the root's Gumbel value `root` [ns] (None: the unit has no bgumbel, it stays), no beam finished, no length,
        every row its own ancestor.  Returns (ns, k, t0, steps, the prefix rows [ns * k, t0] on the device)."""
        if prefix_lens is not None:
            raise ValueError(f"{who}: mixed prefix lengths are not supported; run one decode per length")
        k = int(k)
        if k != self.beams:
            raise ValueError(f"{who}: {k} beams, but start() prepared {self.beams} beam(s) per sample")
        ns, t0 = ys0.shape
        if ns * k != self.n:
            raise ValueError(f"{who}: {ns} prefixes x {k} beams != the {self.n} rows start() prepared")
        steps = max_strlen - 1
        if steps < 1:
            raise ValueError(f"{who}: max_strlen must be at least 2")
        self._check_room(who, t0, steps)
        dev = self.ys.device
        scores, gumbels, _, _ = sbs_init(ns, k, dev, root)
        self.bscores.copy_(scores.view(-1))
        if root is not None:
            self.bgumbel.copy_(gumbels.view(-1))
        self.bfin.zero_()
        self.blen.zero_()
        self.bdone.zero_()
        self.kv_src.copy_(torch.arange(self.n, dtype=torch.int32, device=dev).view(-1, 1).expand(-1, self.T))
        return ns, k, t0, steps, ys0.to(dev).repeat_interleave(k, 0)

    def _beam_tokens(self, ns, k, last):
        """The beams' token rows [ns, k, last]: token t of beam b lies in the row kv_src[b, off + t] that wrote it."""
        ys = torch.gather(self.ys[:, :last], 0, self.kv_src[:, self.off:self.off + last].long())
        return ys.view(ns, k, last)

    # -------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, ys0, max_strlen=80, algo="greedy", seed=0, check_every=8, use_graphs=False, prefix_lens=None,
                 top_k=None, top_p=None, temperature=1.0, return_logp=False, grammar=None, return_stats=False):
        """Mirror of Sampling.decode: appends max_strlen-1 tokens to the prefix ys0 [n, t0]
        (stops early once every sample has produced <eos>, like the reference's break).
        prefix_lens (ints [n], 1 <= t0_r <= t0, optional): row r's prefix is ys0[r, :t0_r] (right-padded); it decodes
        exactly what it would decode alone.  The output is then [n, t0 + G] with row r's G generated tokens at columns
        t0_r .. t0_r + G - 1 and pad behind them: generated_tokens(ys, prefix_lens) returns them as [n, G].  All lengths
        equal to t0 (or None): the uniform path.
        top_k / top_p / temperature (sample_filter_reference states the rules; validated before any device work, bad
        values raise ValueError): with algo="multinomial" and a non-neutral setting every draw goes through the filter
        (a selection mode and graph of its own; vocabularies up to ops.SAMPLE_FILTER_MAX_VOCAB).  Greedy ignores them:
        the filters always keep the top token.
        return_logp=True: returns (ys, token_logp, logp) -- token_logp [n, L] fp32 laid out like ys holds the MODEL's
        log-probability of every generated token up to the row's first <eos> (raw logits at temperature 1, whatever
        filter the draw went through; score_reference's rule), 0 on prefix, pad and later columns; logp [n] its row
        sum.  One small launch per step behind the selection (gct_chosen_logp), no second forward.
        grammar (a SmilesGrammar over the model's vocabulary, optional): constrained decoding -- every mode chooses among
        the tokens the grammar allows after the row's own generated tokens and that still let the row reach <eos> within
        its max_strlen - 1 tokens (gct_grammar_mask in front of the selection, one launch more per step; None: no launch).
        Every row then ends with <eos> and parses; the guarantee is syntactic, not chemical.  return_logp stays the
        model's own log-probability (raw logits).  ValueError for max_strlen < 3 or a grammar of another vocabulary.
        return_stats=True: a StepStats comes last in the result -- per generated token the model's entropy, the
        log-probability under the BEHAVIOUR distribution the token was really drawn from (through the filter, the
        temperature and the grammar; the one-hot under greedy), that distribution's entropy and its KL divergence from
        the model's (step_stats_reference states the rules; gct_step_stats, one small launch per step behind the
        selection).  Combines with everything above; False: nothing of it runs."""
        check_grammar(grammar, self.model.out.weight.shape[0], max_strlen - 1)
        filt = self._check_sampling(algo, top_k, top_p, temperature)
        n, t0 = ys0.shape
        steps = max_strlen - 1
        lens = check_prefix_lens(prefix_lens, n, t0)
        self._check_room("generate", t0, steps)
        plan = StepPlan(self._set_sampling(algo, filt, seed, grammar, steps, t0), UNIFORM if lens is None else MIXED,
                        grammar is not None, bool(return_logp), bool(return_stats))
        if plan.logp:
            self.tok_logp.zero_()
        if plan.stats:                                  # (both buffers exist before a step is run or captured)
            self._stats_tables(plan, zero=True)
            self._behaviour_probs(plan)
        last = self._lockstep(plan, ys0, lens, steps, self.done, check_every, use_graphs)
        lens = row_prefix_lens(lens, n, t0)
        ys, is_eos = self._cut_at_eos(self.ys[:, :last], lens, t0)
        if not (plan.logp or plan.stats):
            return ys.clone()
        # a row's generated span: from its own t0_r to its first <eos>, or all G columns without one
        n_gen = torch.where(is_eos.any(dim=1), is_eos.int().argmax(dim=1) + 1, is_eos.size(1))
        out = (ys.clone(),)
        if plan.logp:
            out += self._span_logp(self.tok_logp, ys, lens, n_gen)
        return out + (self._span_stats(plan, ys, lens, n_gen),) if plan.stats else out

    @torch.no_grad()
    def generate_beam(self, ys0, beam_size, max_strlen=80, alpha=BEAM_ALPHA, check_every=8, use_graphs=False,
                      prefix_lens=None):
        """Beam search from the prefix ys0 [n, t0] after start(..., beams=beam_size): up to max_strlen-1 tokens, stops
        early once every beam of every sample has produced <eos> (checked every `check_every` steps).
        Returns (ys [n, k, L] int64, scores [n, k] fp32 sums of log-probabilities, lengths [n, k] int64), beams sorted
        by score / length**alpha (beam_finalize); pad after each beam's end, L = t0 + the longest beam.
        Mixed prefix lengths are not supported (prefix_lens raises ValueError): decode each length group on its own."""
        ns, k, t0, steps, rows = self._beam_entry("generate_beam", ys0, beam_size, max_strlen, prefix_lens)
        last = self._lockstep(StepPlan(BEAM), rows, None, steps, self.bdone, check_every, use_graphs)
        return beam_finalize(self._beam_tokens(ns, k, last), self.bscores.view(ns, k).clone(),
                             self.blen.view(ns, k).to(torch.int64), t0, alpha)

    @torch.no_grad()
    def generate_sbs(self, ys0, k, max_strlen=80, seed=0, check_every=8, use_graphs=False, prefix_lens=None):
        """Stochastic beam search from the prefix ys0 [n, t0] after start(..., beams=k): k DISTINCT token rows per
        sample, an exact sample without replacement from the model's distribution over sequences of up to max_strlen-1
        tokens (sbs_step_reference states the step; gct_beam_select_gumbel runs it).  generate_beam's flow: prefill,
        sbs_init, the first selection from the prefill's logits, the steps with an early stop once every beam of every
        sample has produced <eos> (checked every `check_every` steps), the gather through kv_src.
        Returns SbsSamples(ys [n, k, L], logp [n, k], gumbel [n, k], lengths [n, k]), beams in drawing order (descending
        Gumbel value, the order the kernel leaves them in; no length normalisation), L = t0 + the longest beam.  The
        root's Gumbel value is drawn too (sbs_root_gumbels(n, seed): sbs_importance_weights needs it).  The same seed
        gives the same sample.  Mixed prefix lengths raise ValueError, as in generate_beam."""
        ns, k, t0, steps, rows = self._beam_entry("generate_sbs", ys0, k, max_strlen, prefix_lens,
                                                  root=sbs_root_gumbels(ys0.shape[0], seed))
        self.seed.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        last = self._lockstep(StepPlan(SBEAM), rows, None, steps, self.bdone, check_every, use_graphs)
        ys, lengths = self._beam_tokens(ns, k, last), self.blen.view(ns, k).to(torch.int64)
        return SbsSamples(ys[:, :, :t0 + int(lengths.max())].contiguous(), self.bscores.view(ns, k).clone(),
                          self.bgumbel.view(ns, k).clone(), lengths)

    @torch.no_grad()
    def generate_smc(self, ys0, k, grammar, max_strlen=80, seed=0, ess_threshold=0.5, check_every=8, use_graphs=False,
                     prefix_lens=None):
        """Sequential Monte Carlo decoding under `grammar` (a SmilesGrammar over the model's vocabulary) from the prefix
        ys0 [n, t0] after start(..., beams=k): k weighted particles per sample whose weighted empirical distribution
        converges to the MODEL's distribution restricted to well-formed strings of up to max_strlen-1 tokens -- not to
        the locally renormalised one generate(grammar=) draws from -- and an unbiased estimate of that event's
        probability (smc_step_reference states the step; gct_grammar_mask_anc and gct_smc_select run it).
        generate_sbs's flow: the prefill, smc_init (every particle live, logw = logp = 0), the first selection from the
        prefill's logits, the steps with an early stop once every particle of every sample has finished.
        ess_threshold in [0, 1]: a sample resamples when its effective sample size falls below ess_threshold * k (0:
        never -- the particles are then the rows generate(algo="multinomial", grammar=) decodes for the latents repeated
        k times under the same seed, weighted per molecule; 1: at every step).  It lives in device memory: one captured
        graph serves every threshold and seed.  Returns SmcSamples.  The same seed gives the same result.
        ValueError, before any device work: a bad ess_threshold, k outside [1, ops.BEAM_MAX_K], no grammar or one of
        another vocabulary, max_strlen < 3, prefix_lens (mixed prefixes are not supported), then _beam_entry's."""
        tau = check_ess_threshold(ess_threshold)
        k = check_particles(k)
        if grammar is None:
            raise ValueError("generate_smc: the grammar is the potential the particles are weighted by; it is required")
        check_grammar(grammar, self.model.out.weight.shape[0], max_strlen - 1)
        if prefix_lens is not None:
            raise ValueError("generate_smc: mixed prefix lengths are not supported; run one decode per length")
        ns, k, t0, steps, rows = self._beam_entry("generate_smc", ys0, k, max_strlen, None)
        self._set_sampling("multinomial", None, seed, grammar, steps, t0)
        self.bscores.zero_()                                # log-weights: every particle live from the start
        self.blogp.zero_()
        self.blogz.zero_()
        self.bres.zero_()
        self.btau.fill_(tau)
        last = self._lockstep(StepPlan(SMC, UNIFORM, True), rows, None, steps, self.bdone, check_every, use_graphs)
        ys, lengths = self._beam_tokens(ns, k, last), self.blen.view(ns, k).to(torch.int64)
        logw, log_z, ess = smc_finalize(self.bscores.view(ns, k), self.blogz)
        return SmcSamples(ys[:, :, :t0 + int(lengths.max())].contiguous(), logw, self.blogp.view(ns, k).clone(), log_z,
                          lengths, ess, self.bres.to(torch.int64))

    # ------------------------------------------------------------------------------------- continuous batching
    @torch.no_grad()
    def start_stream(self, z, src_mask, dconds=None, rows=512, max_total_len=208, refold=False, item_base=0):
        """Prepare `rows` decode rows and a pool of N items for generate_stream: z [N, L_e, latent], src_mask bool
        [N, 1, L_e], dconds [N, n_c] as start() takes them, N smaller or larger than `rows`.  max_total_len and refold
        as in start().  item_base: the pool is items item_base .. item_base + N - 1 of a larger one (their multinomial
        keys; a pool taken in slices decodes exactly what it decodes whole).
        ValueError before any device work for use_cond2dec models, for a latent geometry whose cross-attention keeps
        per-sequence K / V projections (gct_attn_decode_z not taken: latent wider than 128 or
        than 2 d_model / H) and for rows outside [1, ops.STREAM_MAX_ROWS].
        HBM: the pool stays on the device until the next start_stream -- N * L_e * latent * 4 B of latent rows,
        N * (L_e + n_c) B of masks, and with cond2lat the projected condition rows, N * n_c * 2 d_model * 4 B PER
        LAYER (full-size model, n_c = 3, d_model = 512, 6 layers: 2.4 GB at N = 32 768), plus the prefix and result
        tables, 2 * N * T * 8 B.  The pool is not sliced internally; a caller short of memory passes slices with
        item_base.  A pool of the same geometry as the last one (N, rows, latent shape, max_total_len) is copied into
        the same buffers, so the captured stream graphs live on across start_stream / generate_stream calls, as the
        plain path's do; a new geometry drops them."""
        check_stream_model(self.model)
        R = check_stream_rows(rows)
        if z.dim() != 3:
            raise ValueError(f"z must be [N, L_e, latent], got {list(z.shape)}")
        N, Le, lat = z.shape
        if not self._zattn_ok(lat, Le):
            raise ValueError("continuous batching needs the cross-attention over the latent rows (gct_attn_decode_z): "
                             f"latent {lat} / {Le} rows keep per-sequence K / V projections")
        dec, d, dev = self.dec, self.d, z.device
        nc = dec.nconds
        c2l = bool(dec.use_cond2lat and nc > 0)
        if c2l and (dconds is None or tuple(dconds.shape) != (N, nc)):
            raise ValueError(f"a cond2lat model needs dconds [{N}, {nc}]")
        if tuple(src_mask.shape) != (N, 1, Le):                    # the refill copies L_e flags per item from the pool
            raise ValueError(f"src_mask must be [{N}, 1, {Le}] (one flag per latent row), got {list(src_mask.shape)}")
        if N < 1 or int(item_base) < 0 or int(item_base) + N >= 2 ** 31 - 256:
            raise ValueError(f"a pool of {N} items at item_base {item_base} does not fit")
        # the rows' buffers, geometry and folded projections: start() on placeholder rows (every row's latent rows, masks
        # and condition rows are laid out by the refill before the row's first step)
        self.start(torch.zeros(R, Le, lat, device=dev), torch.ones(R, 1, Le, dtype=torch.bool, device=dev),
                   torch.zeros(R, nc, device=dev) if c2l else None, max_total_len, refold)
        sv, klen = memory_masks(src_mask.to(dev), nc if c2l else 0, Le)
        key = (N, R, self._shape, c2l, self.ys.data_ptr())         # (start() reallocates the rows with a new geometry)
        st = self.stream
        if st is None or st["key"] != key:
            # a new pool geometry: new buffers, a new GctStreamState, and the stream graphs that held the old addresses
            # go.  The same geometry again (the sampler's next call) is copied into the buffers: its graphs stay
            T = self.T
            i32 = lambda *a: torch.zeros(*a, dtype=torch.int32, device=dev)               # noqa: E731
            st = self.stream = dict(
                key=key, rows=R, items=N, ckv_row=nc * 2 * d if c2l else 0,
                z_pool=torch.empty(N, Le * lat, device=dev), valid_pool=torch.empty_like(sv),
                klen_pool=torch.empty_like(klen),
                ckv_pool=[torch.empty(N * nc, 2 * d, device=dev) for _ in dec.layers] if c2l else [],
                prefix_pool=torch.full((N, T), self.pad_id, dtype=torch.int64, device=dev), prefix_len=i32(N),
                limit=i32(N), out_ys=torch.full((N, T), self.pad_id, dtype=torch.int64, device=dev), out_len=i32(N),
                out_logp=torch.zeros(N, T, device=dev),           # return_logp: written per (item, column) by the rows
                row_of=i32(N), start_step=i32(N), item=i32(R), harvest=i32(R),
                fresh=torch.zeros(R, dtype=torch.uint8, device=dev), next_item=i32(1), n_harvested=i32(1),
                enable=i32(1))
            state = ops.StreamState()                             # the pool's entries under GctStreamState's own names,
            st["state"] = state.set(                              # then the decoder's rows and the geometry
                **{name: v for name, v in st.items() if name in state.slot},
                ys=self.ys, valid=self.valid, done=self.done, row_off=self.row_off, pos=self.pos, z3=self.z3,
                src_valid=self.src_valid, src_klen=self.src_klen, ckv=[c for c in self.ckv if c is not None],
                ld_ys=self.ys.stride(0), valid_sb=self.valid.stride(0), valid_off=0, T=T, width=T, t0_max=T,
                z_row=self.z3.stride(0), Lk=self.Lk, layers=len(dec.layers) if c2l else 0, pad_id=self.pad_id)
            self._drop_stream_graphs()
        st["item_base"] = int(item_base)
        st["z_pool"].copy_(z.reshape(N, Le * lat))
        st["valid_pool"].copy_(sv)
        st["klen_pool"].copy_(klen)
        if c2l:
            self._cond_rows_pool(dconds.to(dev), st["ckv_pool"])

    def _cond_rows_pool(self, dconds, pool):
        """The shifted keys | values of every item's condition rows (what _fold_cross computes per row) into pool, per
        layer [N * n_c, 2 d].  Projected STREAM_COND_CHUNK items per GEMM, the last chunk padded, so that the GEMM shape --
        and with it an item's rounding -- does not depend on the size of the pool."""
        dec, d, nc, dev = self.dec, self.d, self.dec.nconds, dconds.device
        N, CH = dconds.shape[0], STREAM_COND_CHUNK
        chunk, kv = torch.zeros(CH, nc, device=dev), torch.empty(CH * nc, 2 * d, device=dev)
        for lo in range(0, N, CH):
            m = min(CH, N - lo)
            chunk.zero_()
            chunk[:m] = dconds[lo:lo + m].float()
            cl = ops.small_linear_fwd(chunk, dec.embed_cond2lat.weight, dec.embed_cond2lat.bias).view(CH * nc, d)
            for li in range(len(dec.layers)):
                self._shifted_cond_kv(li, cl, kv)
                pool[li][lo * nc:(lo + m) * nc].copy_(kv[:m * nc])

    def _drop_stream_graphs(self):
        """A captured stream step holds the addresses of the pool's buffers: new buffers, new graphs."""
        for key in [k for k in self.graphs if isinstance(k, tuple) and k[1] == STREAM]:
            del self.graphs[key]

    @torch.no_grad()
    def generate_stream(self, ys0, max_strlen=80, algo="greedy", seed=0, prefix_lens=None, max_new_tokens=None,
                        top_k=None, top_p=None, temperature=1.0, use_graphs=False, check_every=8, return_logp=False,
                        grammar=None, return_stats=False):
        """Decode the pool of start_stream with continuous batching: item i starts from the prefix ys0[i, :t0_i]
        (ys0 [N, t0_max], prefix_lens ints [N] or None = all t0_max) and generates until <eos> or max_new_tokens[i]
        tokens (ints [N] in [1, max_strlen - 1]; None: max_strlen - 1); a row that finishes takes the next item
        (stream_schedule_reference).  algo / seed / top_k / top_p / temperature / use_graphs as in generate(); the
        multinomial key of a draw is (item_base + i, token position).
        Returns (ys, record): ys [N, t0_max + G] int64 in ITEM order with generate(prefix_lens=)'s layout -- item i's
        tokens from column t0_i, pad behind its last one (generated_tokens works on it), cut after the longest item's
        <eos> when every item produced one -- and record = dict(steps: shared steps until the last item was done,
        launched: step units issued (the host looks at ONE device word, n_harvested, every check_every steps and
        nothing else), row_of [N], start_step [N], out_len [N] generated tokens with the <eos>, harvested).
        return_logp=True: returns (ys, record, token_logp, logp) in item order -- token_logp [N, L] fp32 laid out like
        ys, the model's log-probability of item i's generated tokens at columns t0_i .. t0_i + out_len_i - 1 and 0
        elsewhere, logp [N] its row sum (generate()'s return_logp).
        grammar (a SmilesGrammar, optional): as in generate(), with item i's budget max_new_tokens[i] read from the
        device: every item ends with <eos> inside its own limit.  ValueError for a limit below 2.
        return_stats=True: a StepStats in item order comes last in the result (generate()'s return_stats).
        ValueError before any device work for beam search, bad prefix_lens / max_new_tokens / sampling settings and
        lengths beyond the positional table or the cache rows of start_stream."""
        if algo not in ("greedy", "multinomial"):
            raise ValueError(f"generate_stream decodes greedy or multinomial, not {algo!r} (beam search keeps its rows "
                             "in step: generate_beam)")
        check_stream_model(self.model)
        filt = self._check_sampling(algo, top_k, top_p, temperature)
        if ys0.dim() != 2 or ys0.shape[1] < 1:
            raise ValueError(f"ys0 must be [N, t0_max >= 1], got {list(ys0.shape)}")
        N, t0 = ys0.shape
        steps = int(max_strlen) - 1
        if N < 1 or steps < 1:
            raise ValueError("generate_stream: needs at least one item and max_strlen >= 2")
        if isinstance(check_every, bool) or not isinstance(check_every, numbers.Integral) or check_every < 1:
            raise ValueError(f"check_every must be an int >= 1, got {check_every!r}")
        lens = row_prefix_lens(check_prefix_lens(prefix_lens, N, t0), N, t0)
        cap = check_max_new_tokens(max_new_tokens, N, steps)
        check_grammar(grammar, self.model.out.weight.shape[0], cap)
        W = t0 + steps
        self._check_room("generate_stream", t0, steps)
        st = self.stream
        if st is None:
            raise ValueError("generate_stream: no pool (call start_stream first)")
        if N != st["items"]:
            raise ValueError(f"generate_stream: {N} prefixes for the {st['items']} items start_stream prepared")
        if st["key"][2] != self._shape or st["key"][4] != self.ys.data_ptr():      # start() laid the rows out anew since
            raise ValueError("generate_stream: the decoder's rows are not the ones start_stream prepared (start() was "
                             "called with another geometry since); call start_stream again")
        R = st["rows"]
        # (columns behind t0 are never read: prefix_len <= t0)
        st["prefix_pool"][:, :t0].copy_(pad_behind_prefix(ys0.cpu(), lens, self.pad_id))
        st["prefix_len"].copy_(lens)
        st["limit"].copy_(cap)
        st["out_ys"].fill_(self.pad_id)
        for name, v in (("out_len", 0), ("row_of", -1), ("start_step", -1), ("item", -1), ("harvest", -1), ("fresh", 0),
                        ("next_item", 0), ("n_harvested", 0), ("enable", 1)):
            st[name].fill_(v)
        # (a streamed row reads its budget and prefix length per item: limit[item] / prefix_len[item])
        plan = StepPlan(self._set_sampling(algo, filt, seed, grammar, steps, t0), STREAM, grammar is not None,
                        bool(return_logp), bool(return_stats))
        if plan.logp:
            st["out_logp"].zero_()
        if plan.stats:                                  # (both buffers exist before a step is run or captured)
            self._stats_tables(plan, zero=True)
            self._behaviour_probs(plan)
        self.pos.fill_(-1)                                         # the first step consumes every row's token 0
        self.row_off.zero_()
        self.ys.fill_(self.pad_id)
        self.valid.zero_()
        self.done.zero_()
        # list scheduling ends within sum / R + max steps (Graham): a loop that runs past it has lost an item
        most = (N // R + 2) * W + check_every
        launched = 0
        st["state"].refill()                                       # the first wave enters like every later item
        while True:
            self._run_step(plan, use_graphs)
            launched += 1
            if launched % check_every == 0:
                if int(st["n_harvested"].item()) >= N:
                    break
                if launched > most:
                    raise RuntimeError(f"generate_stream: {int(st['n_harvested'].item())} of {N} items after "
                                       f"{launched} steps")
        out_len, start = st["out_len"].cpu().long(), st["start_step"].cpu().long()
        record = dict(steps=int((start + lens + out_len - 1).max()) if N else 0, launched=launched,
                      row_of=st["row_of"].cpu().long(), start_step=start, out_len=out_len,
                      harvested=int(st["n_harvested"].item()))
        ys, _ = self._cut_at_eos(st["out_ys"][:, :W], lens, t0)    # generate()'s cut: the longest item's <eos>
        out = (ys.clone(), record)
        if plan.logp:                                   # an item's generated span: the out_len tokens the refill handed out
            out += self._span_logp(st["out_logp"], ys, lens, out_len)
        return out + (self._span_stats(plan, ys, lens, out_len),) if plan.stats else out

    def _run_step(self, plan, use_graphs):
        g = self.graphs.get(plan.key) if use_graphs else False
        if g is None:
            self._capture(plan)                         # leaves the graph (or False) in self.graphs and runs this step
        elif g is False:                                # no usable graph for these buffers (capture failed, or replay is
            self._advance(plan)                         # the slower launch mode on this box): same kernels, eagerly
        else:
            g.replay()

    @staticmethod
    def _restore(keep):
        for t, k in keep:
            t.copy_(k)

    def _state_tensors(self, plan):
        """Everything a step + selection writes besides the caches' next row (the beam state included)."""
        base = (self.pos, self.ys, self.valid, self.done, self.bscores, self.bgumbel, self.bfin, self.blen,
                self.bparent, self.kv_src, self.bdone)
        if plan.select == SMC:
            base += (self.blogp, self.blogz, self.bres)
        if plan.layout != STREAM:
            return base
        st = self.stream                                  # (the refill is held while a state is kept: _hold_refill)
        return base + (self.row_off, st["item"], st["next_item"], st["n_harvested"])

    def _hold_refill(self, plan, hold):
        """Continuous batching: the capture warm-up and the replay guard execute real steps and then restore
        _state_tensors().  A refill in one of those steps would overwrite a row's latent rows, condition rows and cache
        slots, which no restore covers -- so they run with the device `enable` word at 0: a row that finishes is held
        (it decodes on, as a finished row of the plain path does) and the restore puts it back."""
        if plan.layout == STREAM:
            self.stream["enable"].fill_(0 if hold else 1)

    def _capture(self, plan):
        """Capture step + select into one graph, keep it under plan.key and replay it -- or keep False and run the step
        eagerly (capture failed, or the replay guard found replay slower than eager launches on this box)."""
        # Warm-up run on a side stream (lazy LDS opt-ins, allocator), then capture.  The warm-up really executes a
        # step (it advances the device position and writes a token), so the state it touches is restored before
        # the capture; a capture itself executes nothing.
        self._hold_refill(plan, True)
        keep = [(t, t.clone()) for t in self._state_tensors(plan)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._advance(plan)
        torch.cuda.current_stream().wait_stream(s)
        # (the key / value row the warm-up appended is rewritten with the same values by the replay below)
        self._restore(keep)
        try:
            g = torch.cuda.CUDAGraph(keep_graph=True)   # the hipGraph_t stays readable (graphdiag.census)
        except TypeError:
            g = torch.cuda.CUDAGraph()
        try:
            # thread_local: another thread's runtime calls (the RCCL watchdog of a data-parallel job queries
            # events) must not invalidate this thread's capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._advance(plan)
        except RuntimeError as exc:
            import warnings
            warnings.warn(f"KVDecoder: graph capture failed ({exc}); decoding without graph replay")
            torch.cuda.synchronize()
            self._restore(keep)
            g = None
        fast = g is not None and (not REPLAY_GUARD or self._replay_is_fast(plan, g, keep))
        self._hold_refill(plan, False)
        self.graphs[plan.key] = g if fast else False
        if fast:
            g.replay()
        else:                                           # no graph for these buffers: same kernels, launched eagerly
            self.graph_replay = False
            self._advance(plan)

    def _replay_is_fast(self, plan, g, keep):
        """Replay guard: a few steps launched eagerly and a few replayed, timed on the device, state restored after
        each.  Replay is the faster way to issue the ~70 launches of a step everywhere it behaves; on boxes where it is
        clearly the slower one (round 2: 3-13x) the decoder keeps launching eagerly, says so once, and leaves the
        numbers and the graph's census in `self.replay_probe` for the caller (bench.py prints them)."""
        ahead = int(keep[0][1].item())                                     # position of the row that is furthest along
        if plan.layout == STREAM:
            ahead -= int(self.row_off.min().item())
        room = self.T - self.off - (ahead + 1) - 1                       # steps the caches still have room for
        k = min(4, room)
        if k < 1:
            return True

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(k):
                fn()
            e1.record()
            e1.synchronize()
            self._restore(keep)
            return e0.elapsed_time(e1) / k

        eager = functools.partial(self._advance, plan)
        g.replay()                                                       # first replay (instantiation, upload): untimed
        self._restore(keep)
        t_graph = min(timed(g.replay), timed(g.replay))
        t_eager = min(timed(eager), timed(eager))
        torch.cuda.synchronize()
        try:                                   # the census is evidence for a report, never a reason to fail a decode
            from . import graphdiag
            cen = graphdiag.census(g)
        except Exception as exc:               # noqa: BLE001 -- diagnostics library missing / hipGraphGetNodes refused
            cen = {"error": repr(exc)}
        self.replay_probe = {"ms_per_step_graph": round(t_graph, 4), "ms_per_step_eager": round(t_eager, 4),
                             "steps_timed": k, "rows": self.n, "census": cen}
        if t_graph <= REPLAY_SLOW_FACTOR * t_eager:
            return True
        import warnings
        warnings.warn(f"KVDecoder: replaying the captured step takes {t_graph:.3f} ms against {t_eager:.3f} ms for the "
                      f"same kernels launched eagerly on this box; decoding with eager launches "
                      f"(GCT_DECODE_GRAPH_GUARD=0 forces replay; python tools/graph_probe.py prints the diagnosis)")
        return False


@torch.no_grad()
def reference_style_decode(model, z, src_mask, dconds, ys0, pad_id, eos_id, max_strlen=80, grammar=None):
    """The reference's loop (sampling_tool.py:140-184, greedy) on the un-cached model.decode --
    used by tests/benchmarks as the baseline the KV-cached path must match token for token.
    grammar (a SmilesGrammar, optional): the argmax is taken over grammar.mask_reference of the logits."""
    from .Model.modules import get_trg_mask
    check_grammar(grammar, model.out.weight.shape[0], max_strlen - 1)
    ys = ys0.clone()
    t0 = ys0.size(1)
    done = torch.zeros(ys.size(0), dtype=torch.bool, device=ys.device)
    for _ in range(max_strlen - 1):
        trg_mask = get_trg_mask(ys, pad_id, False, dconds)
        logits = model.decode(ys, z, src_mask, trg_mask, dconds)
        last = logits[:, -1]
        if grammar is not None:
            last = grammar.mask_reference(last.float(), ys, t0, ys.size(1), max_strlen - 1)
        nxt = last.argmax(-1)
        ys = torch.cat([ys, nxt[:, None]], dim=1)
        done |= nxt == eos_id
        if bool(done.all()):
            break
    return ys


@torch.no_grad()
def reference_style_beam_decode(model, z, src_mask, dconds, ys0, pad_id, eos_id, beam_size, max_strlen=80,
                                alpha=BEAM_ALPHA, trace=None):
    """Beam search on the un-cached model.decode over [n*k, t] every step (the reference's loop shape,
    sampling_tool.py:140-184, with beam_step_reference as the selection): the baseline generate_beam must match.
    use_cond2dec: the block mask and the logits of the token rows only, as the cached decoder sees them.
    trace (a list): receives the k+1 best candidate scores [n, k+1] of every step (near-tie diagnostics)."""
    from .Model.modules import get_trg_mask
    dec = model.decoder
    c2d = bool(dec.use_cond2dec and dec.nconds > 0)
    nc = dec.nconds if c2d else 0
    n, t0 = ys0.shape
    k = int(beam_size)
    rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
    z, src_mask, dconds, ys = rep(z), rep(src_mask), rep(dconds), rep(ys0)
    scores, finished, lengths = beam_init(n, k, ys.device)
    base = torch.arange(n, device=ys.device).view(n, 1) * k
    for _ in range(max_strlen - 1):
        logits = model.decode(ys, z, src_mask, get_trg_mask(ys, pad_id, c2d, dconds), dconds)[:, nc:]
        logp = beam_log_softmax(logits[:, -1])
        if trace is not None:
            cand = beam_candidates(scores, finished, logp, k, pad_id)
            trace.append(cand.topk(min(k + 1, cand.shape[1]), dim=1).values.cpu())
        parent, tok, scores, finished, lengths = beam_step_reference(scores, finished, lengths, logp, k, pad_id, eos_id)
        ys = torch.cat([ys[(base + parent).view(-1)], tok.view(-1, 1)], dim=1)
        if bool(finished.all()):
            break
    return beam_finalize(ys.view(n, k, -1), scores, lengths, t0, alpha)


@torch.no_grad()
def reference_style_sbs_decode(model, z, src_mask, dconds, ys0, pad_id, eos_id, k, noise_fn, max_strlen=80, trace=None,
                               root=None):
    """Stochastic beam search on the un-cached model.decode over [n*k, t] every step: reference_style_beam_decode's loop
    with sbs_step_reference as the selection -- the baseline generate_sbs must match.  noise_fn(step) -> [n*k, V] are the
    standard Gumbel variates of step 0, 1, ... (row s*k + b: beam b of sample s); root [n] the roots' Gumbel values
    (sbs_init; None: 0).  Returns SbsSamples.
    trace (a list): receives the k+1 largest candidate values [n, k+1] of every step (near-tie diagnostics)."""
    from .Model.modules import get_trg_mask
    dec = model.decoder
    c2d = bool(dec.use_cond2dec and dec.nconds > 0)
    nc = dec.nconds if c2d else 0
    n, t0 = ys0.shape
    k = int(k)
    rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
    z, src_mask, dconds, ys = rep(z), rep(src_mask), rep(dconds), rep(ys0)
    scores, gumbels, finished, lengths = sbs_init(n, k, ys.device, root=root)
    base = torch.arange(n, device=ys.device).view(n, 1) * k
    for step in range(max_strlen - 1):
        logits = model.decode(ys, z, src_mask, get_trg_mask(ys, pad_id, c2d, dconds), dconds)[:, nc:]
        logp, noise = beam_log_softmax(logits[:, -1]), noise_fn(step).to(ys.device)
        if trace is not None:
            val = sbs_candidates(scores, gumbels, finished, logp, noise, k, pad_id)[0]
            trace.append(val.topk(min(k + 1, val.shape[1]), dim=1).values.cpu())
        parent, tok, scores, gumbels, finished, lengths = sbs_step_reference(scores, gumbels, finished, lengths, logp,
                                                                             noise, k, pad_id, eos_id)
        ys = torch.cat([ys[(base + parent).view(-1)], tok.view(-1, 1)], dim=1)
        if bool(finished.all()):
            break
    ys = ys.view(n, k, -1)
    return SbsSamples(ys[:, :, :t0 + int(lengths.max())].contiguous(), scores, gumbels, lengths)


@torch.no_grad()
def reference_style_smc_decode(model, z, src_mask, dconds, ys0, pad_id, eos_id, k, grammar, u_fn, max_strlen=80,
                               ess_threshold=0.5, trace=None):
    """Sequential Monte Carlo on the un-cached model.decode over [n*k, t] every step: reference_style_sbs_decode's loop
    with grammar.mask_reference and smc_step_reference as the selection -- the baseline generate_smc must match.
    u_fn(step) -> [n, k + 1] are the uniforms of step 0, 1, ... (smc_step_reference's layout).  Returns SmcSamples.
    trace (a list): receives every step's `info` of smc_step_reference plus its uniforms (near-tie diagnostics)."""
    from .Model.modules import get_trg_mask
    dec = model.decoder
    c2d = bool(dec.use_cond2dec and dec.nconds > 0)
    nc = dec.nconds if c2d else 0
    n, t0 = ys0.shape
    k, tau = check_particles(k, "reference_style_smc_decode"), check_ess_threshold(ess_threshold)
    check_grammar(grammar, model.out.weight.shape[0], max_strlen - 1)
    rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
    z, src_mask, dconds, ys = rep(z), rep(src_mask), rep(dconds), rep(ys0)
    logw, logp, finished, lengths, log_z, resamples = smc_init(n, k, ys.device)
    logw, logp = logw.double(), logp.double()
    base = torch.arange(n, device=ys.device).view(n, 1) * k
    for step in range(max_strlen - 1):
        logits = model.decode(ys, z, src_mask, get_trg_mask(ys, pad_id, c2d, dconds), dconds)[:, nc:][:, -1].double()
        masked = grammar.mask_reference(logits, ys, t0, ys.size(1), max_strlen - 1)
        u, info = u_fn(step).to(ys.device), {}
        parent, tok, logw, logp, finished, lengths, log_z, resamples = smc_step_reference(
            logw, logp, finished, lengths, logits, masked, u, k, pad_id, eos_id, tau, log_z, resamples, info=info)
        if trace is not None:
            trace.append(dict(info, u=u, token=tok))
        ys = torch.cat([ys[(base + parent).view(-1)], tok.view(-1, 1)], dim=1)
        if bool(finished.all()):
            break
    ys = ys.view(n, k, -1)
    norm, log_z, ess = smc_finalize(logw, log_z)
    return SmcSamples(ys[:, :, :t0 + int(lengths.max())].contiguous(), norm, logp, log_z, lengths, ess, resamples)
