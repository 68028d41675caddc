"""Sampling front end with the reference's call surface (Inference/sampling_tool.py:19-647,
Model/build_model.py:90-116 `get_sampler`): per-model-type classes exposing
`sample_smiles(...) -> (smiles, toklen, toklen_gen)`, `encode_smiles(...)`, `id_to_smi`,
`sample_toklen`, `sample_z` -- running on the KV-cached decoder (gct_plus_amd.decode) instead
of re-running the decoder per generated token.

Deliberate deviations, none in the arithmetic:
  * vocabularies are gct_plus_amd.data.Vocab objects (no torchtext Field);
  * `id_to_smi` appends each token once (the reference appends it twice, sampling_tool.py:55-63);
  * token lengths are drawn from the same histogram-with-jitter distribution as
    Inference/toklen_sampling.py:19-36, with numpy's Generator instead of the global RNG;
  * decode_algo="beam" (the reference's -decode_algo choice, whose Inference/generate_mols.py code does not run) is
    beam search with frozen finished beams and a length-normalised final ranking (gct_plus_amd.decode): `decode`
    returns the best beam, `decode_beams` all of them;
  * `top_k` (the reference's -top_k) takes effect: the reference's per-model-type constructors never forward it, so there
    the flag is ignored.  Next to it, `top_p` (nucleus) and `temperature`; the rules are decode.sample_filter_reference,
    applied on the device between the softmax and the draw.  Greedy ignores all three (the top token is always kept);
    beam search does not take them;
  * decode_algo="stochastic_beam" with beam_size=k (no counterpart in the reference) is stochastic beam search (Kool, van
    Hoof and Welling 2019; decode.sbs_step_reference): `decode_unique` returns k DISTINCT molecules per latent, an exact
    sample without replacement, with their log-probabilities; `decode` returns the first draw of each, which is
    distributed exactly as a multinomial sample.  "beam"'s refusals apply; `decode_unique` itself works on any sampler.

`sample_multiple_smiles` (scaffold models) is the reference's commented-out PscavaetfSampling.sample_multiple_smiles,
one scaffold per row: the prefixes <sos> scaffold <sep> of different lengths are right-padded into ONE batch and decoded
with per-row positions (KVDecoder.generate(prefix_lens=)), so each row gives exactly what `sample_smiles` gives for its
scaffold alone (no left-padding, which would shift the positional encodings).  Beam search has no mixed-length kernels:
it runs one decode per prefix length and restores the input order.

Log-likelihoods: `score` / `score_smiles` give log p(x | z, conditions, scaffold) of molecules the caller holds
(decode.score_tokens: teacher-forced, one decoder forward), with the token accuracy next to it; `with_logp=True` makes
`decode`, `sample_smiles` and `sample_multiple_smiles` return the model's log-probability of what they drew as one more
element (KVDecoder.generate(return_logp=True): no second forward).  `with_stats=True` adds a decode.StepStats behind it:
per generated token the model's entropy and, for the BEHAVIOUR distribution the token was really drawn from (top-k /
nucleus / temperature and the grammar included), its log-probability, entropy and KL divergence from the model's
(KVDecoder.generate(return_stats=True)) -- Train/finetune.behaviour_weights turns the two log-probabilities into the
importance weights that correct a policy gradient on filtered or constrained samples.

Marginal likelihoods: `marginal` / `marginal_smiles` estimate log p(x) itself, the latent integrated out, by the
importance-weighted bound over K draws of the encoder's posterior (decode.marginal_logp; Burda et al.): one encoder
forward, the draws and their log p(z) - log q(z | x) from one launch per block (ops.latent_iw), score_tokens on the
block, and the bound, the ELBO and the effective sample size per molecule (ops.iw_combine).  The number is
log p(tokens behind the prefix | latent length, scaffold, conditions): the prior is N(0, I) over all of a molecule's own
latent rows, the latent length stays the encoder's, and no log p(toklen) term is added.

Fine-tuning on what was sampled: `return_rows=True` on `decode`, `sample_smiles` and `sample_multiple_smiles` appends a
`DecodedRows` -- the latents, mask, conditions and prefix lengths the decode consumed and the token rows it produced --
and `logp(*rows)` is `score(*rows)` WITH a gradient (decode.sequence_logp), on the device: the policy term of
Train/finetune.reinforce_step.  `policy_terms(*rows, prior=)` adds the policy's entropy and its KL divergence from a
frozen prior (decode.sequence_policy), the regularisers of that step.  `ppo_terms(*rows, old_token_logp=, advantage=,
clip=)` is PPO's clipped surrogate against the log-probabilities the rows were sampled with (decode.sequence_ppo), the
objective of Train/finetune.ppo_update's several updates per scored batch.  Not with beam search.

`well_formed=True` (optional): greedy / multinomial decodes are constrained by smiles.SmilesGrammar built from the target
vocabulary -- every returned string has balanced branches, paired ring-closure numbers, no dangling bond, and ended
with <eos> inside max_strlen.  Syntax only: no valence or aromaticity check (`check_rows` / `is_valid` below check the
decoded rows for those).  Not with beam search: the constructor
refuses decode_algo="beam", and `decode_beams` of such a sampler raises.

`check_rows(rows)` (any sampler): smiles.SmilesChemistry's check of decoded rows on the device, one launch -- a
ChemReport(status, position, atoms, ring_bonds) per row: valence caps, ring closures that double a bond or disagree on
its order, aromatic atoms outside an aromatic ring.  A necessary condition of validity, not a toolkit's verdict.
Train/finetune.validity_reward turns the report into the reward of reinforce_step / ppo_update; `is_valid(smiles)` is the
same verdict for one string, usable as accept= of interpolate_smiles.

`randomize_smiles(smiles_list, scaffold_list, k, seed)` (any sampler): k random spellings of every given molecule -- the
same graph written out by a random depth-first traversal (randomize.SmilesRandomizer, one launch, no rdkit), for
encode_smiles / score_smiles; the reference's randomize_smiles for callers.

`molecule_keys(rows or smiles)` / `basic_metrics(rows, index)` (any sampler): a spelling-independent 64-bit key per
molecule (molkey.SmilesKeys, one launch) and with it the reference's valid / unique / novel figures on the device --
`first_occurrence`, `MolKeyIndex` and Train/finetune.uniqueness_reward work on the same keys.

`fingerprints(rows or smiles)` / `snn(rows, ref)` / `basic_metrics(rows, index, int_div=True)` (any sampler): a 1024-bit
circular fingerprint per molecule (fingerprint.SmilesFingerprints, one launch) and the all-pairs Tanimoto figures over
them (gct_fp_tanimoto): similarity to the nearest neighbour in a fingerprint.FingerprintIndex, and `intDiv`, which
completes the reference's get_basic_metrics; Train/finetune.similarity_reward reads the same aggregates.

`descriptors(rows or smiles)` / `property_report(rows, targets)` (any sampler): twelve integer descriptors per molecule
-- atoms, hydrogens, molecular weight, charge, Lipinski's donor and acceptor counts, rotatable bonds, rings, aromatic
rings, TPSA, ring bonds (descriptor.SmilesDescriptors, one launch, no rdkit) -- and the reference's get_errors of target
minus computed property over them; Train/finetune.property_reward turns a column into a reward.

`murcko_scaffolds(rows or smiles)` (any sampler) / `scaffold_report(rows)` (a scaffold model): the Murcko scaffold of
every molecule -- key, spelling and kept atoms (scaffold.SmilesScaffolds, one launch, no rdkit) -- and, for rows that read
<sos> scaffold <sep> molecule <eos>, whether the molecule has the scaffold it was given: molkey.scaffold_metrics'
same_scaffold and Train/finetune.scaffold_reward read that report.

`decode_smc` (any sampler, any decode_algo): sequential Monte Carlo under the grammar (KVDecoder.generate_smc) -- k weighted
well-formed molecules per latent whose weighted distribution converges to the model's own distribution restricted to
well-formed strings, which a well_formed=True decode's locally renormalised draws do not follow, and an unbiased estimate
of the probability that an unconstrained sample is well formed.  decode.smc_row_weights turns the weights into the
`weight=` of Train/finetune.reinforce_step / ppo_update.

`stream_rows=R` (optional): greedy / multinomial decodes run with continuous batching (KVDecoder.generate_stream) -- the
n rows of a call are a pool that R decode rows work through, a row whose molecule reached <eos> taking the next one, so
`sample_smiles(30000)` is one call that never computes past a molecule's end.  Every decode of such a sampler goes that
way, also one of fewer than R rows (a single wave): what a molecule decodes then never depends on n or R.

`interpolate_smiles` (the reference's Inference/mol_interpolation.py, its fifth inference entry point): P pairs of
molecules x A interior alphas, every cell decoded from latents interpolated between the two endpoints' encodings
(ops.latent_stats / ops.latent_interp build them on the device) with the reference's retry ladder of rising noise -- the
tries of every cell are rows of ONE decode per round.  `reconstruct_smiles` is the exact-latent round trip (z = the
encoder's mean) that interpolation approximates.  Inference/mol_interpolation.py holds the rules and the deviations.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..Model.modules import get_src_mask
from ..data import Vocab, tokenize
from .mol_interpolation import Interpolation, interior_alphas, interp_plan, lerp, noise_ladder, run_ladder
from ..decode import (BEAM_ALPHA, KVDecoder, Marginal, PolicyTerms, PpoTerms, check_beam_size, check_ess_threshold,
                      check_particles, check_sample_filter, check_stream_model, check_stream_rows, generated_tokens,
                      marginal_logp, score_tokens, sequence_logp, sequence_policy, sequence_ppo)
from ..descriptor import DescRows, SmilesDescriptors, property_errors
from ..fingerprint import FpRows, SmilesFingerprints, snn as fp_snn
from ..molkey import MolKeys, SmilesKeys, basic_metrics
from ..scaffold import ScaffoldRows, SmilesScaffolds
from ..randomize import SmilesRandomizer
from ..smiles import ChemReport, SmilesChemistry, SmilesGrammar, check_grammar


BEAM_ALGOS = ("beam", "stochastic_beam")        # decode_algo values that decode k rows per sample in step (kv_src)


class Scores(NamedTuple):
    """What Sampling.score returns, on the CPU: logp [n] fp32 = log p(tokens | z, conditions, prefix), tokens [n] int32
    scored tokens (the <eos> included), hits [n] int32 of them the model's top choice under teacher forcing,
    token_logp [n, W] fp32 per column (0 on prefix and pad columns).  decode.score_reference states the rule."""
    logp: torch.Tensor
    tokens: torch.Tensor
    hits: torch.Tensor
    token_logp: torch.Tensor


class DecodedRows(NamedTuple):
    """What a greedy / multinomial decode consumed and produced (return_rows=True), on the sampler's device; the
    argument list of Sampling.score and Sampling.logp: zs [n, L_e, latent], ys int64 [n, L] the full token rows --
    prefix, generated tokens up to the row's first generated <eos>, pad behind it (the decoder goes on writing there and
    id_to_smi drops it: the rows hold exactly the molecules that were returned) --, src_mask bool [n, 1, L_e], dconds
    [n, n_c] or None, prefix_lens int64 [n] on the CPU (row r's prefix is ys[r, :prefix_lens[r]]; it is not scored)."""
    zs: torch.Tensor
    ys: torch.Tensor
    src_mask: torch.Tensor
    dconds: Optional[torch.Tensor]
    prefix_lens: torch.Tensor


def _rows_kw(return_rows):
    """The keyword of `decode` only when it is asked for: a `decode` with the earlier signature keeps working."""
    return {"return_rows": True} if return_rows else {}


def sample_token_lengths(data: Sequence[int], size: int, rng: np.random.Generator) -> np.ndarray:
    """Histogram of the training token lengths (one bin per integer) sampled by inverse CDF,
    plus half-bin Gaussian jitter, rounded (toklen_sampling.py:9-36, sampling_tool.py:75-81)."""
    data = np.asarray(data, dtype=float)
    nbins = max(1, int(data.max() - data.min()))
    count, edges = np.histogram(data, bins=nbins)
    pdf = count / count.sum()
    dx = edges[1] - edges[0]
    centres = edges[:-1] + 0.5 * dx
    cdf = np.concatenate([[0.0], np.cumsum(pdf)])
    u = rng.uniform(0, 1, size)
    idx = np.clip(np.argmax(cdf[None, :] >= u[:, None], axis=1) - 1, 0, nbins - 1)
    return np.rint(centres[idx] + dx * rng.normal(size=size) / 2).astype(int)


def pack_prefixes(rows: Sequence[Sequence[int]], pad_id: int):
    """Token-id rows of different lengths -> (ys0 [n, t0_max] int64 right-padded with pad_id, lens [n] int64)."""
    lens = [len(r) for r in rows]
    if not rows or min(lens) < 1:
        raise ValueError("pack_prefixes: every row needs at least one token")
    ys0 = torch.full((len(rows), max(lens)), pad_id, dtype=torch.long)
    for i, r in enumerate(rows):
        ys0[i, :len(r)] = torch.as_tensor(list(r), dtype=torch.long)
    return ys0, torch.as_tensor(lens, dtype=torch.long)


def group_by_length(lens):
    """Row indices grouped by prefix length, shortest first, input order within a group: [(length, idx int64)]."""
    lens = torch.as_tensor(lens).long().view(-1)
    return [(int(v), (lens == v).nonzero().view(-1)) for v in torch.unique(lens).tolist()]


def latent_setup_rows(extras, zs, toklen, latent_dim, sample_toklen, sample_z):
    """Per-row latent geometry of a mixed-scaffold batch: row r uses extras[r] + toklen[r] latent rows (its scaffold,
    <sep>, then the molecule), L_e = the maximum, src_mask [n, 1, L_e] marks each row's own rows.  zs (optional)
    [n, >= L_e, latent]; with zs and no toklen, toklen[r] = zs.size(1) - extras[r] (sample_smiles' rule per row).
    Returns (zs [n, L_e, latent], toklen list, src_mask)."""
    n = len(extras)
    if zs is not None:
        if zs.dim() != 3 or zs.size(0) != n:
            raise ValueError(f"zs must be [{n}, L_e, {latent_dim}], got {list(zs.shape)}")
        if toklen is None:
            toklen = [zs.size(1) - e for e in extras]
    elif toklen is None:
        toklen = list(sample_toklen(n))
    toklen = [int(t) for t in toklen]
    if len(toklen) != n:
        raise ValueError(f"toklen has {len(toklen)} entries for {n} rows")
    stop = torch.as_tensor(toklen, dtype=torch.long) + torch.as_tensor(list(extras), dtype=torch.long)
    if int(stop.min()) < 1:
        raise ValueError("every row needs at least one latent row")
    lat = int(stop.max())
    if zs is None:
        zs = sample_z(lat, n)
    elif zs.size(1) < lat:
        raise ValueError(f"zs has {zs.size(1)} latent rows, a row needs {lat}")
    else:
        zs = zs[:, :lat]
    src_mask = torch.arange(lat).expand(n, 1, lat) < stop.view(n, 1, 1)
    return zs, toklen, src_mask


class Sampling:
    uses_scaffold = uses_props = False          # what the model type's encode_smiles / sample_smiles take

    def __init__(self, model, SRC: Vocab, TRG: Vocab, latent_dim: int, max_strlen: int = 80,
                 cond_dim: int = 0, decode_algo: str = "greedy", toklen_data: Optional[Sequence[int]] = None,
                 scaler=None, device="cuda", seed: int = 0, use_graphs: bool = False, beam_size: int = 4,
                 beam_alpha: float = BEAM_ALPHA, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 temperature: float = 1.0, stream_rows: Optional[int] = None, with_logp: bool = False,
                 well_formed: bool = False, with_stats: bool = False):
        V = model.out.weight.shape[0]
        if well_formed and decode_algo in BEAM_ALGOS:
            raise ValueError(f"well_formed is not supported with decode_algo={decode_algo!r} (beam rows keep their history "
                             "behind the ancestry map)")
        self.TRG = TRG
        self._vocab_grammar = self._chemistry = self._keys = self._scaffolds = self._fingerprinter = self._describer = None
        # constrained decoding: the grammar over the target vocabulary, passed to every decode
        self.grammar = self.vocab_grammar if well_formed else None
        if with_logp and decode_algo in BEAM_ALGOS:
            raise ValueError(f"with_logp is not supported with decode_algo={decode_algo!r}: decode_beams / decode_unique "
                             "return the beams' scores, which are sums of log-probabilities already")
        if with_stats and decode_algo in BEAM_ALGOS:
            raise ValueError(f"with_stats is not supported with decode_algo={decode_algo!r}: decode_beams / decode_unique "
                             "return the beams' scores, which are sums of log-probabilities already")
        self.with_logp, self.with_stats = bool(with_logp), bool(with_stats)
        if stream_rows is not None:
            if decode_algo in BEAM_ALGOS:
                raise ValueError(f"stream_rows is not supported with decode_algo={decode_algo!r} (beam search keeps its "
                                 "rows in step)")
            check_stream_rows(stream_rows)
            check_stream_model(model, latent_dim)
        self.stream_rows = stream_rows
        if check_sample_filter(top_k, top_p, temperature, V) and decode_algo in BEAM_ALGOS:
            raise ValueError(f"top_k / top_p / temperature are not supported with decode_algo={decode_algo!r}")
        if decode_algo in BEAM_ALGOS:
            check_beam_size(beam_size, V)
        self.top_k, self.top_p, self.temperature = top_k, top_p, temperature
        self.beam_size, self.beam_alpha = beam_size, float(beam_alpha)
        self.model, self.SRC = model.eval(), SRC
        self.pad_id, self.sos_id, self.eos_id = SRC.stoi["<pad>"], TRG.stoi["<sos>"], TRG.stoi["<eos>"]
        self.sep_id = TRG.stoi.get("<sep>")
        self.add_sep = self.sep_id is not None
        self.latent_dim, self.max_strlen, self.cond_dim = latent_dim, max_strlen, cond_dim
        self.decode_algo, self.toklen_data, self.scaler = decode_algo, toklen_data, scaler
        self.device, self.use_graphs = device, use_graphs
        self.rng = np.random.default_rng(seed)
        self.gen = torch.Generator().manual_seed(seed)
        self.seed = seed
        self.latent_seed = seed                 # interpolate_smiles' latents: one stream per sampler, not per decode
        self.marginal_seed = seed               # marginal(seed=None): advanced once per call, so calls draw afresh
        self.kv = KVDecoder(model, self.pad_id, self.sos_id, self.eos_id)

    # ---- one of each SMILES object per vocabulary: the grammar serves well_formed, decode_smc, interpolate_smiles, the
    # chemistry check and the randomiser; the keys (and their randomiser) serve scaffolds, fingerprints and descriptors
    @property
    def vocab_grammar(self) -> SmilesGrammar:
        """The SmilesGrammar over the target vocabulary, built on first use (self.grammar is it, or None: whether a
        decode is constrained).  Its <pad> is the TARGET vocabulary's id, also for the chemistry check, the randomiser
        and the keys, which used to build their grammars with the source vocabulary's: the same id in every vocabulary
        pair data.py makes."""
        if self._vocab_grammar is None:
            self._vocab_grammar = SmilesGrammar(self.TRG.itos, self.TRG.stoi["<pad>"], self.TRG.stoi["<eos>"])
        return self._vocab_grammar

    def _smiles_rows(self, what, rows, scaffold_list=None, repeat=1):
        """THE row intake of the SMILES front ends -> (ys, start, W): `rows` a DecodedRows or (ys, prefix_lens), taken as
        they are (W None; a DecodedRows' scaffold_list is ignored, as it always was), or SMILES strings -- their ids and
        <eos>, behind `scaffold <sep>` with scaffold_list, <pad> to the widest row W, every row `repeat` times in a row,
        copied to the sampler's device, with zero starts on the CPU."""
        if isinstance(rows, DecodedRows):
            return rows.ys, rows.prefix_lens, None
        if isinstance(rows, tuple) and len(rows) == 2 and torch.is_tensor(rows[0]):
            if scaffold_list is not None:
                raise ValueError(f"{what}: scaffold_list goes with strings; token rows hold their scaffold")
            return (*rows, None)
        ids = [self.smi_to_id(s, add_eos=True) for s in rows]
        n = len(ids)
        if scaffold_list is not None:
            if not self.add_sep:
                raise ValueError("scaffold_list needs a scaffold model's vocabulary (no <sep> token here)")
            scaffold_list = list(scaffold_list)
            if len(scaffold_list) != n:
                raise ValueError(f"{len(scaffold_list)} scaffolds for {n} molecules")
            ids = [self.smi_to_id(c) + [self.sep_id] + r for c, r in zip(scaffold_list, ids)]
        W = max((len(r) for r in ids), default=1)
        ys = torch.tensor([r + [self.pad_id] * (W - len(r)) for r in ids], dtype=torch.int64).view(n, W)
        return ys.repeat_interleave(repeat, 0).to(self.device), torch.zeros(n * repeat, dtype=torch.int64), W

    # ---- chemical validity of decoded rows (smiles.SmilesChemistry: a check behind the decode, not a constraint on it)
    @property
    def chemistry(self) -> SmilesChemistry:
        """The SmilesChemistry over the target vocabulary, built on first use."""
        if self._chemistry is None:
            self._chemistry = SmilesChemistry(self.TRG.itos, self.pad_id, self.eos_id, grammar=self.vocab_grammar)
        return self._chemistry

    def check_rows(self, rows, prefix_lens=None) -> ChemReport:
        """The chemistry check of decoded rows on their device, one launch: `rows` a DecodedRows, or ys int64 [n, L]
        with prefix_lens ints [n].  ChemReport(status, position, atoms, ring_bonds), int32 [n] each; positions count
        from the row's first generated token."""
        if isinstance(rows, DecodedRows):
            rows, prefix_lens = rows.ys, rows.prefix_lens
        elif isinstance(rows, tuple) and len(rows) == 2 and prefix_lens is None:
            rows, prefix_lens = rows
        if prefix_lens is None:
            raise ValueError("check_rows: a DecodedRows, or (ys, prefix_lens)")
        return self.chemistry.check_rows(rows, prefix_lens)

    def is_valid(self, smiles, scaffold=None) -> bool:
        """True when `smiles` passes the chemistry check (its tokens and <eos>; a token outside the vocabulary is <unk>,
        which no SMILES holds).  `scaffold` is accepted and ignored, so that the method serves as accept= of
        interpolate_smiles whatever the model type."""
        return bool(smiles) and self.chemistry.valid(self.smi_to_id(smiles, add_eos=True))

    # ---- random spellings of given molecules (randomize.SmilesRandomizer: the reference's randomize_smiles, no rdkit)
    @property
    def randomizer(self) -> SmilesRandomizer:
        """The SmilesRandomizer over the target vocabulary: the keys'."""
        return self.keys.randomizer

    def randomize_smiles(self, smiles_list, scaffold_list=None, k=1, seed=0):
        """k random spellings of every molecule, for encode_smiles / score_smiles: one launch on the sampler's device.
        Returns (spellings, status): spellings[i] a list of k strings -- of k (scaffold, smiles) pairs with
        scaffold_list, both parts respelled on their own -- and status int32 [n, k, 2] on the CPU = the ops.RAND_* code
        of the molecule and of the scaffold (-1 without one).  A part that cannot be randomised (a stereo mark, a dot,
        a token outside the vocabulary, no room inside 256 tokens) comes back as it was written and its status says
        why.  Spelling j of molecule i is keyed i | j << 32 under `seed`: it does not depend on k or on the other
        molecules.  The same graph in another atom order: atoms and bond symbols are carried verbatim."""
        smiles_list, k = list(smiles_list), int(k)
        if k < 1:
            raise ValueError(f"k must be at least 1, got {k}")
        ys, start, W = self._smiles_rows("randomize_smiles", smiles_list, scaffold_list, repeat=k)
        n = len(smiles_list)
        key = torch.arange(n, dtype=torch.int64).view(n, 1) | (torch.arange(k, dtype=torch.int64).view(1, k) << 32)
        got = self.randomizer.randomize_rows(ys, start, key.reshape(-1), seed, 1.0, out_width=max(W, min(W + 32, 256)))
        out, tokens = [], got.tokens.cpu().tolist()
        for i in range(n):
            spell = []
            for row in tokens[i * k:(i + 1) * k]:
                ids = row[:row.index(self.eos_id)] if self.eos_id in row else row
                if scaffold_list is not None and self.sep_id in ids:
                    c = ids.index(self.sep_id)
                    spell.append((self.id_to_smi(ids[:c]), self.id_to_smi(ids[c + 1:])))
                else:
                    spell.append(self.id_to_smi(ids))
            out.append(spell)
        return out, got.info[:, :2].cpu().view(n, k, 2)

    # ---- molecule identity (molkey.SmilesKeys: uniqueness and novelty without moses or rdkit)
    @property
    def keys(self) -> SmilesKeys:
        """The SmilesKeys over the target vocabulary, built on first use, with its randomiser over self.vocab_grammar."""
        if self._keys is None:
            rz = SmilesRandomizer(self.TRG.itos, self.pad_id, self.eos_id, self.sep_id, grammar=self.vocab_grammar)
            self._keys = SmilesKeys(self.TRG.itos, self.pad_id, self.eos_id, self.sep_id, randomizer=rz)
        return self._keys

    def molecule_keys(self, rows, scaffold_list=None) -> MolKeys:
        """Spelling-independent 64-bit keys on the sampler's device, one launch: `rows` a DecodedRows or
        (ys, prefix_lens) -- the span behind a row's prefix is keyed, as check_rows reads it -- or SMILES strings, with
        scaffold_list as `scaffold <sep> molecule` rows whose two parts are keyed on their own.  MolKeys(key int64 [n, 2]
        = (molecule, scaffold or 0), info int32 [n, 4] = (ops.KEY_* status of the molecule, of the scaffold or -1, atoms,
        bonds)).  Equal keys: the same molecule as far as molkey's rule can tell; a part with a stereo mark, a dot or bad
        syntax is the same only as the same string."""
        return self.keys.key_rows(*self._smiles_rows("molecule_keys", rows, scaffold_list)[:2])

    def basic_metrics(self, rows, index=None, int_div=False) -> dict:
        """valid / unique / novel of decoded rows (molkey.basic_metrics, moses' definitions): check_rows, molecule_keys
        and the counting on the device, one read-back for the dict.  index: a molkey.MolKeyIndex of the training set
        (without one there is no `novel`).  int_div=True adds `intDiv`, moses' internal diversity over the valid rows
        (fingerprint.internal_diversity: one gct_smiles_fp and one gct_fp_tanimoto launch more), and n_fp, the valid
        rows that have a fingerprint -- the fourth figure of the reference's get_basic_metrics."""
        return basic_metrics(self.check_rows(rows), self.molecule_keys(rows), index,
                             self.fingerprints(rows) if int_div else None)

    # ---- fingerprints and Tanimoto figures (fingerprint.SmilesFingerprints: intDiv and SNN without moses or rdkit)
    @property
    def fingerprinter(self) -> SmilesFingerprints:
        """The SmilesFingerprints over the target vocabulary, next to self.keys, built on first use."""
        if self._fingerprinter is None:
            self._fingerprinter = SmilesFingerprints(self.TRG.itos, self.pad_id, self.eos_id, self.sep_id, keys=self.keys)
        return self._fingerprinter

    def fingerprints(self, rows) -> FpRows:
        """1024-bit circular fingerprints on the sampler's device, one launch: `rows` a DecodedRows or (ys, prefix_lens)
        -- the span behind a row's prefix is read as molecule_keys reads it, and of `scaffold <sep> molecule` the
        molecule is fingerprinted -- or SMILES strings.  FpRows(bits int64 [n, 16], info int32 [n, 4] = (ops.FP_* status,
        bits set, atoms, bonds)); a part with a stereo mark, a dot or bad syntax has no bit."""
        return self.fingerprinter.fp_rows(*self._smiles_rows("fingerprints", rows)[:2])

    def snn(self, rows, ref) -> float:
        """Similarity to the nearest neighbour (the reference's get_snn_from_mol): the mean over the rows that have a
        fingerprint of the largest Tanimoto similarity to `ref`, a fingerprint.FingerprintIndex (of a training set) or
        an FpRows.  `rows` as `fingerprints` takes them, or an FpRows.  0.0 if either side is empty.  One read-back."""
        return fp_snn(rows if isinstance(rows, FpRows) else self.fingerprints(rows), ref)

    # ---- molecular descriptors (descriptor.SmilesDescriptors: MW, Lipinski counts, rings and TPSA without rdkit)
    @property
    def describer(self) -> SmilesDescriptors:
        """The SmilesDescriptors over the target vocabulary, next to self.keys, built on first use."""
        if self._describer is None:
            self._describer = SmilesDescriptors(self.TRG.itos, self.pad_id, self.eos_id, self.sep_id, keys=self.keys)
        return self._describer

    def descriptors(self, rows) -> DescRows:
        """Integer descriptors on the sampler's device, one launch: `rows` a DecodedRows or (ys, prefix_lens) -- the span
        behind a row's prefix is read as molecule_keys reads it, and of `scaffold <sep> molecule` the molecule is
        described -- or SMILES strings.  DescRows(values int32 [n, 12]): the ops.DESC_* columns; a part with a stereo
        mark, a dot, bad syntax or an atom the rule does not know has a status other than DESC_OK and zeros."""
        return self.describer.desc_rows(*self._smiles_rows("descriptors", rows)[:2])

    def property_report(self, rows, targets, valid_only=True) -> dict:
        """The reference's get_errors of decoded rows against property targets: targets a dict column name (as
        DescRows.column takes it: `tpsa`, `mw`, `hbd`, ...) -> a number or one target per row; returns name ->
        {mae, mse, max, min, aard, amsd, n} (descriptor.property_errors) over the rows that are DESC_OK and, with
        valid_only, pass check_rows.  `rows` a DecodedRows or (ys, prefix_lens).  One read-back."""
        mask = (self.check_rows(rows).status == ops.CHEM_OK) if valid_only else None
        return property_errors(self.descriptors(rows), targets, mask)

    # ---- Murcko scaffolds (scaffold.SmilesScaffolds: the reference's murcko_scaffold and scaffold filter, no rdkit)
    @property
    def scaffolds(self) -> SmilesScaffolds:
        """The SmilesScaffolds over the target vocabulary, next to self.keys, built on first use."""
        if self._scaffolds is None:
            self._scaffolds = SmilesScaffolds(self.TRG.itos, self.pad_id, self.eos_id, self.sep_id, keys=self.keys)
        return self._scaffolds

    def murcko_scaffolds(self, rows):
        """The Murcko scaffold of every molecule on the sampler's device, one launch: `rows` a DecodedRows or
        (ys, prefix_lens) -- the span behind a row's prefix holds the molecule, as check_rows reads it -- or SMILES
        strings.  Returns (strings, ScaffoldRows): strings[i] the scaffold's spelling, "" for a row without one
        (info[i, 0] says why: ops.SCA_ACYCLIC, SCA_SYNTAX, SCA_UNSUPPORTED, ...).  One read-back, for the strings."""
        ys, start, W = self._smiles_rows("murcko_scaffolds", rows)
        got = self.scaffolds.scaffold_rows(ys, start, out_width=None if W is None else max(W, min(W + 32, 256)))
        return [self.id_to_smi(r) for r in got.tokens.cpu().tolist()], got

    def scaffold_report(self, rows) -> ScaffoldRows:
        """Does every decoded molecule have the scaffold it was asked for?  `rows`: a DecodedRows of a scaffold model, or
        (ys, prefix_lens), whose rows read <sos> scaffold <sep> molecule <eos> (mixed-scaffold batches are not
        left-padded: every row begins with <sos>, see the module notes).  One launch on the span behind <sos>, so that
        the kernel sees both parts: key[:, 0] is the key of the scaffold EXTRACTED from the molecule, key[:, 1] the key of
        the one given; scaffold.scaffold_match, molkey.scaffold_metrics and finetune.scaffold_reward read the result."""
        if not self.add_sep:
            raise ValueError("scaffold_report needs a scaffold model's vocabulary (no <sep> token here)")
        ys = rows.ys if isinstance(rows, DecodedRows) else rows[0]
        return self.scaffolds.scaffold_rows(ys, torch.ones(ys.shape[0], dtype=torch.int64))

    # ---- helpers with the reference's names ------------------------------------------------
    def init_y(self, n, add_sos=True, sca_ids=None, add_sep=False):
        ids = ([self.sos_id] if add_sos else []) + list(sca_ids or []) + ([self.sep_id] if add_sep else [])
        return torch.tensor([ids] * n, dtype=torch.long)

    def id_to_smi(self, ids) -> str:
        out = []
        for i in ids:
            i = int(i)
            if i == self.eos_id:
                break
            if i != self.sos_id:
                out.append(self.TRG.itos[i])
        return "".join(out)

    def smi_to_id(self, smi, add_sos=False, add_sep=False, add_eos=False) -> List[int]:
        ids = ([self.sos_id] if add_sos else []) + ([self.sep_id] if add_sep else [])
        ids += [self.TRG.stoi.get(t, self.TRG.stoi["<unk>"]) for t in tokenize(smi, self.add_sep)]
        return ids + ([self.eos_id] if add_eos else [])

    def sample_toklen(self, n):
        if self.toklen_data is None:
            raise ValueError("toklen_data (training-set token lengths) is required to sample lengths")
        return sample_token_lengths(self.toklen_data, n, self.rng) + self.cond_dim

    def sample_z(self, toklen, n):
        return torch.randn(n, toklen, self.latent_dim, generator=self.gen)

    def transform(self, prop):
        if self.scaler is not None:
            prop = self.scaler.transform(np.asarray(prop))
        return torch.as_tensor(np.asarray(prop), dtype=torch.float32)

    def tokenize_smiles(self, smiles_list):
        return self.SRC.encode_batch(list(smiles_list), self.add_sep, sos_eos=False)[0]

    # ---- decode: KV-cached equivalent of Sampling.decode (sampling_tool.py:140-184) ----------
    @torch.no_grad()
    def decode(self, zs, ys, src_mask, dconds=None, prefix_lens=None, return_rows=False):
        """ids [n, L] (prefix included); with decode_algo="beam" the best beam of each sample.
        prefix_lens (ints [n], optional): row r's prefix is ys[r, :t0_r] (KVDecoder.generate); not with beam search.
        The sampler's top_k / top_p / temperature apply to every draw (sample_smiles, sample_multiple_smiles).
        With stream_rows the n rows are a pool decoded by continuous batching; same layout, input order.
        with_logp (constructor): returns (ids, logp), logp [n] fp32 on the CPU = the model's log-probability of each
        row's generated tokens up to its <eos> (raw logits at temperature 1, whatever filter the draw went through).
        with_stats (constructor): a decode.StepStats on the CPU follows (behind logp when both are on) -- per generated
        token the model's entropy, the log-probability under the distribution the token was really drawn from (filter,
        temperature and grammar included), that distribution's entropy and its KL divergence from the model's, and
        behaviour_logp_sum [n] (KVDecoder.generate(return_stats=True)).
        return_rows=True appends a DecodedRows (what this decode consumed, and its token rows cut at each row's <eos>):
        `score(*rows)` / `logp(*rows)` score exactly what was decoded.  ValueError with beam search."""
        if return_rows and self.decode_algo == "beam":
            raise ValueError("return_rows is not supported with decode_algo='beam' (a beam row's history lies behind the "
                             "ancestry map; score the returned beams with score())")
        if self.decode_algo == "stochastic_beam":        # the first draw of each sample: an exact ordinary sample
            if return_rows:
                raise ValueError("return_rows is not supported with decode_algo='stochastic_beam': "
                                 "decode_unique(return_rows=True) returns the rows of all k draws")
            if prefix_lens is not None:
                raise ValueError("decode: beam search takes prefixes of one length (see sample_multiple_smiles)")
            return self.decode_unique(zs, ys, src_mask, dconds).ys[:, 0]
        if self.decode_algo == "beam":
            if prefix_lens is not None:
                raise ValueError("decode: beam search takes prefixes of one length (see sample_multiple_smiles)")
            return self.decode_beams(zs, ys, src_mask, dconds)[0][:, 0]
        self.seed += 1
        zs, ys, src_mask, dconds = self._start_rows(zs, ys, src_mask, dconds)
        kw = dict(algo=self.decode_algo, seed=self.seed, use_graphs=self.use_graphs, prefix_lens=prefix_lens,
                  top_k=self.top_k, top_p=self.top_p, temperature=self.temperature, return_logp=self.with_logp,
                  grammar=self.grammar, return_stats=self.with_stats)
        if self.stream_rows is not None:
            out = self.kv.generate_stream(ys, self.max_strlen, **kw)
            out = (out[0],) + tuple(out[2:])                       # (without the schedule's record)
        else:
            out = self.kv.generate(ys, self.max_strlen, **kw)
        if self.with_logp or self.with_stats:                      # (ys, [token_logp, logp], [StepStats])
            res = (out[0],) + ((out[2].cpu(),) if self.with_logp else ())
            if self.with_stats:
                res += (out[-1]._make(t.cpu() for t in out[-1]),)
        else:
            res = out[0] if self.stream_rows is not None else out
        return self._with_rows(res, zs, ys, src_mask, dconds, prefix_lens) if return_rows else res

    def _start_rows(self, zs, ys, src_mask, dconds, beams=None):
        """THE way a decode's inputs reach the decoder: the four tensors to the sampler's device (returned), and the
        decoder's rows started for them -- beams=k: k rows per sample in step (KVDecoder.start(beams=k)); None: the
        sampler's own rows, the pool of start_stream with stream_rows.  The rows are laid out for the prefix +
        max_strlen tokens, capped at the rows of the decoder's positional table, of which use_cond2dec spends n_c
        (KVDecoder.off) on the condition tokens."""
        zs, ys, src_mask = zs.to(self.device), ys.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        room = min(self.model.decoder.pe.pe.shape[1] - self.kv.off, ys.size(1) + self.max_strlen)
        if beams is None and self.stream_rows is not None:
            self.kv.start_stream(zs, src_mask, dconds, rows=self.stream_rows, max_total_len=room)
        else:
            self.kv.start(zs, src_mask, dconds, max_total_len=room, beams=beams or 1)
        return zs, ys, src_mask, dconds

    def _with_rows(self, res, zs, ys0, src_mask, dconds, prefix_lens):
        """decode's result with the DecodedRows of the call appended."""
        extras = self.with_logp or self.with_stats
        rows = self._decoded_rows(res[0] if extras else res, zs, ys0.size(1), src_mask, dconds, prefix_lens)
        return res + (rows,) if extras else (res, rows)

    def _decoded_rows(self, ids, zs, t0, src_mask, dconds, prefix_lens):
        """The DecodedRows of decoded ids [n, L] (prefixes of width t0, or prefix_lens): token rows cut at each row's
        first generated <eos>."""
        n, L = ids.shape
        lens = (torch.full((n,), t0, dtype=torch.long) if prefix_lens is None
                else torch.as_tensor(prefix_lens).to("cpu", torch.long).view(-1))
        cols = torch.arange(L, device=ids.device).view(1, -1)
        is_eos = (ids == self.eos_id) & (cols >= lens.to(ids.device).view(-1, 1))
        first = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full_like(is_eos[:, 0], L, dtype=torch.long))
        clean = torch.where(cols <= first.view(-1, 1), ids, torch.full_like(ids, self.pad_id))
        return DecodedRows(zs, clean, src_mask, dconds, lens)

    def logp(self, zs, ys, src_mask, dconds=None, prefix_lens=None) -> Scores:
        """`score` with a gradient (decode.sequence_logp): the same arguments -- a DecodedRows unpacks into them -- and
        the same values, but NOT under no_grad and on the DEVICE: logp [n] and token_logp [n, W] are attached to the
        graph of the decoder's parameters and model.out (and of zs when it requires grad).  One forward over all n rows,
        in the model's current train / eval mode."""
        zs, src_mask = zs.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        logp, tokens, hits, token_logp = sequence_logp(self.model, zs, src_mask, dconds, ys, prefix_lens=prefix_lens,
                                                       pad_id=self.pad_id)
        return Scores(logp, tokens, hits, token_logp)

    def policy_terms(self, zs, ys, src_mask, dconds=None, prefix_lens=None, prior=None) -> PolicyTerms:
        """`logp` plus the terms of a regularised policy-gradient step, from the same ONE forward
        (decode.sequence_policy): the entropy of the model's next-token distribution at every scored token and -- with
        `prior`, a second model of the same architecture (Train/finetune.frozen_prior) -- KL(model || prior) there and
        the prior's log-likelihood of the same tokens (one forward of the prior, no gradient).  The arguments of `logp`,
        so `policy_terms(*rows, prior=p)` takes a DecodedRows; PolicyTerms on the device, with gradients."""
        zs, src_mask = zs.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        return sequence_policy(self.model, zs, src_mask, dconds, ys, prefix_lens=prefix_lens, pad_id=self.pad_id,
                               prior=prior)

    def ppo_terms(self, zs, ys, src_mask, dconds=None, prefix_lens=None, *, old_token_logp, advantage, clip=0.2,
                  prior=None, entropy=False) -> PpoTerms:
        """PPO's clipped surrogate of decoded rows (decode.sequence_ppo), from ONE forward: the arguments of `logp` -- so
        `ppo_terms(*rows, old_token_logp=, advantage=)` takes a DecodedRows -- plus old_token_logp [n, W], the
        log-probabilities the rows were sampled with (`score(*rows).token_logp`, or `logp(*rows).token_logp` under
        no_grad, BEFORE the first update), one advantage per row, and clip: a number or (clip_lo, clip_hi).  prior /
        entropy add policy_terms' terms.  PpoTerms on the device; surrogate and token_surrogate carry the gradient."""
        zs, src_mask = zs.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        return sequence_ppo(self.model, zs, src_mask, dconds, ys, old_token_logp, advantage, clip=clip,
                            prefix_lens=prefix_lens, pad_id=self.pad_id, prior=prior, entropy=entropy)

    @torch.no_grad()
    def score(self, zs, ys, src_mask, dconds=None, prefix_lens=None) -> Scores:
        """Teacher-forced log-likelihood of the full token rows ys [n, W] (prefix, tokens, pad: the layout `decode`
        returns) under the latents zs, mask and conditions `decode` takes (decode.score_tokens).  Scores on the CPU."""
        zs, src_mask = zs.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        logp, tokens, hits, token_logp = score_tokens(self.model, zs, src_mask, dconds, ys, prefix_lens=prefix_lens,
                                                      pad_id=self.pad_id)
        return Scores(logp.cpu(), tokens.cpu(), hits.cpu(), token_logp.cpu())

    def _score_targets(self, smiles_list, scaffold_list=None):
        """<sos> [scaffold <sep>] smiles <eos> per molecule -> (ys [n, W] right-padded, prefix_lens or None, extras:
        latent rows in front of the molecule's own -- scaffold tokens + 1, or 0)."""
        smiles_list = list(smiles_list)
        if scaffold_list is None:
            rows = [[self.sos_id] + self.smi_to_id(s) + [self.eos_id] for s in smiles_list]
            return pack_prefixes(rows, self.pad_id)[0], None, [0] * len(rows)
        scaffold_list = list(scaffold_list)
        if len(scaffold_list) != len(smiles_list):
            raise ValueError(f"{len(smiles_list)} molecules for {len(scaffold_list)} scaffolds")
        sca = [self.smi_to_id(s) for s in scaffold_list]
        rows = [[self.sos_id] + c + [self.sep_id] + self.smi_to_id(s) + [self.eos_id] for c, s in zip(sca, smiles_list)]
        return (pack_prefixes(rows, self.pad_id)[0], torch.as_tensor([len(c) + 2 for c in sca], dtype=torch.long),
                [len(c) + 1 for c in sca])

    def _score_smiles(self, smiles_list, scaffold_list, conds, zs, transform=True):
        """What the types' score_smiles share (scaffolds / raw conds: None where the type has none).  zs None: the
        deterministic reconstruction score -- the latent is the encoder's MEAN of the same molecule and the mask the
        encoder's (_encode_endpoints).  zs given: latent_setup_rows' mask rule."""
        ys, lens, extras = self._score_targets(smiles_list, scaffold_list)
        if zs is None:
            zs, _, src_mask = self._encode_endpoints(smiles_list, scaffold_list, conds, transform)
        else:
            zs, _, src_mask = latent_setup_rows(extras, zs, None, self.latent_dim, self.sample_toklen, self.sample_z)
        return self.score(zs, ys, src_mask, self._conds(conds, transform), lens)

    @torch.no_grad()
    def marginal(self, mu, log_var, src_mask, ys, dconds=None, prefix_lens=None, K=64, seed=None, chunk=4096,
                 items=None, return_weights=False) -> Marginal:
        """Importance-weighted estimate of log p(x) of the full token rows ys [n, W] (`score`'s layout) from K draws of
        the posterior N(mu, exp(log_var)) -- mu, log_var [n, L_e, latent] and src_mask [n, 1, L_e] as the encoder gives
        them (decode.marginal_logp; decode.Marginal says what comes back).  Marginal on the CPU.
        seed None: the sampler's own counter, advanced once per call (two calls draw different latents); an int makes
        the call repeatable.  The draws of molecule i are keyed by (seed, items[i], k), items default arange(n)."""
        if seed is None:
            self.marginal_seed += 1
            seed = self.marginal_seed
        mu, log_var, src_mask = mu.to(self.device), log_var.to(self.device), src_mask.to(self.device)
        dconds = None if dconds is None else dconds.to(self.device)
        out = marginal_logp(self.model, mu, log_var, src_mask, dconds, ys, prefix_lens=prefix_lens, K=K, seed=seed,
                            items=items, chunk=chunk, pad_id=self.pad_id, return_weights=return_weights)
        return Marginal(*(None if t is None else t.cpu() for t in out))

    @torch.no_grad()
    def _marginal_smiles(self, smiles_list, scaffold_list, conds, transform=True, K=64, seed=None, chunk=4096,
                         return_weights=False):
        """What the types' marginal_smiles share: the targets of `score_smiles` (_score_targets), ONE encoder forward
        of the same molecules for mu, log_var and the encoder's own mask (_encode_endpoints), then `marginal`.
        The number is log p(tokens behind the prefix | latent length, scaffold, conditions): the prior is N(0, I) over
        ALL of the molecule's own latent rows (condition rows, scaffold, <sep>, tokens: what sample_z /
        latent_setup_rows draw from), the latent length is held at the encoder's, and the token-length histogram term
        log p(toklen) that sample_toklen draws from is NOT added."""
        smiles_list = list(smiles_list)
        ys, lens, _ = self._score_targets(smiles_list, scaffold_list)
        mu, log_var, src_mask = self._encode_endpoints(smiles_list, scaffold_list, conds, transform)
        return self.marginal(mu, log_var, src_mask, ys, self._conds(conds, transform), lens, K=K, seed=seed, chunk=chunk,
                             return_weights=return_weights)

    @torch.no_grad()
    def decode_beams(self, zs, ys, src_mask, dconds=None, beam_size=None, alpha=None):
        """Beam search: (ids [n, k, L], scores [n, k] sums of log-probabilities, lengths [n, k]), beams sorted by
        score / length**alpha (KVDecoder.generate_beam).  beam_size / alpha default to the constructor's."""
        if self.grammar is not None:
            raise ValueError("decode_beams: beam search takes no grammar, and this sampler was built with well_formed=True")
        k = self.beam_size if beam_size is None else beam_size
        check_beam_size(k, self.model.out.weight.shape[0])
        ys = self._start_rows(zs, ys, src_mask, dconds, beams=k)[1]
        return self.kv.generate_beam(ys, k, self.max_strlen, alpha=self.beam_alpha if alpha is None else alpha,
                                     use_graphs=self.use_graphs)

    @torch.no_grad()
    def decode_unique(self, zs, ys, src_mask, dconds=None, k=None, return_rows=False):
        """Stochastic beam search (KVDecoder.generate_sbs): k DISTINCT molecules per row of zs, an exact sample without
        replacement from the model's distribution for that latent, conditions and prefix.  Returns decode.SbsSamples
        (ys [n, k, L], logp [n, k], gumbel [n, k], lengths [n, k]) on the sampler's device, draws in drawing order: the
        first alone is an ordinary sample, and decode.sbs_importance_weights(logp, gumbel) weights all k into an unbiased
        estimator.  k defaults to the constructor's beam_size.  Any decode_algo (the sampler's filters and stream_rows do
        not apply: the draw is from the model's own distribution), but not well_formed=True samplers: ValueError.
        return_rows=True: (SbsSamples, DecodedRows) -- the n*k rows in sample-major order (row s*k + i: draw i of sample
        s), zs / src_mask / dconds repeated per draw, token rows cut at each row's <eos> as `decode` cuts them: what
        `logp(*rows)`, Train/finetune.reinforce_step and ppo_update take.  self.seed advances once per call."""
        if self.grammar is not None:
            raise ValueError("decode_unique: beam search takes no grammar, and this sampler was built with well_formed=True")
        k = self.beam_size if k is None else k
        check_beam_size(k, self.model.out.weight.shape[0])
        self.seed += 1
        zs, ys, src_mask, dconds = self._start_rows(zs, ys, src_mask, dconds, beams=k)
        out = self.kv.generate_sbs(ys, k, self.max_strlen, seed=self.seed, use_graphs=self.use_graphs)
        if not return_rows:
            return out
        rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
        ids = out.ys.reshape(-1, out.ys.shape[2])
        return out, self._decoded_rows(ids, rep(zs), ys.size(1), rep(src_mask), rep(dconds), None)

    @torch.no_grad()
    def decode_smc(self, zs, ys, src_mask, dconds=None, k=None, ess_threshold=0.5, return_rows=False):
        """Sequential Monte Carlo decoding under the SMILES grammar (KVDecoder.generate_smc): k weighted molecules per row
        of zs, every one well formed, whose weighted distribution converges to the model's OWN distribution restricted to
        well-formed strings -- where a well_formed=True decode draws from the locally renormalised one, biased towards
        what the mask favours -- and, per row, an unbiased estimate exp(log_z) of the probability that an unconstrained
        sample is well formed.  Returns decode.SmcSamples on the sampler's device.  k defaults to the constructor's
        beam_size; ess_threshold in [0, 1] is the share of k below which a sample resamples.  Any sampler type and any
        decode_algo: the grammar is the sampler's, or built from the target vocabulary when it has none (the sampler's
        filters and stream_rows do not apply).  No mixed prefixes, no streaming, k <= ops.BEAM_MAX_K.
        return_rows=True: (SmcSamples, DecodedRows) as decode_unique returns them; decode.smc_row_weights(samples) are the
        rows' weights for Train/finetune.reinforce_step(..., weight=) / ppo_update(..., weight=).  self.seed advances
        once per call.  ValueError for a bad ess_threshold or k, or max_strlen < 3, before any device work."""
        check_ess_threshold(ess_threshold)
        k = check_particles(self.beam_size if k is None else k, "decode_smc")
        grammar = self.vocab_grammar
        check_grammar(grammar, self.model.out.weight.shape[0], self.max_strlen - 1)
        self.seed += 1
        zs, ys, src_mask, dconds = self._start_rows(zs, ys, src_mask, dconds, beams=k)
        out = self.kv.generate_smc(ys, k, grammar, self.max_strlen, seed=self.seed, ess_threshold=ess_threshold,
                                   use_graphs=self.use_graphs)
        if not return_rows:
            return out
        rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
        ids = out.ys.reshape(-1, out.ys.shape[2])
        return out, self._decoded_rows(ids, rep(zs), ys.size(1), rep(src_mask), rep(dconds), None)

    # ---- molecule -> latent -> molecule ------------------------------------------------------
    def _endpoint_args(self, what, n, scaffolds, props):
        """The arguments the model type takes, checked: (scaffold list or None, raw property array [n, n_c] or None)."""
        if (scaffolds is not None) != self.uses_scaffold:
            raise ValueError(f"{what}: {type(self).__name__} takes {'a scaffold per molecule' if self.uses_scaffold else 'no scaffolds'}")
        if (props is not None) != self.uses_props:
            raise ValueError(f"{what}: {type(self).__name__} takes {'a property row per molecule' if self.uses_props else 'no properties'}")
        if scaffolds is not None:
            scaffolds = list(scaffolds)
            if len(scaffolds) != n:
                raise ValueError(f"{what}: {n} molecules for {len(scaffolds)} scaffolds")
        if props is not None:
            props = np.asarray(props, dtype=np.float64)
            if props.ndim != 2 or props.shape[0] != n:
                raise ValueError(f"{what}: {n} molecules for a property array of shape {list(props.shape)}")
        return scaffolds, props

    def _encoder_inputs(self, smiles, scaffolds=None, props=None, transform=True):
        """THE statement of what the encoder sees for this model type, on the sampler's device: (src, src_mask, econds).
        src int64 [n, L]: the tokens of scaffold<sep>smiles (uses_scaffold) or of smiles, right-padded; econds [n, n_c]:
        the raw properties through `_conds` (uses_props), else None; src_mask bool [n, 1, n_c + L]: the condition rows'
        flags, then the tokens' (get_src_mask).  An argument the type does not use is ignored."""
        strings = [b + "<sep>" + a for a, b in zip(smiles, scaffolds)] if self.uses_scaffold else smiles
        src = self.tokenize_smiles(strings).to(self.device)
        econds = self._conds(props, transform).to(self.device) if self.uses_props else None
        return src, get_src_mask(src, self.pad_id, econds), econds

    def _encode_endpoints(self, smiles, scaffolds, props, transform):
        """One encoder forward of the molecules -> (mu, log_var [n, L_e, latent], src_mask [n, 1, L_e] the encoder's own
        mask: condition rows, scaffold, <sep>, tokens)."""
        src, src_mask, econds = self._encoder_inputs(smiles, scaffolds, props, transform)
        _, mu, log_var = self.model.encode(src=src, src_mask=src_mask, econds=econds)
        return mu, log_var, src_mask

    def _conds(self, props, transform):
        """Raw property rows -> the fp32 conditions the model takes (through the scaler with transform); None: None."""
        if props is None:
            return None
        return self.transform(props) if transform else torch.as_tensor(props, dtype=torch.float32)

    def interpolate_smiles(self, src0, src1, n_interpolations=8, *, scaffolds0=None, scaffolds1=None, props0=None,
                           props1=None, ladder=None, chunk=16, accept=None, pair_ids=None, return_rows=False):
        """The call every type answers (`_interpolate` states it); the types' own front ends below take only what their
        encode_smiles / sample_smiles take, the property types with `transform` as there."""
        return self._interpolate(src0, src1, n_interpolations, scaffolds0=scaffolds0, scaffolds1=scaffolds1, props0=props0,
                                 props1=props1, ladder=ladder, chunk=chunk, accept=accept, pair_ids=pair_ids,
                                 return_rows=return_rows)

    @torch.no_grad()
    def _interpolate(self, src0, src1, n_interpolations=8, *, scaffolds0=None, scaffolds1=None, props0=None,
                     props1=None, ladder=None, chunk=16, accept=None, pair_ids=None, return_rows=False, transform=True):
        """Interpolate between the molecules src0[p] and src1[p] of P pairs at the A = n_interpolations interior alphas of
        np.linspace(0, 1, A + 2) (mol_interpolation.py of the reference; the module of that name here states the rules).
        One encode_smiles of all 2 P endpoints and one ops.latent_stats; then rounds: every unresolved (pair, alpha) cell
        sends its next `chunk` rungs of `ladder` (noise standard deviations; default noise_ladder()) as rows through one
        ops.latent_interp and one `decode` -- stream rows, grammar, graphs and filters as the sampler is configured --
        until every cell has an accepted row or the ladder is exhausted.  Rows of a round: cells in (pair, alpha) order,
        a cell's rungs ascending; row's latent rows = toklen of its cell (interp_plan), its random streams are keyed by
        item = (pair_id * A + alpha_index) * len(ladder) + rung, so a cell's latents do not depend on the other pairs of
        the call, on chunk or on the round (pair_ids: ints [P], default 0 .. P - 1; ValueError when an item does not fit
        int32) under the sampler's constructor seed.
        Scaffold types decode behind <sos> scaffolds0[p] <sep>, as the reference does; property types with the
        transformed lerp of the raw properties.  accept(smiles) -> bool; the default is SmilesGrammar.well_formed on the
        row's tokens and a non-empty string (syntax only -- a caller with rdkit passes its own).
        Returns an Interpolation; return_rows=True: (Interpolation, [DecodedRows of each round]).  ValueError with
        decode_algo="beam"."""
        if self.decode_algo in BEAM_ALGOS:
            raise ValueError(f"interpolate_smiles is not supported with decode_algo={self.decode_algo!r} (the retry ladder is one mixed "
                             "batch of greedy / multinomial rows)")
        src0, src1 = list(src0), list(src1)
        P = len(src0)
        if P < 1 or len(src1) != P:
            raise ValueError(f"interpolate_smiles: {P} first molecules for {len(src1)} second ones")
        sca0, props0 = self._endpoint_args("interpolate_smiles", P, scaffolds0, props0)
        sca1, props1 = self._endpoint_args("interpolate_smiles", P, scaffolds1, props1)
        alphas = interior_alphas(n_interpolations)
        ladder = noise_ladder() if ladder is None else np.asarray(ladder, dtype=np.float64).reshape(-1)
        if ladder.size < 1 or not np.all(ladder >= 0):
            raise ValueError("ladder: at least one noise standard deviation, none negative")
        A, K = alphas.size, ladder.size
        mu, log_var, mask = self._encode_endpoints(src0 + src1, None if sca0 is None else sca0 + sca1,
                                                   None if props0 is None else np.concatenate([props0, props1]),
                                                   transform)
        lens = mask.sum(-1).view(-1).cpu().numpy()
        prefixes = None
        if self.uses_scaffold:
            ys0_all, plens_all, extras = self._scaffold_prefixes(sca0)
            prefixes = (ys0_all, plens_all)
        toklen = interp_plan(lens[:P], lens[P:], alphas, extras if self.uses_scaffold else None)
        stats = ops.latent_stats(mu.contiguous(), log_var.contiguous(), lens)
        if accept is None:
            grammar = self.vocab_grammar
            verdict = lambda o: bool(o[0]) and grammar.well_formed(o[1])          # noqa: E731
        else:
            verdict = lambda o: bool(accept(o[0]))                                # noqa: E731
        decoded = []

        def decode_round(rnd):
            p, i = torch.as_tensor(rnd.pair), rnd.alpha
            tl = toklen[rnd.pair, i]
            T = int(tl.max())
            zs = ops.latent_interp(stats, rnd.pair, rnd.pair + P, alphas[i], ladder[rnd.tries], tl, rnd.item, T,
                                   self.latent_seed)
            src_mask = torch.arange(T).view(1, 1, T) < torch.as_tensor(tl).view(-1, 1, 1)
            dconds = None
            if self.uses_props:
                dconds = self._conds(lerp(props0[rnd.pair], props1[rnd.pair], alphas[i][:, None]), transform)
            if prefixes is None:
                outs = self.decode(zs, self.init_y(len(p)), src_mask, dconds, return_rows=True)
            else:
                pl = prefixes[1][p]
                outs = self.decode(zs, prefixes[0][p][:, :int(pl.max())], src_mask, dconds, prefix_lens=pl,
                                   return_rows=True)
            rows = self._split(outs, True)[1][-1]
            decoded.append(rows)
            gen = generated_tokens(rows.ys, rows.prefix_lens).cpu().numpy()
            return [(self.id_to_smi(g), g) for g in gen]

        tries, results, rows_decoded = run_ladder(P, A, K, chunk, pair_ids, decode_round, verdict)
        smiles = [[None if o is None else o[0] for o in row] for row in results]
        res = Interpolation(smiles, tries, np.where(tries >= 0, ladder[np.maximum(tries, 0)], np.nan), toklen,
                            rows_decoded)
        return (res, decoded) if return_rows else res

    @torch.no_grad()
    def reconstruct_smiles(self, smiles_list, scaffold_list=None, props=None, transform=True, return_rows=False):
        """The exact-latent round trip: encode the molecules and decode with z = the encoder's mean under the encoder's
        own mask (scaffold types behind <sos> scaffold <sep>, property types with the same properties).  Returns
        (smiles, same): the decoded strings and, per molecule, whether the decoded tokens equal the input's token for
        token; return_rows=True appends the DecodedRows.  ValueError with decode_algo="beam"."""
        if self.decode_algo in BEAM_ALGOS:
            raise ValueError(f"reconstruct_smiles is not supported with decode_algo={self.decode_algo!r}")
        smiles_list = list(smiles_list)
        sca, props = self._endpoint_args("reconstruct_smiles", len(smiles_list), scaffold_list, props)
        mu, _, src_mask = self._encode_endpoints(smiles_list, sca, props, transform)
        ys0, lens = (self.init_y(len(smiles_list)), None) if sca is None else self._scaffold_prefixes(sca)[:2]
        outs = self.decode(mu, ys0, src_mask, self._conds(props, transform), prefix_lens=lens, return_rows=True)
        rows = self._split(outs, True)[1][-1]
        gen = generated_tokens(rows.ys, rows.prefix_lens).cpu().tolist()
        ids = [g[:g.index(self.eos_id)] if self.eos_id in g else g for g in gen]
        out = ([self.id_to_smi(g) for g in ids], [g == self.smi_to_id(s) for g, s in zip(ids, smiles_list)])
        return out + (rows,) if return_rows else out

    def _latent_setup(self, n, zs, toklen, extra=0):
        if zs is not None:
            assert n == zs.size(0)
            if toklen is None:
                toklen = [zs.size(1) - extra] * n
        elif toklen is None:
            toklen = list(self.sample_toklen(n))
        lat = extra + max(toklen)
        if zs is None:
            zs = self.sample_z(lat, n)
        stop = torch.as_tensor(toklen, dtype=torch.long).view(n, 1, 1) + extra
        src_mask = torch.arange(lat).expand(n, 1, lat) < stop
        return zs, toklen, src_mask

    def _scaffold_prefixes(self, scaffolds):
        """<sos> scaffold <sep> per row -> (ys0 [n, t0_max], lens [n], extras: scaffold tokens + 1 per row)."""
        sca = [self.smi_to_id(s) for s in scaffolds]
        ys0, lens = pack_prefixes([[self.sos_id] + ids + [self.sep_id] for ids in sca], self.pad_id)
        return ys0, lens, [len(ids) + 1 for ids in sca]

    @torch.no_grad()
    def _sample_multiple(self, scaffolds, zs, toklen, dconds, return_rows=False):
        """One scaffold per row (sample_multiple_smiles): a single mixed-prefix decode, or for beam search one decode
        per prefix length; (smiles, toklen, toklen_gen) in input order (with_logp: and logp [n]; return_rows: and the
        DecodedRows)."""
        if return_rows and self.decode_algo in BEAM_ALGOS:
            raise ValueError(f"return_rows is not supported with decode_algo={self.decode_algo!r}")
        scaffolds = list(scaffolds)
        if not scaffolds:
            raise ValueError("sample_multiple_smiles: no scaffolds")
        ys0, lens, extras = self._scaffold_prefixes(scaffolds)
        zs, toklen, src_mask = latent_setup_rows(extras, zs, toklen, self.latent_dim, self.sample_toklen,
                                                 self.sample_z)
        n = len(scaffolds)
        tail = ()
        if self.decode_algo in BEAM_ALGOS:
            gens = [None] * n
            for t0, idx in group_by_length(lens):
                outs = self.decode(zs[idx], ys0[idx, :t0], src_mask[idx], None if dconds is None else dconds[idx])
                for i, row in zip(idx.tolist(), outs[:, t0:].cpu()):
                    gens[i] = row
        else:
            outs = self.decode(zs, ys0, src_mask, dconds, prefix_lens=lens, **_rows_kw(return_rows))
            outs, tail = self._split(outs, return_rows)
            gens = list(generated_tokens(outs, lens).cpu())
        smiles = [self.id_to_smi(g.numpy()) for g in gens]
        return (smiles, toklen, [len(tokenize(s, self.add_sep)) for s in smiles]) + tail

    def _split(self, outs, return_rows):
        """decode's result -> (ids, what follows them: logp with with_logp, the StepStats with with_stats, the
        DecodedRows with return_rows)."""
        if self.with_logp or self.with_stats or return_rows:
            return outs[0], tuple(outs[1:])
        return outs, ()

    def _finish(self, outs, toklen, skip=0, return_rows=False):
        """with_logp: `outs` is decode's (ids, logp) and logp becomes the fourth element; with_stats: the StepStats
        follows; return_rows: the DecodedRows the last one."""
        outs, tail = self._split(outs, return_rows)
        outs = outs.cpu().numpy()
        smiles = [self.id_to_smi(ids[skip:]) for ids in outs]
        return (smiles, toklen, [len(tokenize(s, self.add_sep)) for s in smiles]) + tail


class VaetfSampling(Sampling):
    def interpolate_smiles(self, src0, src1, n_interpolations=8, **kw):
        """Sampling._interpolate of molecules alone."""
        return self._interpolate(src0, src1, n_interpolations, **kw)

    def encode_smiles(self, smiles_list):
        src, src_mask, econds = self._encoder_inputs(smiles_list)
        return self.model.encode(src=src, src_mask=src_mask, econds=econds)

    def sample_smiles(self, n, zs=None, toklen=None, return_rows=False):
        zs, toklen, src_mask = self._latent_setup(n, zs, toklen)
        outs = self.decode(zs, self.init_y(n), src_mask, **_rows_kw(return_rows))
        return self._finish(outs, toklen, return_rows=return_rows)

    def score_smiles(self, smiles_list, zs=None) -> Scores:
        """log p(<sos> smiles <eos> | z): z = zs [n, L_e, latent], or (None) the encoder's mean of the same molecule."""
        return self._score_smiles(smiles_list, None, None, zs)

    def marginal_smiles(self, smiles_list, K=64, seed=None, chunk=4096, return_weights=False) -> Marginal:
        """Importance-weighted estimate of log p(<sos> smiles <eos> | latent length) from K posterior draws per molecule
        (Sampling._marginal_smiles says what the number is; decode.Marginal what comes back)."""
        return self._marginal_smiles(smiles_list, None, None, True, K, seed, chunk, return_weights)


class CvaetfSampling(Sampling):
    uses_props = True

    def interpolate_smiles(self, src0, src1, n_interpolations=8, *, props0=None, props1=None, transform=True, **kw):
        """Sampling._interpolate with a property row per endpoint (raw; transformed like encode_smiles' econds)."""
        return self._interpolate(src0, src1, n_interpolations, props0=props0, props1=props1, transform=transform, **kw)

    def encode_smiles(self, smiles_list, econds, transform=True):
        src, src_mask, econds = self._encoder_inputs(smiles_list, None, econds, transform)
        return self.model.encode(src=src, src_mask=src_mask, econds=econds)

    def sample_smiles(self, dconds, zs=None, toklen=None, transform=True, return_rows=False):
        n = len(dconds)
        dconds = self._conds(dconds, transform)
        if zs is None and toklen is not None:
            toklen = [t + self.cond_dim for t in toklen]
        zs, toklen, src_mask = self._latent_setup(n, zs, toklen)
        outs = self.decode(zs, self.init_y(n), src_mask, dconds, **_rows_kw(return_rows))
        return self._finish(outs, toklen, return_rows=return_rows)

    def score_smiles(self, smiles_list, conds, zs=None, transform=True) -> Scores:
        """log p(<sos> smiles <eos> | z, conds); zs None: the encoder's mean of (smiles, conds)."""
        return self._score_smiles(smiles_list, None, conds, zs, transform)

    def marginal_smiles(self, smiles_list, conds, K=64, seed=None, chunk=4096, transform=True,
                        return_weights=False) -> Marginal:
        """Importance-weighted estimate of log p(<sos> smiles <eos> | latent length, conds); the encoder sees
        (smiles, conds), as in score_smiles(zs=None)."""
        return self._marginal_smiles(smiles_list, None, conds, transform, K, seed, chunk, return_weights)


class ScaVaeSampling(Sampling):
    uses_scaffold = True

    def interpolate_smiles(self, src0, src1, n_interpolations=8, *, scaffolds0=None, scaffolds1=None, **kw):
        """Sampling._interpolate with a scaffold per endpoint; rows decode behind <sos> scaffolds0[p] <sep>."""
        return self._interpolate(src0, src1, n_interpolations, scaffolds0=scaffolds0, scaffolds1=scaffolds1, **kw)

    def encode_smiles(self, smiles_list, scaffold_list):
        src, src_mask, econds = self._encoder_inputs(smiles_list, scaffold_list)
        return self.model.encode(src=src, src_mask=src_mask, econds=econds)

    def sample_smiles(self, n, scaffold, zs=None, toklen=None, return_rows=False):
        sca_ids = self.smi_to_id(scaffold)
        zs, toklen, src_mask = self._latent_setup(n, zs, toklen, extra=len(sca_ids) + 1)
        outs = self.decode(zs, self.init_y(n, True, sca_ids, True), src_mask, **_rows_kw(return_rows))
        return self._finish(outs, toklen, skip=1 + len(sca_ids) + 1, return_rows=return_rows)

    def score_smiles(self, smiles_list, scaffold_list, zs=None) -> Scores:
        """log p(smiles <eos> | <sos> scaffold <sep>, z), one scaffold per molecule (the prefix is not scored); zs None:
        the encoder's mean of scaffold <sep> smiles."""
        return self._score_smiles(smiles_list, scaffold_list, None, zs)

    def marginal_smiles(self, smiles_list, scaffold_list, K=64, seed=None, chunk=4096, return_weights=False) -> Marginal:
        """Importance-weighted estimate of log p(smiles <eos> | <sos> scaffold <sep>, latent length), one scaffold per
        molecule (the prefix is not scored); the encoder sees scaffold <sep> smiles."""
        return self._marginal_smiles(smiles_list, scaffold_list, None, True, K, seed, chunk, return_weights)

    def sample_multiple_smiles(self, scaffolds, zs=None, toklen=None, return_rows=False):
        """One molecule per scaffold, all rows in one batch: row r decodes as sample_smiles(1, scaffolds[r]) with z
        row zs[r] and token length toklen[r] would (latent rows len(scaffold tokens) + 1 + toklen[r])."""
        return self._sample_multiple(scaffolds, zs, toklen, None, return_rows)


class PscavaetfSampling(Sampling):
    uses_scaffold = uses_props = True

    def interpolate_smiles(self, src0, src1, n_interpolations=8, *, scaffolds0=None, scaffolds1=None, props0=None,
                           props1=None, transform=True, **kw):
        """Sampling._interpolate with a scaffold and a property row per endpoint."""
        return self._interpolate(src0, src1, n_interpolations, scaffolds0=scaffolds0, scaffolds1=scaffolds1,
                                 props0=props0, props1=props1, transform=transform, **kw)

    def encode_smiles(self, smiles_list, scaffold_list, econds, transform=True):
        src, src_mask, econds = self._encoder_inputs(smiles_list, scaffold_list, econds, transform)
        return self.model.encode(src=src, src_mask=src_mask, econds=econds)

    def sample_smiles(self, dconds, scaffold, zs=None, toklen=None, transform=True, return_rows=False):
        """prefix = <sos> scaffold <sep> (sampling_tool.py:452-498)."""
        n = len(dconds)
        dconds = self._conds(dconds, transform)
        sca_ids = self.smi_to_id(scaffold)
        zs, toklen, src_mask = self._latent_setup(n, zs, toklen, extra=len(sca_ids) + 1)
        outs = self.decode(zs, self.init_y(n, True, sca_ids, True), src_mask, dconds, **_rows_kw(return_rows))
        return self._finish(outs, toklen, skip=1 + len(sca_ids) + 1, return_rows=return_rows)

    def score_smiles(self, smiles_list, scaffold_list, conds, zs=None, transform=True) -> Scores:
        """log p(smiles <eos> | <sos> scaffold <sep>, z, conds), one scaffold per molecule; zs None: the encoder's mean
        of (scaffold <sep> smiles, conds)."""
        return self._score_smiles(smiles_list, scaffold_list, conds, zs, transform)

    def marginal_smiles(self, smiles_list, scaffold_list, conds, K=64, seed=None, chunk=4096, transform=True,
                        return_weights=False) -> Marginal:
        """Importance-weighted estimate of log p(smiles <eos> | <sos> scaffold <sep>, latent length, conds), one
        scaffold per molecule; the encoder sees (scaffold <sep> smiles, conds)."""
        return self._marginal_smiles(smiles_list, scaffold_list, conds, transform, K, seed, chunk, return_weights)

    def sample_multiple_smiles(self, dconds, scaffolds, zs=None, toklen=None, transform=True, return_rows=False):
        """The reference's intended sample_multiple_smiles (sampling_tool.py, commented out there): row r has the
        properties dconds[r] and the scaffold scaffolds[r]; all rows are one batch and row r decodes as
        sample_smiles(dconds[r:r+1], scaffolds[r]) would."""
        if len(dconds) != len(scaffolds):
            raise ValueError(f"{len(dconds)} property rows for {len(scaffolds)} scaffolds")
        dconds = self._conds(dconds, transform)
        return self._sample_multiple(scaffolds, zs, toklen, dconds, return_rows)


sampling_tool_dict = {
    "vaetf": VaetfSampling,
    "pvaetf": CvaetfSampling,
    "scavaetf": ScaVaeSampling,
    "pscavaetf": PscavaetfSampling,
}


def get_sampler(model_type, model, SRC, TRG, **kwargs):
    """Model/build_model.py:90-116 counterpart."""
    return sampling_tool_dict[model_type](model, SRC, TRG, **kwargs)
