"""Latent-space interpolation between molecules: the reference's Inference/mol_interpolation.py (approximate_z,
interpolate_z_pair, the retry loop of interpolate_smiles, :124-141 and :192-259) on the batched decoder.

The reference handles one pair, one alpha and one attempt at a time: it fits a per-dimension Gaussian to the per-token
mu and log_var of each endpoint, draws a fresh latent of the interpolated length from each fit, slerps them token by
token, adds noise of a slowly rising standard deviation, decodes ONE row, asks rdkit whether it parses, and retries --
up to 400 times per cell.  Every attempt is independent of every other, so here the attempts of every (pair, alpha) cell
are rows of one decode (Sampling.interpolate_smiles), and the latents in front of the decoder are built on the device
(ops.latent_stats / ops.latent_interp, csrc/latent.hip).  This module holds the host side: the interpolation rules on
arrays, the plan, the ladder and the round loop -- all pure, none of it needs a GPU -- and SmilesInterpolation, the
reference's class over a sampler.

Deliberate deviations:
  * token length: toklen = int(lerp(len0, len1, alpha)).  The reference passes z1.size(0) twice (:134), so there every
    interpolated latent has the first molecule's length; that is a bug, and the second length is used here;
  * a molecule of one latent row has standard deviation 0 (torch.std gives NaN);
  * slerp falls back to lerp when an endpoint is zero or the two are (anti)parallel to within SLERP_MAX_COS (the
    reference divides by zero);
  * the retry ladder is decoded `chunk` rungs at a time; the result is the LOWEST accepted rung of a cell, which is what
    the one-at-a-time loop stops at (the rungs above it are decoded and dropped);
  * acceptance is syntactic by default (smiles.SmilesGrammar.well_formed and a non-empty string) -- rdkit stays outside
    the package; a caller that has it passes `accept=`.  No CSV files, plots or Tanimoto figures.
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

SLERP_MAX_COS = 1.0 - 2.0 ** -20            # GCT_LATENT_SLERP_MAX_COS (include/gctplus_hip.h)


def lerp(v1, v2, alpha):
    return v1 * (1 - alpha) + v2 * alpha


def slerp(v1, v2, alpha):
    """Spherical interpolation over the LAST axis of two numpy arrays or two tensors: with c = v1.v2 / (|v1| |v2|) and
    w = acos(c), (sin((1 - alpha) w) v1 + sin(alpha w) v2) / sin(w); not renormalised.  Where |v1| == 0, |v2| == 0 or
    not |c| <= SLERP_MAX_COS the result is the lerp, evaluated as v1 + alpha (v2 - v1) (v1 == v2 gives v1 exactly)."""
    is_torch = isinstance(v1, torch.Tensor) and isinstance(v2, torch.Tensor)
    xp = torch if is_torch else np
    if not is_torch:
        v1, v2 = np.asarray(v1), np.asarray(v2)
    n1, n2 = ((v * v).sum(-1, keepdims=True) ** 0.5 if not is_torch else (v * v).sum(-1, keepdim=True) ** 0.5
              for v in (v1, v2))
    dot = (v1 * v2).sum(-1, keepdim=True) if is_torch else (v1 * v2).sum(-1, keepdims=True)
    den = n1 * n2
    ok = den != 0
    c = dot / xp.where(ok, den, xp.ones_like(den))
    ok = ok & (abs(c) <= SLERP_MAX_COS)
    w = (torch.acos if is_torch else np.arccos)(xp.where(ok, c, xp.zeros_like(c)))       # the guard's lanes: acos(0)
    out = (xp.sin((1 - alpha) * w) * v1 + xp.sin(alpha * w) * v2) / xp.sin(w)
    return xp.where(ok, out, v1 + alpha * (v2 - v1))


def interior_alphas(n_interpolations: int) -> np.ndarray:
    """The reference's alphas without the two endpoints (:200-206)."""
    if int(n_interpolations) < 1:
        raise ValueError(f"n_interpolations must be >= 1, got {n_interpolations}")
    return np.linspace(0, 1, int(n_interpolations) + 2)[1:-1]


def interp_plan(lens0, lens1, alphas, extras=None) -> np.ndarray:
    """The cell table: toklen int64 [P, A], cell (p, i) decoding from int(lerp(lens0[p], lens1[p], alphas[i])) latent
    rows -- lens0 / lens1 the latent rows of the two endpoints (condition rows, scaffold and <sep> included).  The
    reference takes the first molecule's length for both arguments (mol_interpolation.py:134), a bug: with
    lens0 != lens1 the lengths here move from one to the other.  extras (ints [P], optional): latent rows the decode
    prefix of pair p occupies (scaffold tokens + 1); ValueError when a cell would get fewer than extras[p] + 1 rows."""
    lens0, lens1 = np.asarray(lens0, dtype=np.int64).reshape(-1), np.asarray(lens1, dtype=np.int64).reshape(-1)
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1)
    if lens0.shape != lens1.shape:
        raise ValueError(f"{lens0.size} first molecules for {lens1.size} second ones")
    if lens0.size and min(lens0.min(), lens1.min()) < 1:
        raise ValueError("every molecule needs at least one latent row")
    toklen = np.array([[int(lerp(int(l0), int(l1), float(al))) for al in alphas] for l0, l1 in zip(lens0, lens1)],
                      dtype=np.int64).reshape(lens0.size, alphas.size)
    need = np.ones(lens0.size, dtype=np.int64) if extras is None else np.asarray(extras, dtype=np.int64).reshape(-1) + 1
    if need.shape != lens0.shape:
        raise ValueError(f"{need.size} prefixes for {lens0.size} pairs")
    short = toklen < need[:, None]
    if short.any():
        p, i = (int(x[0]) for x in np.nonzero(short))
        raise ValueError(f"pair {p}, alpha {alphas[i]:.3f}: {int(toklen[p, i])} latent rows, but the prefix takes "
                         f"{int(need[p]) - 1} and the molecule needs at least one")
    return toklen


def noise_ladder(step: float = 0.005, tries_per_std: int = 2, max_std: float = 1.0) -> np.ndarray:
    """The reference's retry schedule (:210-259) as an array, one entry per try: the noise standard deviation starts at
    0, rises by `step` after every `tries_per_std` tries (by repeated addition, as there), and the loop gives up once
    it reaches max_std -- 0, 0, .005, .005, ..., 400 tries with the defaults."""
    if not (step > 0 and max_std > 0 and int(tries_per_std) >= 1):
        raise ValueError("noise_ladder: step, max_std > 0 and tries_per_std >= 1")
    out, std = [], 0.0
    while std < max_std:
        out += [std] * int(tries_per_std)
        std += step
    return np.asarray(out, dtype=np.float64)


def first_accepted(flags) -> np.ndarray:
    """flags bool [P, A, K] -> int64 [P, A]: the lowest accepted try of each cell, -1 where there is none."""
    flags = np.asarray(flags, dtype=bool)
    if flags.shape[-1] == 0:
        return np.full(flags.shape[:-1], -1, dtype=np.int64)
    return np.where(flags.any(-1), flags.argmax(-1), -1).astype(np.int64)


def item_keys(pair_ids, n_alphas: int, n_tries: int) -> np.ndarray:
    """int64 [P, A, K]: the identity of every (pair, alpha, try) for the random streams of gct_latent_interp,
    (pair_id * A + alpha_index) * K + try_index.  ValueError when one does not fit int32."""
    pair_ids = np.asarray(pair_ids, dtype=np.int64).reshape(-1)
    if pair_ids.size and pair_ids.min() < 0:
        raise ValueError("pair_ids must be >= 0")
    if pair_ids.size and (int(pair_ids.max()) * n_alphas + n_alphas) * n_tries > 2 ** 31:
        raise ValueError(f"pair id {int(pair_ids.max())} with {n_alphas} alphas and {n_tries} tries: the item key "
                         "does not fit int32")
    cell = pair_ids[:, None] * n_alphas + np.arange(n_alphas, dtype=np.int64)[None, :]
    return cell[:, :, None] * n_tries + np.arange(n_tries, dtype=np.int64)[None, None, :]


class Round(NamedTuple):
    """The rows of one round, in decode order: cells in (pair, alpha) order, the tries of a cell ascending."""
    pair: np.ndarray            # int64 [n] index into the call's pairs
    alpha: np.ndarray           # int64 [n] index into the alphas
    tries: np.ndarray           # int64 [n] rung of the ladder
    item: np.ndarray            # int64 [n] item key


def run_ladder(n_pairs: int, n_alphas: int, n_tries: int, chunk: int, pair_ids, decode_round: Callable[[Round], Sequence],
               accept: Callable[[object], bool]):
    """The round loop.  Every unresolved cell sends its next `chunk` rungs into one decode_round(Round) -> one result
    per row; accept(result) -> bool; a cell is resolved by its LOWEST accepted rung, so the outcome does not depend on
    `chunk`.  Ends when every cell is resolved or the ladder is exhausted.
    Returns (tries int64 [P, A] (-1: unresolved), results [P][A] (the accepted one or None), rows_decoded)."""
    if int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    pair_ids = np.arange(n_pairs) if pair_ids is None else np.asarray(pair_ids, dtype=np.int64).reshape(-1)
    if pair_ids.size != n_pairs:
        raise ValueError(f"{pair_ids.size} pair ids for {n_pairs} pairs")
    keys = item_keys(pair_ids, n_alphas, n_tries)
    tries = np.full((n_pairs, n_alphas), -1, dtype=np.int64)
    results: List[List[Optional[object]]] = [[None] * n_alphas for _ in range(n_pairs)]
    rows_decoded = 0
    for k0 in range(0, n_tries, int(chunk)):
        cells = np.argwhere(tries < 0)
        if not len(cells):
            break
        ks = np.arange(k0, min(k0 + int(chunk), n_tries), dtype=np.int64)
        p, i, k = np.repeat(cells[:, 0], ks.size), np.repeat(cells[:, 1], ks.size), np.tile(ks, len(cells))
        rnd = Round(p, i, k, keys[p, i, k])
        out = list(decode_round(rnd))
        if len(out) != p.size:
            raise ValueError(f"decode_round returned {len(out)} results for {p.size} rows")
        rows_decoded += p.size
        flags = np.array([bool(accept(o)) for o in out], dtype=bool).reshape(len(cells), ks.size)
        for c, first in enumerate(first_accepted(flags[None])[0]):
            if first >= 0:
                tries[cells[c, 0], cells[c, 1]] = ks[first]
                results[cells[c, 0]][cells[c, 1]] = out[c * ks.size + first]
    return tries, results, rows_decoded


class Interpolation(NamedTuple):
    """What Sampling.interpolate_smiles returns: smiles [P][A] (None where no rung was accepted), tries int64 [P, A]
    (the accepted rung, -1), noise_std float64 [P, A] (the ladder's value at that rung, NaN), toklen int64 [P, A]
    latent rows of the cell, rows_decoded: rows that went through the decoder."""
    smiles: List[List[Optional[str]]]
    tries: np.ndarray
    noise_std: np.ndarray
    toklen: np.ndarray
    rows_decoded: int


class SmilesInterpolation:
    """The reference's class over one of this package's samplers, chemistry-free: records instead of files.
    sampler: a gct_plus_amd.Inference.sampling_tool sampler (greedy or multinomial)."""

    def __init__(self, sampler, n_interpolations: int = 8, ladder=None, chunk: int = 16, accept=None, transform=True):
        self.sampler = sampler
        self.n_interpolations, self.ladder, self.chunk, self.accept = n_interpolations, ladder, chunk, accept
        self.transform = transform              # property types: props_0 / props_1 are raw and go through the scaler

    def approximate_z(self, mu, log_var, rows):
        """The per-dimension Gaussian fits of the reference's approximate_z for n molecules at once: mu, log_var
        [n, L_e, D] on the device, rows [n] the latent rows each molecule owns -> stats [n, 4, D] (ops.latent_stats)."""
        from .. import ops
        return ops.latent_stats(mu.contiguous(), log_var.contiguous(), rows)

    def interpolate_z_pair(self, stats, a, b, alpha, toklen, noise_std=0.0, item=0, seed=0):
        """One interpolated latent [1, toklen, D] between molecules a and b of stats (ops.latent_interp): the
        reference's interpolate_z_pair of mu and of log_var and its reparameterisation, in one launch."""
        from .. import ops
        return ops.latent_interp(stats, [a], [b], [alpha], [noise_std], [toklen], [item], toklen, seed)

    def interpolate_smiles(self, pairs):
        """pairs: a DataFrame (or a list of dicts) with the reference's columns src_0, src_1 and, as the sampler's type
        needs them, scaffold_0, scaffold_1 and props_0, props_1 (one property vector per cell).  Returns a DataFrame with
        one record per (pair, alpha): pair, alpha, smiles (None when the ladder was exhausted), try, noise_std, toklen."""
        import pandas as pd
        df = pairs if isinstance(pairs, pd.DataFrame) else pd.DataFrame(list(pairs))
        kw = {}
        if "scaffold_0" in df.columns:
            kw.update(scaffolds0=list(df["scaffold_0"]), scaffolds1=list(df["scaffold_1"]))
        if "props_0" in df.columns:
            kw.update(props0=np.stack([np.asarray(v, dtype=np.float64) for v in df["props_0"]]),
                      props1=np.stack([np.asarray(v, dtype=np.float64) for v in df["props_1"]]),
                      transform=self.transform)
        res = self.sampler.interpolate_smiles(list(df["src_0"]), list(df["src_1"]), self.n_interpolations,
                                              ladder=self.ladder, chunk=self.chunk, accept=self.accept, **kw)
        alphas = interior_alphas(self.n_interpolations)
        recs = [dict(pair=df.index[p], alpha=float(al), smiles=res.smiles[p][i], **{"try": int(res.tries[p, i])},
                     noise_std=float(res.noise_std[p, i]), toklen=int(res.toklen[p, i]))
                for p in range(len(df)) for i, al in enumerate(alphas)]
        return pd.DataFrame(recs, columns=["pair", "alpha", "smiles", "try", "noise_std", "toklen"])
