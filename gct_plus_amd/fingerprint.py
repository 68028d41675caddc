"""Circular fingerprints and Tanimoto metrics (what the reference's Inference/metrics.py takes from rdkit and moses for
`intDiv` -- the fourth figure of get_basic_metrics -- and for get_snn_from_mol, without either): a Morgan-style
1024-bit fingerprint of the labelled graph that randomize.SmilesRandomizer.parse reads from a token row, all-pairs
Tanimoto aggregates over such fingerprints, and what they are for -- internal diversity, similarity to the nearest
neighbour in a reference set, an index of a training set's fingerprints, a similarity reward.

SmilesFingerprints.fingerprint is THE statement for one part, fp_reference the batch rule; gct_smiles_fp
(csrc/fingerprint.hip, SmilesFingerprints.fp_rows) implements them and is compared with them bit for bit.
tanimoto_reference is THE statement of the aggregates; gct_fp_tanimoto (the same file, tanimoto_agg) implements it.

The fingerprint.  All arithmetic is in uint64 and wraps.  mix, the atom label L(a) (the FNV-1a hash of the token's
STRING) and the bond label o(e) are exactly molkey's.
  1. id_0(a) = mix(L(a) ^ mix(0x200 + deg(a))), deg the number of bonds of a in the parsed graph
  2. id_{r+1}(a) = mix(3 id_r(a) + sum over bonds (b, o) of a of mix(id_r(b) ^ mix(o + 0x100))): molkey's refinement
  3. for r = 0 .. ops.FP_RADIUS (2) and every atom, bit id_r(a) mod ops.FP_BITS (1024) is set
  4. 16 uint64 words: word w holds bits 64 w .. 64 w + 63, bit k at 1 << (k & 63)
A part without a graph -- it does not parse (FP_SYNTAX), or the randomiser's UNSUPPORTED set applies: a / or \\ bond, an
@ atom, a dot, a RING_BOND closure, a ninth bond (FP_UNSUPPORTED) -- has all-zero words.  A popcount of 0 is the only
"absent" marker the Tanimoto side knows.

Tanimoto.  c = popcount(a & b), u = |a| + |b| - c, T = (float)c / (float)u correctly rounded to fp32; T^2 is the fp64
product of that fp32 value with itself, so every term of a sum is exact in fp64 and only the order of the additions can
differ between two implementations.  Maxima are decided by integer cross-multiplication, and the lowest index wins a tie.

Limits, on purpose.  These are NOT rdkit's bit positions: the figures compare between runs of this code, not with
published MOSES tables.  Duplicate environments are not removed -- a radius whose neighbourhood did not grow still sets
its bit.  There is no ring-membership, implicit-hydrogen or chirality invariant beyond what the token string carries
([CH3] differs from C, a Kekule spelling from an aromatic one).  A fingerprint is not identity: non-isomorphic graphs
whose atoms see the same radius-2 neighbourhoods (decalin and bicyclopentyl) share one; the keys of molkey.py are for
identity.  Stereo and dotted rows have no fingerprint at all."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .molkey import SmilesKeys, as_int64, mix
from .smiles import chunked, launch_rows, on_device, row_mask, row_spans

_M = 0xFFFFFFFFFFFFFFFF


class FpRows(NamedTuple):
    """What fp_rows / fp_reference return.  bits int64 [n, 16]: the fingerprint's words; info int32 [n, 4] = (status,
    number of bits set, atoms, bonds); a row without <eos> in its span has no bit and info (-1, 0, 0, 0)."""
    bits: torch.Tensor
    info: torch.Tensor


class TanimotoAgg(NamedTuple):
    """What tanimoto_agg / tanimoto_reference return for the rows of a against b.  best fp32 [n]: the largest T over the
    present rows of b; arg int32 [n]: the lowest row of b that attains it; total fp64 [n]: the sum of T^p over them;
    present: the number of present rows of b (a scalar int64 tensor).  An absent row of a, and every row when no row of
    b is present: (0, -1, 0)."""
    best: torch.Tensor
    arg: torch.Tensor
    total: torch.Tensor
    present: torch.Tensor


class SmilesFingerprints:
    """Fingerprints of SMILES token rows over a target vocabulary, next to a SmilesKeys (self.keys: its randomiser,
    grammar, labels and words are this object's too, and gct_smiles_fp reads the keys' device tables).  ValueError for a
    vocabulary the randomiser rejects."""

    def __init__(self, itos, pad_id, eos_id, sep_id=None, keys=None):
        self.keys = ks = keys if keys is not None else SmilesKeys(itos, pad_id, eos_id, sep_id)
        self.randomizer, self.grammar = ks.randomizer, ks.grammar
        self.pad_id, self.eos_id, self.sep_id = ks.pad_id, ks.eos_id, ks.sep_id
        self.labels, self.words = ks.labels, ks.words

    def __len__(self):
        return len(self.grammar)

    # ------------------------------------------------------------------------------------------------ one part
    def identifiers(self, tokens, parsed):
        """[id_0, ..., id_R]: per generation the identifier of every atom of a parsed part, as unsigned ints."""
        apos, bonds, lists, _ = parsed
        A = len(apos)
        o = [self.keys.bond_label(tokens, apos, b) for b in bonds]
        near = [[(bonds[e][0] ^ bonds[e][1] ^ a, o[e]) for e in lists[a]] for a in range(A)]
        gen = [[mix(self.labels[tokens[apos[a]]] ^ mix(0x200 + len(near[a]))) for a in range(A)]]
        for _ in range(ops.FP_RADIUS):
            c = gen[-1]
            gen.append([mix(3 * c[a] + sum(mix(c[v] ^ mix(ob + 0x100)) for v, ob in near[a])) for a in range(A)])
        return gen

    def _part(self, tokens):
        """(status, the 16 words as unsigned ints, atoms, bonds)."""
        tokens = [int(t) for t in tokens]
        parsed = self.randomizer.parse(tokens)
        words = [0] * ops.FP_WORDS
        if parsed is None:
            return ops.FP_SYNTAX, words, 0, 0
        atoms, bonds = len(parsed[0]), len(parsed[1])
        if parsed[3]:
            return ops.FP_UNSUPPORTED, words, atoms, bonds
        for gen in self.identifiers(tokens, parsed):
            for x in gen:
                k = x % ops.FP_BITS
                words[k >> 6] |= 1 << (k & 63)
        return ops.FP_GRAPH, words, atoms, bonds

    def fingerprint(self, tokens):
        """THE statement for one part: tokens = its ids (no <eos>, no <sep>) -> (status, the 16 words), each word as the
        signed integer an int64 tensor holds.  The module docstring states the rule."""
        status, words, _, _ = self._part(tokens)
        return status, [as_int64(w) for w in words]

    # --------------------------------------------------------------------------------------------------- batches
    def fp_reference(self, ys, start):
        """THE batch rule (gct_smiles_fp implements it), on the CPU.  Spans, absent rows and the two parts are
        smiles.row_spans': an absent row has no bit and info (-1, 0, 0, 0).  Otherwise the molecule is fingerprinted; of
        `scaffold <sep> molecule` that is the part BEHIND the first <sep>, and the scaffold in front of it is not (a
        scaffold's fingerprint is fp_rows of the rows that murcko_scaffolds returns)."""
        spans = row_spans(ys, start, self.eos_id, self.sep_id)
        bits = torch.zeros(len(spans), ops.FP_WORDS, dtype=torch.int64)
        info = torch.zeros(len(spans), 4, dtype=torch.int32)
        for r, sp in enumerate(spans):
            if sp.molecule is None:
                info[r, 0] = -1
                continue
            status, words, atoms, nbonds = self._part(sp.molecule)
            bits[r] = torch.tensor([as_int64(w) for w in words])
            info[r] = torch.tensor([status, sum(bin(w).count("1") for w in words), atoms, nbonds])
        return FpRows(bits, info)

    def fp_rows(self, ys, start):
        """The same on the device of ys: one gct_smiles_fp launch, no synchronisation.  ys integers [n, W]; start ints
        [n] (on the CPU: checked there, as key_rows does) or an int32 tensor on the device (taken as it is: a row
        outside the range has no fingerprint).  ValueError for a span wider than 256 columns or a start outside
        [0, W]."""
        ys, st = launch_rows(ys, start, "the fingerprints take")
        table, labels = self.keys.device_tables(ys.device)
        return FpRows(*ops.smiles_fp(ys, st, table, labels, self.pad_id, self.eos_id,
                                     -1 if self.sep_id is None else self.sep_id))


# ------------------------------------------------------------------------------------------------- Tanimoto
def _check_fps(name, fps):
    if not isinstance(fps, FpRows):
        raise ValueError(f"{name} must be an FpRows, got {type(fps).__name__}")
    b, i = fps.bits, fps.info
    if b.dtype != torch.int64 or b.dim() != 2 or b.shape[1] != ops.FP_WORDS:
        raise ValueError(f"{name}.bits must be int64 [n, {ops.FP_WORDS}], got {b.dtype} {list(b.shape)}")
    if i.dtype != torch.int32 or i.dim() != 2 or i.shape != (b.shape[0], 4):
        raise ValueError(f"{name}.info must be int32 [{b.shape[0]}, 4], got {i.dtype} {list(i.shape)}")
    return fps


def _check_p(p):
    if p not in (1, 2):
        raise ValueError(f"p must be 1 or 2, got {p}")
    return int(p)


def _big(bits):
    """Every row's 16 words as one Python int of 1024 bits."""
    out = []
    for row in bits.cpu().tolist():
        x = 0
        for w, v in enumerate(row):
            x |= (v & _M) << (64 * w)
        out.append(x)
    return out


def tanimoto_reference(a: FpRows, b: FpRows, p=1, counts=None) -> TanimotoAgg:
    """THE statement of the aggregates, on the CPU in Python integers: for every row i of a, over the rows j of b in
    ascending order that are present (count != 0), c = popcount(a_i & b_j), u = |a_i| + |b_j| - c; T = c / u rounded
    once to fp32 (numpy's float32 division); total += T (p = 1) or float(T) * float(T) (p = 2: exact in fp64), in that
    order; the best pair is replaced when c * u_best > c_best * u (so the lowest j keeps a tie).  counts = (cnt_a, cnt_b)
    replaces info[:, 1] of the two sides (what internal_diversity masks rows with)."""
    _check_fps("a", a), _check_fps("b", b)
    p = _check_p(p)
    ca, cb = (a.info[:, 1], b.info[:, 1]) if counts is None else counts
    ca, cb = [int(x) for x in ca.cpu().tolist()], [int(x) for x in cb.cpu().tolist()]
    xa, xb = _big(a.bits), _big(b.bits)
    f32 = np.float32
    best, arg, total = [], [], []
    for i, x in enumerate(xa):
        bc, bu, bj, t = -1, 1, -1, 0.0
        if ca[i]:
            for j, y in enumerate(xb):
                if not cb[j]:
                    continue
                c = bin(x & y).count("1")
                u = ca[i] + cb[j] - c
                q = float(f32(c) / f32(u))
                t += q * q if p == 2 else q
                if c * bu > bc * u:
                    bc, bu, bj = c, u, j
        none = bj < 0
        best.append(0.0 if none else float(f32(bc) / f32(bu)))
        arg.append(bj)
        total.append(0.0 if none else t)
    return TanimotoAgg(torch.tensor(best, dtype=torch.float32), torch.tensor(arg, dtype=torch.int32),
                       torch.tensor(total, dtype=torch.float64), torch.tensor(sum(1 for c in cb if c), dtype=torch.int64))


def tanimoto_agg(a: FpRows, b: FpRows, p=1, counts=None) -> TanimotoAgg:
    """The same on the device of a (b is taken there): gct_fp_tanimoto, no synchronisation.  counts as in
    tanimoto_reference (int32 tensors)."""
    _check_fps("a", a), _check_fps("b", b)
    p = _check_p(p)
    dev = a.bits.device
    ca, cb = (a.info[:, 1], b.info[:, 1]) if counts is None else counts
    ca, cb = ca.to(dev).contiguous(), cb.to(dev).contiguous()
    best, arg, total = ops.fp_tanimoto(a.bits, ca, b.bits.to(dev), cb, p)
    return TanimotoAgg(best, arg, total, (cb != 0).sum())


def _agg(a, b, p=1, counts=None):
    """tanimoto_agg for rows on a GPU, tanimoto_reference otherwise."""
    return (tanimoto_agg if a.bits.is_cuda else tanimoto_reference)(a, b, p, counts)


def _present(fps, valid=None):
    keep = fps.info[:, 1] > 0
    if valid is not None:
        keep = keep & row_mask("valid", valid, keep.numel(), keep.device)
    return keep


def _diversity_terms(fps, valid, p):
    """fp64 [2] on the rows' device: (sum over the kept rows i of (total_i / N)^(1/p), N), N the kept rows."""
    keep = _present(_check_fps("fps", fps), valid)
    cnt = torch.where(keep, fps.info[:, 1], torch.zeros_like(fps.info[:, 1]))
    agg = _agg(fps, fps, _check_p(p), (cnt, cnt))
    N = keep.sum().to(torch.float64)
    per_row = agg.total.to(keep.device) / N.clamp(min=1.0)
    if p == 2:
        per_row = per_row.sqrt()
    return torch.stack([torch.where(keep, per_row, torch.zeros_like(per_row)).sum(), N])


def internal_diversity(fps: FpRows, valid=None, p=1) -> float:
    """moses' internal diversity of a set: 1 - mean_i((sum_j T(i, j)^p / N)^(1/p)) over the N rows that have a
    fingerprint (and, with valid bool [n], are valid).  Self pairs and duplicates are counted, as moses counts them: k
    copies of one molecule give 0, two disjoint molecules in equal shares 0.5.  0.0 for an empty set.  The aggregate is
    one gct_fp_tanimoto call for rows on a GPU (tanimoto_reference otherwise), the reduction from `total` runs in fp64
    torch on the rows' device; one read-back."""
    s, N = _diversity_terms(fps, valid, p).tolist()
    return 1.0 - s / N if N else 0.0


def _reference_rows(ref, device):
    """The FpRows of a reference set on `device`: an index's (copied there once), or the FpRows given."""
    if isinstance(ref, FingerprintIndex):
        return ref.rows_on(device)
    _check_fps("ref", ref)
    return FpRows(ref.bits.to(device), ref.info.to(device))


def snn(gen: FpRows, ref) -> float:
    """Similarity to the nearest neighbour (the reference's get_snn_from_mol): mean over the rows of gen that have a
    fingerprint of max_j T against ref (a FingerprintIndex or an FpRows), the fp32 maxima averaged in fp64.  0.0 if
    either side is empty.  One read-back."""
    _check_fps("gen", gen)
    agg = _agg(gen, _reference_rows(ref, gen.bits.device))
    keep = (gen.info[:, 1] > 0) & (agg.arg.to(gen.info.device) >= 0)
    best = agg.best.to(keep.device).to(torch.float64)
    s, k = torch.stack([torch.where(keep, best, torch.zeros_like(best)).sum(), keep.sum().to(torch.float64)]).tolist()
    return s / k if k else 0.0


class FingerprintIndex:
    """The fingerprints of a reference set -- a training set's molecules: self.bits int64 [m, 16], self.counts int32 [m]
    (their numbers of set bits), and the (ops.FP_BITS, ops.FP_RADIUS) they were made with (self.shape).  Only rows that
    have a fingerprint are kept; duplicates stay (SNN and a reward do not care, and `nearest` then indexes the rows
    that were put in)."""

    def __init__(self, bits, counts, shape=(ops.FP_BITS, ops.FP_RADIUS)):
        bits, counts = torch.as_tensor(bits), torch.as_tensor(counts)
        if bits.dtype != torch.int64 or bits.dim() != 2 or bits.shape[1] != ops.FP_WORDS:
            raise ValueError(f"an index holds int64 [m, {ops.FP_WORDS}] words, got {bits.dtype} {list(bits.shape)}")
        if counts.dtype != torch.int32 or counts.shape != (bits.shape[0],):
            raise ValueError(f"an index holds int32 [{bits.shape[0]}] counts, got {counts.dtype} {list(counts.shape)}")
        self.bits, self.counts = bits.contiguous(), counts.contiguous()
        self.shape = (int(shape[0]), int(shape[1]))
        self._on = {}

    def __len__(self):
        return self.bits.shape[0]

    @staticmethod
    def _kept(got):
        keep = (got.info[:, 0] == ops.FP_GRAPH) & (got.info[:, 1] > 0)
        return got.bits[keep], got.info[:, 1][keep]

    @classmethod
    def _of(cls, chunks):
        if not chunks:
            return cls(torch.zeros(0, ops.FP_WORDS, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
        dev = chunks[0][0].device
        return cls(torch.cat([b.to(dev) for b, _ in chunks]), torch.cat([c.to(dev) for _, c in chunks]))

    @classmethod
    def from_rows(cls, fps_obj, batches):
        """From an iterable of (ys, start) batches through fps_obj (a SmilesFingerprints): fp_rows for rows on a GPU,
        fp_reference otherwise.  Rows enter in order; rows without a fingerprint are left out."""
        chunks = []
        for ys, start in batches:
            ys = torch.as_tensor(ys)
            chunks.append(cls._kept(fps_obj.fp_rows(ys, start) if ys.is_cuda else fps_obj.fp_reference(ys, start)))
        return cls._of(chunks)

    @classmethod
    def from_smiles(cls, sampler, iterable, chunk=65536):
        """From SMILES strings, `chunk` at a time through sampler.fingerprints (one launch per chunk)."""
        return cls._of([cls._kept(sampler.fingerprints(batch)) for batch in chunked(iterable, chunk)])

    def save(self, path):
        torch.save({"bits": self.bits.cpu(), "counts": self.counts.cpu(), "fp_bits": self.shape[0],
                    "fp_radius": self.shape[1]}, path)

    @classmethod
    def load(cls, path, device=None):
        """ValueError for an index made with another width or radius: its bits compare with nothing made here."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        shape = (int(blob["fp_bits"]), int(blob["fp_radius"]))
        if shape != (ops.FP_BITS, ops.FP_RADIUS):
            raise ValueError(f"{path} holds fingerprints of {shape[0]} bits at radius {shape[1]}, this build makes "
                             f"{ops.FP_BITS} at radius {ops.FP_RADIUS}: build the index again")
        bits, counts = blob["bits"], blob["counts"]
        return cls(bits if device is None else bits.to(device), counts if device is None else counts.to(device), shape)

    def rows_on(self, device):
        """The index as an FpRows on `device` (copied once): info = (FP_GRAPH, count, 0, 0)."""
        def make():
            info = torch.zeros(len(self), 4, dtype=torch.int32, device=device)
            info[:, 1] = self.counts.to(device)
            return FpRows(self.bits.to(device), info)

        return on_device(self._on, device, make)

    def nearest(self, fps: FpRows, chunk=1 << 20):
        """(best fp32 [n], arg int32 [n]) of the rows of fps against the index, on their device: the largest T and the
        lowest index row that attains it, (0, -1) for a row without a fingerprint or an empty index.  The index is
        walked `chunk` rows at a time, which bounds the split workspace of a call.  Chunks combine exactly: two distinct
        quotients c / u with c, u <= 1024 differ by at least 2^-20, more than an fp32 ulp below 1, and rounding is
        monotonic, so comparing the chunks' fp32 maxima orders them as cross-multiplication would; a later chunk only
        takes a row over with a strictly larger maximum, so the lowest global j wins."""
        _check_fps("fps", fps)
        if int(chunk) < 1:
            raise ValueError(f"chunk must be at least 1, got {chunk}")
        dev = fps.bits.device
        mine = self.rows_on(dev)
        n = fps.bits.shape[0]
        best = torch.zeros(n, dtype=torch.float32, device=dev)
        arg = torch.full((n,), -1, dtype=torch.int32, device=dev)
        for lo in range(0, len(self), int(chunk)):
            got = _agg(fps, FpRows(mine.bits[lo:lo + int(chunk)], mine.info[lo:lo + int(chunk)]))
            take = (got.arg >= 0) & ((arg < 0) | (got.best > best))
            best = torch.where(take, got.best, best)
            arg = torch.where(take, got.arg + lo, arg)
        return best, arg
