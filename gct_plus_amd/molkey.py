"""Molecule identity keys (what the reference's Inference/metrics.py get_basic_metrics takes from moses and rdkit for
`unique` and `novel`, without either): a spelling-independent 64-bit key of the labelled graph that
randomize.SmilesRandomizer.parse reads from a token row, and what a batch of such keys is for -- a per-row "first of its
kind" mask, a sorted index of training-set keys, the valid / unique / novel figures and, over the keys of scaffold.py's
Murcko scaffolds, scaffold fidelity (scaffold_metrics).

SmilesKeys.key is THE statement for one part, key_reference the batch rule; gct_smiles_key (csrc/molkey.hip,
SmilesKeys.key_rows) implements them and is compared with them bit for bit.

The rule.  All arithmetic is in uint64 and wraps; every combination over neighbours or atoms is a SUM, so no order can
leak in.  mix is splitmix64's finaliser.  L(a) is the FNV-1a 64-bit hash of the atom token's STRING (not its id: keys
compare across vocabularies).  o(e) is the bond's label: the written symbol's (- 1, = 2, # 3, $ 4, : 5, ~ 6), without a
symbol 5 between two aromatic atom tokens (smiles.chem_atom_entry) and 1 otherwise.
  1. distance profile: c_0(a) = mix(L(a) + sum over b reachable from a, a included, of mix(L(b) ^ mix(dist(a, b) + 1)))
  2. ops.KEY_ROUNDS rounds: c_{r+1}(a) = mix(3 c_r(a) + sum over bonds (b, o) of a of mix(c_r(b) ^ mix(o + 0x100)))
  3. key = mix(sum over a of mix(c_R(a)) + atoms * 0x9E3779B97F4A7C15 + bonds)
A part without a graph -- it does not parse (KEY_STRING_SYNTAX), or the randomiser's UNSUPPORTED set applies: a / or \\
bond, an @ atom, a dot, a RING_BOND closure, a ninth bond (KEY_STRING_UNSUPPORTED) -- gets an order-dependent hash of its
tokens' strings under another domain constant (string_key): two such parts are the same only if spelled the same.

Limits, on purpose.  Key equality is NECESSARY for identity, not proof of it: graphs that this refinement cannot
separate exist (the distance profile separates the drug-like pairs plain refinement merges, such as decalin and
bicyclopentyl; strongly regular graphs stay merged), and 64 bits collide by accident at about n^2 / 2^65.  Atom tokens
are compared verbatim: [CH3] differs from C, and a Kekule spelling differs from an aromatic one -- no aromaticity
perception, no kekulisation.  Stereo and dotted rows fall back to string identity.  No canonical SMILES string is made."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from .randomize import SmilesRandomizer
from .smiles import ChemReport, chem_atom_entry, chunked, launch_rows, on_device, row_mask, row_spans

_M = 0xFFFFFFFFFFFFFFFF
GOLD = 0x9E3779B97F4A7C15
STRING_DOMAIN = 0xA0761D6478BD642F                 # where a string key's chain starts (csrc/molkey.hip kStringDomain)
UNKNOWN_DOMAIN = 0xE7037ED1A0B428DB                # the label of an id outside the vocabulary: mix(id ^ this)
BOND_LABELS = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 5, "~": 6}


def mix(x):
    """splitmix64's finaliser on a Python int (taken mod 2^64)."""
    x &= _M
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def fnv1a64(text):
    """FNV-1a, 64 bits, over the UTF-8 bytes of a string."""
    h = 0xCBF29CE484222325
    for b in str(text).encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & _M
    return h


def as_int64(x):
    """The 64 bits of x as the signed integer an int64 tensor holds."""
    x &= _M
    return x - (1 << 64) if x >> 63 else x


def _lsr(x, k):
    return (x >> k) & ((1 << (64 - k)) - 1)


def mix_tensor(x):
    """mix on an int64 tensor, bit for bit (int64 multiplication wraps; the shifts are made logical)."""
    x = x ^ _lsr(x, 30)
    x = x * as_int64(0xBF58476D1CE4E5B9)
    x = x ^ _lsr(x, 27)
    x = x * as_int64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


class MolKeys(NamedTuple):
    """What key_rows / key_reference return.  key int64 [n, 2] = (the molecule's key, the scaffold's or 0); info int32
    [n, 4] = (status of the molecule part, status of the scaffold part or -1, atoms, bonds of the molecule part); a row
    without <eos> in its span has keys 0 and info (-1, -1, 0, 0)."""
    key: torch.Tensor
    info: torch.Tensor


class SmilesKeys:
    """Identity keys of SMILES token rows over a target vocabulary, next to a SmilesRandomizer (self.randomizer: its
    grammar, its parse and its UNSUPPORTED set).  self.labels: the FNV-1a hash of every token's string; self.words:
    gct_smiles_key's table32, the randomiser's word | from bit 21 the key's label of a BOND token or `aromatic` of an ATOM
    token.  randomizer: a SmilesRandomizer over the same vocabulary and ids to share instead of building one.  ValueError
    for a vocabulary the randomiser rejects."""

    def __init__(self, itos, pad_id, eos_id, sep_id=None, randomizer=None):
        self.randomizer = rz = randomizer if randomizer is not None else SmilesRandomizer(itos, pad_id, eos_id, sep_id)
        self.grammar = g = rz.grammar
        self.pad_id, self.eos_id, self.sep_id = rz.pad_id, rz.eos_id, rz.sep_id
        self.labels = [fnv1a64(t) for t in g.itos]
        self.words = []
        for t, c, w in zip(g.itos, g.classes, rz.words):
            if c == ops.GRAMMAR_BOND:
                w |= BOND_LABELS.get(t, 0) << 21           # (/ and \\ have none: their parts are UNSUPPORTED)
            elif c == ops.GRAMMAR_ATOM:
                w |= int(bool(chem_atom_entry(t)[2])) << 21
            self.words.append(w)
        self.table = torch.tensor(self.words, dtype=torch.int32)
        self.label_table = torch.tensor([as_int64(h) for h in self.labels], dtype=torch.int64)
        self._device_tables = {}

    def __len__(self):
        return len(self.grammar)

    def device_tables(self, device):
        """(table32 int32 [V], label64 int64 [V]) on `device` (copied once)."""
        return on_device(self._device_tables, device, lambda: (self.table.to(device), self.label_table.to(device)))

    # ------------------------------------------------------------------------------------------------ one part
    def label(self, t):
        """The 64-bit label of token id t: its string's hash, or mix(id ^ UNKNOWN_DOMAIN) outside the vocabulary."""
        t = int(t)
        return self.labels[t] if 0 <= t < len(self.labels) else mix((t & _M) ^ UNKNOWN_DOMAIN)

    def string_key(self, tokens):
        """The order-dependent key of a part without a graph: h = STRING_DOMAIN; per token h = mix((h + GOLD) ^ label);
        mix(h + number of tokens)."""
        h = STRING_DOMAIN
        for t in tokens:
            h = mix((h + GOLD) ^ self.label(t))
        return mix(h + len(tokens))

    def bond_label(self, tokens, apos, bond):
        a, b, sym = bond
        if sym is not None:
            return (self.words[tokens[sym]] >> 21) & 7
        return 5 if (self.words[tokens[apos[a]]] >> 21) & (self.words[tokens[apos[b]]] >> 21) & 1 else 1

    def colours(self, tokens, parsed):
        """c_R(a) of every atom of a parsed part (the per-atom values behind the key), as unsigned ints."""
        apos, bonds, lists, _ = parsed
        A = len(apos)
        L = [self.labels[tokens[p]] for p in apos]
        o = [self.bond_label(tokens, apos, b) for b in bonds]
        near = [[(bonds[e][0] ^ bonds[e][1] ^ a, o[e]) for e in lists[a]] for a in range(A)]
        c = []
        for a in range(A):
            seen, frontier, dist, total = {a}, [a], 0, 0
            while frontier:
                md = mix(dist + 1)
                total += sum(mix(L[b] ^ md) for b in frontier)
                nxt = []
                for b in frontier:
                    for v, _ in near[b]:
                        if v not in seen:
                            seen.add(v), nxt.append(v)
                frontier, dist = nxt, dist + 1
            c.append(mix(L[a] + total))
        for _ in range(ops.KEY_ROUNDS):
            c = [mix(3 * c[a] + sum(mix(c[v] ^ mix(ob + 0x100)) for v, ob in near[a])) for a in range(A)]
        return c

    def _part(self, tokens):
        tokens = [int(t) for t in tokens]
        parsed = self.randomizer.parse(tokens)
        if parsed is None:
            return ops.KEY_STRING_SYNTAX, self.string_key(tokens), 0, 0
        atoms, bonds = len(parsed[0]), len(parsed[1])
        if parsed[3]:
            return ops.KEY_STRING_UNSUPPORTED, self.string_key(tokens), atoms, bonds
        c = self.colours(tokens, parsed)
        return ops.KEY_GRAPH, mix(sum(mix(x) for x in c) + atoms * GOLD + bonds), atoms, bonds

    def key(self, tokens):
        """THE statement for one part: tokens = its ids (no <eos>, no <sep>) -> (status, key), the key as the signed
        integer an int64 tensor holds (as_int64 of the 64 bits).  The module docstring states the rule."""
        status, k, _, _ = self._part(tokens)
        return status, as_int64(k)

    # --------------------------------------------------------------------------------------------------- batches
    def key_reference(self, ys, start):
        """THE batch rule (gct_smiles_key implements it), on the CPU.  Spans, absent rows and the two parts are
        smiles.row_spans': an absent row (no <eos> in its span, a span wider than 256 columns, a start outside [0, W]) has
        keys 0 and info (-1, -1, 0, 0); otherwise the molecule and, where there is one, the scaffold go through `key`,
        each on its own."""
        spans = row_spans(ys, start, self.eos_id, self.sep_id)
        key = torch.zeros(len(spans), 2, dtype=torch.int64)
        info = torch.zeros(len(spans), 4, dtype=torch.int32)
        for r, sp in enumerate(spans):
            if sp.molecule is None:
                info[r, 0] = info[r, 1] = -1
                continue
            sca = None if sp.scaffold is None else self._part(sp.scaffold)
            mol = self._part(sp.molecule)
            key[r, 0] = as_int64(mol[1])
            key[r, 1] = as_int64(sca[1]) if sca else 0
            info[r] = torch.tensor([mol[0], sca[0] if sca else -1, mol[2], mol[3]])
        return MolKeys(key, info)

    def key_rows(self, ys, start):
        """The same on the device of ys: one gct_smiles_key launch, no synchronisation.  ys integers [n, W]; start ints
        [n] (on the CPU: checked there, as SmilesRandomizer.randomize_rows does) or an int32 tensor on the device (taken
        as it is: a row outside the range has no key).  ValueError for a span wider than 256 columns or a start outside
        [0, W]."""
        ys, st = launch_rows(ys, start, "the keys take")
        table, labels = self.device_tables(ys.device)
        return MolKeys(*ops.smiles_key(ys, st, table, labels, self.pad_id, self.eos_id,
                                       -1 if self.sep_id is None else self.sep_id))


# ------------------------------------------------------------------------------------------- what the keys are for
def _molecule_column(keys):
    """int64 [n] of a MolKeys, a key tensor [n, 2] (its molecule column) or a key vector [n]."""
    k = keys.key if isinstance(keys, MolKeys) else torch.as_tensor(keys)
    if k.dtype != torch.int64 or k.dim() not in (1, 2):
        raise ValueError(f"keys must be int64 [n] or [n, 2], got {k.dtype} {list(k.shape)}")
    return k[:, 0] if k.dim() == 2 else k


def first_occurrence(keys, group=None, valid=None):
    """bool [n] on the keys' device: True on the lowest-index row of each distinct key, by stable sort and scatter (no
    host loop, no synchronisation).  group ints [n]: per group, through mix(key ^ mix(group)) -- per-scaffold or
    per-condition uniqueness.  valid bool [n]: rows outside it are never first and do not count as an occurrence."""
    k = _molecule_column(keys)
    n = k.numel()
    if group is not None:
        group = torch.as_tensor(group).to(k.device)
        if group.dtype.is_floating_point or group.numel() != n:
            raise ValueError(f"group must be {n} integers, one per row, got {group.dtype} {list(group.shape)}")
        k = mix_tensor(k ^ mix_tensor(group.reshape(-1).to(torch.int64)))
    rows = torch.arange(n, device=k.device)
    if valid is not None:
        valid = row_mask("valid", valid, n, k.device)
        rows = torch.sort((~valid).to(torch.uint8), stable=True).indices      # the valid rows first, each side in row order
    ordered, order = torch.sort(k[rows], stable=True)
    rows = rows[order]
    first = torch.ones(n, dtype=torch.bool, device=k.device)
    first[1:] = ordered[1:] != ordered[:-1]
    if valid is not None:
        first &= valid[rows]                                 # (a run with a valid row starts with one)
    out = torch.zeros(n, dtype=torch.bool, device=k.device)
    out[rows] = first
    return out


class MolKeyIndex:
    """A sorted, de-duplicated int64 tensor of keys (self.keys) -- a training set's molecules -- and the rounds of
    refinement they were made with (self.rounds)."""

    def __init__(self, keys, rounds=ops.KEY_ROUNDS):
        keys = torch.as_tensor(keys)
        if keys.dtype != torch.int64:
            raise ValueError(f"an index holds int64 keys, got {keys.dtype}")
        self.keys = torch.unique(keys.reshape(-1))           # (sorted ascending as signed integers)
        self.rounds = int(rounds)
        self._on = {}

    def __len__(self):
        return self.keys.numel()

    @classmethod
    def from_rows(cls, keys_obj, batches, graph_only=True):
        """From an iterable of (ys, start) batches through keys_obj (a SmilesKeys): key_rows for rows on a GPU,
        key_reference otherwise; every batch is de-duplicated on its own, so the rows are never held together.  Only
        KEY_GRAPH molecule keys enter (graph_only=False: every row with a key)."""
        chunks = []
        for ys, start in batches:
            ys = torch.as_tensor(ys)
            got = keys_obj.key_rows(ys, start) if ys.is_cuda else keys_obj.key_reference(ys, start)
            keep = got.info[:, 0] == ops.KEY_GRAPH if graph_only else got.info[:, 0] >= 0
            chunks.append(torch.unique(got.key[:, 0][keep]))
        if not chunks:
            return cls(torch.zeros(0, dtype=torch.int64))
        return cls(torch.cat([c.to(chunks[0].device) for c in chunks]))

    @classmethod
    def from_smiles(cls, sampler, iterable, chunk=65536, graph_only=True):
        """From SMILES strings, `chunk` at a time through sampler.molecule_keys (one launch per chunk)."""
        chunks = []
        for batch in chunked(iterable, chunk):
            got = sampler.molecule_keys(batch)
            keep = got.info[:, 0] == ops.KEY_GRAPH if graph_only else got.info[:, 0] >= 0
            chunks.append(torch.unique(got.key[:, 0][keep]))
        if not chunks:
            return cls(torch.zeros(0, dtype=torch.int64))
        return cls(torch.cat(chunks))

    def save(self, path):
        torch.save({"keys": self.keys.cpu(), "rounds": self.rounds}, path)

    @classmethod
    def load(cls, path, device=None):
        """ValueError for an index made with another number of rounds: its keys compare with nothing made here."""
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if int(blob["rounds"]) != ops.KEY_ROUNDS:
            raise ValueError(f"{path} holds keys of {int(blob['rounds'])} rounds of refinement, this build makes "
                             f"{ops.KEY_ROUNDS}: build the index again")
        return cls(blob["keys"] if device is None else blob["keys"].to(device), blob["rounds"])

    def contains(self, keys):
        """bool [n] on the keys' device: the key is in the index (torch.searchsorted; the index is copied to a device
        once)."""
        k = _molecule_column(keys)
        mine = on_device(self._on, k.device, lambda: self.keys.to(k.device))
        if mine.numel() == 0:
            return torch.zeros(k.shape, dtype=torch.bool, device=k.device)
        at = torch.searchsorted(mine, k.contiguous()).clamp_(max=mine.numel() - 1)
        return mine[at] == k


def basic_metrics(report: ChemReport, keys, index=None, fps=None):
    """The reference's get_basic_metrics figures, with moses' definitions: valid = the share of rows whose ChemReport
    status is OK; unique = distinct keys among the valid rows / valid rows; novel (only with an index) = the share of
    those distinct keys that the index does not hold; 0 for an empty denominator.  Also the counts n, n_valid, n_unique
    (and n_novel).  Everything is computed on the keys' device; one read-back.  fps (a fingerprint.FpRows of the same
    rows) adds intDiv = fingerprint.internal_diversity over the valid rows and n_fp, the valid rows that have a
    fingerprint, with a read-back of their own; without it the dict is what it was before there were fingerprints."""
    k = _molecule_column(keys)
    ok = (report.status == ops.CHEM_OK).to(k.device)
    if ok.shape != k.shape:
        raise ValueError(f"{ok.numel()} report rows for {k.numel()} keys")
    if fps is not None and fps.bits.shape[0] != k.numel():
        raise ValueError(f"{fps.bits.shape[0]} fingerprints for {k.numel()} keys")
    first = first_occurrence(k, valid=ok)
    counts = [ok.sum(), first.sum()]
    if index is not None:
        counts.append((first & ~index.contains(k)).sum())
    counts = torch.stack(counts).tolist()
    n, n_valid, n_unique = k.numel(), counts[0], counts[1]
    out = {"valid": n_valid / n if n else 0.0, "unique": n_unique / n_valid if n_valid else 0.0}
    if index is not None:
        out["novel"] = counts[2] / n_unique if n_unique else 0.0
    out.update(n=n, n_valid=n_valid, n_unique=n_unique)
    if index is not None:
        out["n_novel"] = counts[2]
    if fps is not None:
        from .fingerprint import _diversity_terms
        s, n_fp = _diversity_terms(fps, ok.to(fps.bits.device), 1).tolist()
        out["intDiv"] = 1.0 - s / n_fp if n_fp else 0.0
        out["n_fp"] = int(n_fp)
    return out


def scaffold_metrics(report: ChemReport, sca, keys=None):
    """Scaffold fidelity of decoded `scaffold <sep> molecule` rows (what the reference's Plot/sampled_molecules.py reads
    off `df.scaffold == scaffold`): report a ChemReport, sca a scaffold.ScaffoldRows of the same rows
    (Sampling.scaffold_report).  same_scaffold = the valid rows whose molecule has the scaffold it was given
    (scaffold.scaffold_match) / valid rows; n_scaffolds = distinct extracted scaffold keys among the valid rows that have
    a scaffold; with keys (the rows' molecule keys) unique_on_scaffold = distinct (extracted scaffold, molecule) pairs
    among the valid rows / valid rows.  0 for an empty denominator.  Also n, n_valid, n_same.  Everything is computed on
    the rows' device; one read-back."""
    from .scaffold import scaffold_match
    k = sca.key[:, 0]
    ok = (report.status == ops.CHEM_OK).to(k.device)
    if ok.shape != k.shape:
        raise ValueError(f"{ok.numel()} report rows for {k.numel()} scaffold rows")
    counts = [ok.sum(), (scaffold_match(sca) & ok).sum(),
              first_occurrence(k, valid=ok & (sca.info[:, 0] == ops.SCA_OK)).sum()]
    if keys is not None:
        mol = _molecule_column(keys).to(k.device)
        if mol.shape != k.shape:
            raise ValueError(f"{mol.numel()} molecule keys for {k.numel()} scaffold rows")
        counts.append(first_occurrence(mol, group=k, valid=ok).sum())
    counts = torch.stack(counts).tolist()
    n, n_valid = k.numel(), counts[0]
    out = {"same_scaffold": counts[1] / n_valid if n_valid else 0.0, "n_scaffolds": counts[2]}
    if keys is not None:
        out["unique_on_scaffold"] = counts[3] / n_valid if n_valid else 0.0
    out.update(n=n, n_valid=n_valid, n_same=counts[1])
    return out
