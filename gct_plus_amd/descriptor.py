"""Molecular descriptors (what the reference's Utils/properties.py property_fn takes from rdkit for MW, HAC, HBA, HBD,
RBN, AIRN, ARRN and tPSA, and Inference/metrics.py get_errors on top of them, without rdkit): integer descriptors of the
labelled graph that randomize.SmilesRandomizer.parse reads from a token row, with ring perception -- which bonds lie on a
ring, the smallest ring through a bond, how many rings there are and how many of them are aromatic.

SmilesDescriptors.describe is THE statement for one part, desc_reference the batch rule; gct_smiles_desc
(csrc/descriptor.hip, csrc/smiles_desc.h, SmilesDescriptors.desc_rows) implements them and is compared with them exactly:
every output is an integer.

The rule.
  Atom entries come from the token STRING (atom_entry; desc32 is the per-token table the kernel reads, its bit layout is
  documented in include/gctplus_hip.h).  Element: B C N O F Si P S Cl Br I, masses in mDa 10810, 12011, 14007, 15999,
  18998, 28086, 30974, 32060, 35450, 79904, 126904; H 1008.  Any other element, `*`, an element H atom, a stated isotope, a
  bracket smiles._CHEM_BRACKET does not read, or a charge outside -3 .. 3 is UNKNOWN: one such atom makes the part
  DESC_UNKNOWN_ATOM.  Formal charge: as the bracket states it, 0 for a bare atom.  Stated hydrogens: a bracket atom has
  exactly what it states (H alone: 1), a bare atom has 0 stated plus its implicit hydrogens.  Aromatic: a lower-case symbol.
  Ring perception.  Bond e = (a, b) is a ring bond iff b is reachable from a without e; s(e) = 1 + the length of the
  shortest such path is the smallest ring through e; an atom is in a 3-ring iff one of its bonds has s = 3.
  Bond classes.  A written - or ~ is SINGLE, = DOUBLE, # TRIPLE, $ QUAD, : AROMATIC; without a symbol SINGLE, except
  between two aromatic atoms WHEN THE BOND IS A RING BOND, where it is AROMATIC (the linker of c1ccccc1c1ccccc1 is single;
  this is deliberately not molkey's bond label, which has no ring perception).  sigma(a) is the sum of the orders of a's
  bonds, AROMATIC counting 1.
  Implicit hydrogens of a bare atom.  Normal valences B {3}, C {4}, N {3, 5}, O {2}, P {3, 5}, S {2, 4, 6}, F Cl Br I {1};
  v0 is the smallest one >= sigma, h = 0 if there is none; otherwise h = v0 - sigma, for an aromatic atom
  max(0, v0 - sigma - 1).
  heavy_atoms = atoms; hydrogens = sum of h; mw_mda = sum of masses + 1008 hydrogens; charge = sum of charges;
  hbd = N or O atoms with h >= 1; hba = N and O atoms (Lipinski's counts); rings = bonds - atoms + 1;
  ring_bonds = bonds with s(e) > 0.
  rotatable = bonds of class SINGLE that are not ring bonds, both ends of degree >= 2, neither end with a TRIPLE bond.
  aromatic_rings: R = the AROMATIC ring bonds; |R| - (atoms touched by R) + (connected components of the subgraph R).
  tpsa_centi = sum over N and O atoms of Ertl's contribution in 0.01 A^2, TPSA_LINES below: n = degree, h = hydrogens,
  sg / db / tr / ar = the atom's SINGLE / DOUBLE / TRIPLE / AROMATIC bond counts (which must account for all n bonds),
  q = charge, r3 = in a 3-ring; the first matching line wins; without one N gets max(0, 3050 - 820 n + 150 h) and O
  max(0, 2850 - 860 n + 150 h).

Limits, on purpose.  No aromaticity perception: a Kekule spelling gets Kekule contributions and 0 aromatic rings.  No
stereo or dotted rows (DESC_UNSUPPORTED, the randomiser's set).  Lipinski's NO / NHOH counts, not rdkit's CalcNumHBA /
CalcNumHBD patterns.  Our own rotatable-bond rule, not rdkit's strict pattern: an amide C-N counts.  TPSA without S and P
(rdkit's default).  Average masses rounded to 1 mDa.  No logP (Wildman-Crippen's 72 SMARTS atom types), no QED (it needs
logP and a structural-alert list), no SAS, no NP: those tables cannot be restated here without the library, and a table
written from memory would be wrong silently.  The figures compare between runs of this code and with targets computed by
this code; they track rdkit's for ordinary MOSES-like molecules but are not promised to equal them."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from .molkey import SmilesKeys
from .smiles import _CHEM_BRACKET, launch_rows, on_device, row_mask, row_spans

ELEMENTS = ("B", "C", "N", "O", "F", "Si", "P", "S", "Cl", "Br", "I")
MASS_MDA = (10810, 12011, 14007, 15999, 18998, 28086, 30974, 32060, 35450, 79904, 126904)
H_MDA = 1008
VALENCES = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "P": (3, 5), "S": (2, 4, 6), "F": (1,), "Cl": (1,), "Br": (1,),
            "I": (1,)}
SINGLE, DOUBLE, TRIPLE, QUAD, AROMATIC = 1, 2, 3, 4, 5      # bond classes; a class's order is itself, AROMATIC's is 1
_WRITTEN = {1: SINGLE, 2: DOUBLE, 3: TRIPLE, 4: QUAD, 5: AROMATIC, 6: SINGLE}   # molkey.BOND_LABELS -> class
COLUMNS = ("status", "heavy_atoms", "hydrogens", "mw_mda", "charge", "hbd", "hba", "rotatable", "rings",
           "aromatic_rings", "tpsa_centi", "ring_bonds")
# (element, n, h, sg, db, tr, ar, q, needs a 3-ring, contribution): the first matching line wins
TPSA_LINES = (
    ("N", 1, 0, 0, 0, 1, 0, 0, False, 2379), ("N", 1, 1, 0, 1, 0, 0, 0, False, 2385), ("N", 1, 2, 1, 0, 0, 0, 0, False, 2602),
    ("N", 1, 2, 0, 1, 0, 0, 1, False, 2559), ("N", 1, 3, 1, 0, 0, 0, 1, False, 2764),
    ("N", 2, 0, 1, 1, 0, 0, 0, False, 1236), ("N", 2, 0, 0, 1, 1, 0, 0, False, 1360), ("N", 2, 1, 2, 0, 0, 0, 0, True, 2194),
    ("N", 2, 1, 2, 0, 0, 0, 0, False, 1203), ("N", 2, 0, 1, 0, 1, 0, 1, False, 436), ("N", 2, 1, 1, 1, 0, 0, 1, False, 1397),
    ("N", 2, 2, 2, 0, 0, 0, 1, False, 1661), ("N", 2, 0, 0, 0, 0, 2, 0, False, 1289), ("N", 2, 1, 0, 0, 0, 2, 0, False, 1579),
    ("N", 2, 1, 0, 0, 0, 2, 1, False, 1414),
    ("N", 3, 0, 3, 0, 0, 0, 0, True, 301), ("N", 3, 0, 3, 0, 0, 0, 0, False, 324), ("N", 3, 0, 1, 2, 0, 0, 0, False, 1168),
    ("N", 3, 0, 2, 1, 0, 0, 1, False, 301), ("N", 3, 1, 3, 0, 0, 0, 1, False, 444), ("N", 3, 0, 0, 0, 0, 3, 0, False, 441),
    ("N", 3, 0, 1, 0, 0, 2, 0, False, 493), ("N", 3, 0, 0, 1, 0, 2, 0, False, 410), ("N", 3, 0, 0, 0, 0, 3, 1, False, 410),
    ("N", 3, 0, 1, 0, 0, 2, 1, False, 388),
    ("N", 4, 0, 4, 0, 0, 0, 1, False, 0),
    ("O", 1, 0, 0, 1, 0, 0, 0, False, 1707), ("O", 1, 1, 1, 0, 0, 0, 0, False, 2023), ("O", 1, 0, 1, 0, 0, 0, -1, False, 2306),
    ("O", 2, 0, 2, 0, 0, 0, 0, True, 1253), ("O", 2, 0, 2, 0, 0, 0, 0, False, 923), ("O", 2, 0, 0, 0, 0, 2, 0, False, 1314))


def atom_entry(token):
    """(element index into ELEMENTS or None for UNKNOWN, charge, stated hydrogens, aromatic, bracket) of an ATOM token's
    string, as the module docstring reads it."""
    t = str(token)
    if t.startswith("["):
        m = _CHEM_BRACKET.fullmatch(t)
        if not m:
            return None, 0, 0, False, True
        iso, sym, h, ch = m.group(1), m.group(2), m.group(4), m.group(5)
        q = 0 if not ch else (int(ch) if len(ch) > 1 and ch[1:].isdigit() else (len(ch) if ch[0] == "+" else -len(ch)))
        stated = 0 if not h else int(h[1:] or 1)
        aromatic, el = sym[0].islower(), sym[0].upper() + sym[1:]
        known = iso is None and el in ELEMENTS and -3 <= q <= 3
        return (ELEMENTS.index(el), q, stated, aromatic, True) if known else (None, 0, 0, False, True)
    el = t[:1].upper() + t[1:]
    if el not in ELEMENTS:
        return None, 0, 0, False, False
    return ELEMENTS.index(el), 0, 0, t[0].islower(), False


def desc_word(token):
    """The desc32 word of an ATOM token's string (include/gctplus_hip.h documents the layout): element index + 1 (0:
    UNKNOWN) | aromatic << 4 | bracket << 5 | stated hydrogens << 6 (4 bits) | (charge + 3) << 10 (3 bits)."""
    el, q, h, aromatic, bracket = atom_entry(token)
    if el is None:
        return int(bracket) << 5
    return (el + 1) | (int(aromatic) << 4) | (int(bracket) << 5) | (h << 6) | ((q + 3) << 10)


def tpsa_line(el, n, h, sg, db, tr, ar, q, r3):
    """The index of the first line of TPSA_LINES that matches, or None."""
    for k, line in enumerate(TPSA_LINES):
        if line[:8] == (el, n, h, sg, db, tr, ar, q) and (r3 or not line[8]):
            return k
    return None


def tpsa_contribution(el, n, h, sg, db, tr, ar, q, r3):
    """Ertl's contribution of one N or O atom in 0.01 A^2: the first matching line of TPSA_LINES, else the fallback."""
    k = tpsa_line(el, n, h, sg, db, tr, ar, q, r3)
    if k is not None:
        return TPSA_LINES[k][9]
    return max(0, 3050 - 820 * n + 150 * h) if el == "N" else max(0, 2850 - 860 * n + 150 * h)


class DescRows(NamedTuple):
    """What desc_rows / desc_reference return: values int32 [n, 12], the columns of COLUMNS (ops.DESC_* index them).
    status: DESC_OK 0, DESC_SYNTAX 1, DESC_UNSUPPORTED 2, DESC_UNKNOWN_ATOM 3, -1 for a span without <eos>, wider than 256
    or with a start outside [0, W].  Where status is not DESC_OK, columns 3 .. 11 are 0, hydrogens is 0, and heavy_atoms
    is the number of atoms where a graph was parsed (UNSUPPORTED, UNKNOWN_ATOM), else 0."""
    values: torch.Tensor

    status = property(lambda self: self.values[:, ops.DESC_STATUS])
    heavy_atoms = property(lambda self: self.values[:, ops.DESC_HEAVY_ATOMS])
    hydrogens = property(lambda self: self.values[:, ops.DESC_HYDROGENS])
    mw_mda = property(lambda self: self.values[:, ops.DESC_MW_MDA])
    charge = property(lambda self: self.values[:, ops.DESC_CHARGE])
    hbd = property(lambda self: self.values[:, ops.DESC_HBD])
    hba = property(lambda self: self.values[:, ops.DESC_HBA])
    rotatable = property(lambda self: self.values[:, ops.DESC_ROTATABLE])
    rings = property(lambda self: self.values[:, ops.DESC_RINGS])
    aromatic_rings = property(lambda self: self.values[:, ops.DESC_AROMATIC_RINGS])
    tpsa_centi = property(lambda self: self.values[:, ops.DESC_TPSA_CENTI])
    ring_bonds = property(lambda self: self.values[:, ops.DESC_RING_BONDS])

    @property
    def ok(self):
        """bool [n]: status == DESC_OK."""
        return self.values[:, ops.DESC_STATUS] == ops.DESC_OK

    @property
    def mw(self):
        """Molecular weight in dalton, fp32 [n] on the rows' device: the integer divided once."""
        return self.column("mw")

    @property
    def tpsa(self):
        """Polar surface area in A^2, fp32 [n] on the rows' device: the integer divided once."""
        return self.column("tpsa")

    @property
    def aliphatic_rings(self):
        return self.values[:, ops.DESC_RINGS] - self.values[:, ops.DESC_AROMATIC_RINGS]

    def column(self, name, dtype=torch.float32):
        """`dtype` [n] on the rows' device: `mw`, `tpsa`, `aliphatic_rings` or a name of COLUMNS.  mw and tpsa are the
        integer divided once in fp64 -- a correctly rounded division on every device, so the figures of a GPU and of the
        host agree to the bit -- and rounded once to `dtype`.  (The integers themselves are self.values: mw_mda can
        exceed what fp32 holds exactly.)"""
        if name == "mw":
            return (self.values[:, ops.DESC_MW_MDA].to(torch.float64) / 1000.0).to(dtype)
        if name == "tpsa":
            return (self.values[:, ops.DESC_TPSA_CENTI].to(torch.float64) / 100.0).to(dtype)
        if name == "aliphatic_rings":
            return self.aliphatic_rings.to(dtype)
        if name not in COLUMNS:
            raise ValueError(f"no descriptor column `{name}`: mw, tpsa, aliphatic_rings or one of {', '.join(COLUMNS)}")
        return self.values[:, COLUMNS.index(name)].to(dtype)

    def columns(self, names):
        """fp32 [n, len(names)]: `column` of every name, gathered."""
        names = list(names)
        if not names:
            return torch.zeros(self.values.shape[0], 0, dtype=torch.float32, device=self.values.device)
        return torch.stack([self.column(k) for k in names], 1)


class SmilesDescriptors:
    """Descriptors of SMILES token rows over a target vocabulary, next to a SmilesKeys (self.keys: its randomiser,
    grammar and device tables are this object's too).  self.desc: the desc32 word of every token (desc_word for an ATOM
    token, 0 otherwise).  ValueError for a vocabulary the randomiser rejects."""

    def __init__(self, itos, pad_id, eos_id, sep_id=None, keys=None):
        self.keys = ks = keys if keys is not None else SmilesKeys(itos, pad_id, eos_id, sep_id)
        self.randomizer, self.grammar = ks.randomizer, ks.grammar
        self.pad_id, self.eos_id, self.sep_id = ks.pad_id, ks.eos_id, ks.sep_id
        g = self.grammar
        self.entries = [atom_entry(t) if c == ops.GRAMMAR_ATOM else None for t, c in zip(g.itos, g.classes)]
        self.desc = [desc_word(t) if c == ops.GRAMMAR_ATOM else 0 for t, c in zip(g.itos, g.classes)]
        self.desc_table = torch.tensor(self.desc, dtype=torch.int32)
        self._device_tables = {}

    def __len__(self):
        return len(self.grammar)

    def device_tables(self, device):
        """(table32 int32 [V] -- the keys' --, desc32 int32 [V]) on `device` (copied once)."""
        return on_device(self._device_tables, device,
                         lambda: (self.keys.device_tables(device)[0], self.desc_table.to(device)))

    # ------------------------------------------------------------------------------------------------ one part
    @staticmethod
    def ring_sizes(A, bonds, lists):
        """s(e) of every bond, 0 for a bond that lies on no ring: a breadth-first search from one end with the bond
        excluded, stopped at the other end."""
        out = []
        for e, (a, b, _) in enumerate(bonds):
            seen, frontier, dist, size = {a}, [a], 0, 0
            while frontier and not size:
                dist, nxt = dist + 1, []
                for u in frontier:
                    for x in lists[u]:
                        v = bonds[x][0] ^ bonds[x][1] ^ u
                        if x != e and v not in seen:
                            seen.add(v), nxt.append(v)
                if b in seen:
                    size = dist + 1
                frontier = nxt
            out.append(size)
        return out

    def bond_classes(self, tokens, apos, bonds, sizes):
        out = []
        for (a, b, sym), s in zip(bonds, sizes):
            if sym is not None:
                out.append(_WRITTEN[(self.keys.words[tokens[sym]] >> 21) & 7])
            else:
                both = self.entries[tokens[apos[a]]][3] and self.entries[tokens[apos[b]]][3]
                out.append(AROMATIC if both and s else SINGLE)
        return out

    def describe(self, tokens):
        """THE statement for one part: tokens = its ids (no <eos>, no <sep>) -> the 12 integers of COLUMNS.  The module
        docstring states the rule."""
        tokens = [int(t) for t in tokens]
        parsed = self.randomizer.parse(tokens)
        if parsed is None:
            return [ops.DESC_SYNTAX] + [0] * 11
        apos, bonds, lists, unsupported = parsed
        A = len(apos)
        if unsupported:
            return [ops.DESC_UNSUPPORTED, A] + [0] * 10
        ent = [self.entries[tokens[p]] for p in apos]
        if any(x[0] is None for x in ent):
            return [ops.DESC_UNKNOWN_ATOM, A] + [0] * 10
        sizes = self.ring_sizes(A, bonds, lists)
        cls = self.bond_classes(tokens, apos, bonds, sizes)
        hs, triple = [], []
        mw = charge = hbd = hba = tpsa = 0
        for a, (el, q, stated, aromatic, bracket) in enumerate(ent):
            mine = [cls[e] for e in lists[a]]
            sigma = sum(1 if c == AROMATIC else c for c in mine)
            name = ELEMENTS[el]
            if bracket:
                h = stated
            else:
                v0 = min((v for v in VALENCES.get(name, ()) if v >= sigma), default=None)
                h = 0 if v0 is None else (max(0, v0 - sigma - 1) if aromatic else v0 - sigma)
            hs.append(h), triple.append(TRIPLE in mine)
            mw += MASS_MDA[el] + H_MDA * h
            charge += q
            if name in ("N", "O"):
                hba += 1
                hbd += h >= 1
                r3 = any(sizes[e] == 3 for e in lists[a])
                tpsa += tpsa_contribution(name, len(mine), h, mine.count(SINGLE), mine.count(DOUBLE), mine.count(TRIPLE),
                                          mine.count(AROMATIC), q, r3)
        rot = sum(1 for (a, b, _), c, s in zip(bonds, cls, sizes)
                  if c == SINGLE and not s and len(lists[a]) >= 2 and len(lists[b]) >= 2 and not triple[a] and not triple[b])
        R = [e for e in range(len(bonds)) if cls[e] == AROMATIC and sizes[e]]
        touched = {x for e in R for x in bonds[e][:2]}
        rep = {}                                                 # atom -> the lowest atom reached over the bonds of R
        for a in sorted(touched):
            seen, todo = {a}, [a]
            while todo:
                u = todo.pop()
                for e in lists[u]:
                    v = bonds[e][0] ^ bonds[e][1] ^ u
                    if cls[e] == AROMATIC and sizes[e] and v not in seen:
                        seen.add(v), todo.append(v)
            rep[a] = min(seen)
        comps = sum(1 for a in touched if rep[a] == a)
        return [ops.DESC_OK, A, sum(hs), mw, charge, hbd, hba, rot, len(bonds) - A + 1, len(R) - len(touched) + comps,
                tpsa, sum(1 for s in sizes if s)]

    # --------------------------------------------------------------------------------------------------- batches
    def desc_reference(self, ys, start) -> DescRows:
        """THE batch rule (gct_smiles_desc implements it), on the CPU.  Spans, absent rows and the two parts are
        smiles.row_spans': an absent row is (-1, 0, ..., 0).  Otherwise the molecule is described; of `scaffold <sep>
        molecule` that is the part BEHIND the first <sep>."""
        spans = row_spans(ys, start, self.eos_id, self.sep_id)
        out = torch.zeros(len(spans), ops.DESC_COLUMNS, dtype=torch.int32)
        for r, sp in enumerate(spans):
            if sp.molecule is None:
                out[r, 0] = -1
            else:
                out[r] = torch.tensor(self.describe(sp.molecule), dtype=torch.int32)
        return DescRows(out)

    def desc_rows(self, ys, start) -> DescRows:
        """The same on the device of ys: one gct_smiles_desc launch, no synchronisation.  ys integers [n, W]; start ints
        [n] (on the CPU: checked there, as key_rows does) or an int32 tensor on the device (taken as it is: a row
        outside the range has status -1).  ValueError for a span wider than 256 columns or a start outside [0, W]."""
        ys, st = launch_rows(ys, start, "the descriptors take")
        table, desc = self.device_tables(ys.device)
        return DescRows(ops.smiles_desc(ys, st, table, desc, self.pad_id, self.eos_id,
                                        -1 if self.sep_id is None else self.sep_id))


# ------------------------------------------------------------------------------------- what the descriptors are for
ERROR_KEYS = ("mae", "mse", "max", "min", "aard", "amsd")


def _error_terms(value, target, keep):
    """fp64 [7] on value's device: the six sums / extremes of get_errors over the kept rows, and their number."""
    v = value.to(torch.float64)
    t = torch.as_tensor(target).to(v.device).to(torch.float64)
    t = t.expand_as(v) if t.dim() == 0 else t.reshape(-1)
    if t.shape != v.shape:
        raise ValueError(f"{t.numel()} targets for {v.numel()} rows")
    if v.numel() == 0:
        return torch.zeros(7, dtype=torch.float64, device=v.device)
    d = t - v
    rel = d / t
    zero, inf = torch.zeros_like(d), torch.full_like(d, float("inf"))
    n = keep.sum().to(torch.float64)
    k, none = n.clamp(min=1.0), n == 0
    mean = lambda x: torch.where(keep, x, zero).sum() / k
    return torch.stack([mean(d.abs()), mean(d), torch.where(none, zero[0], torch.where(keep, d, -inf).max()),
                        torch.where(none, zero[0], torch.where(keep, d, inf).min()), mean(rel.abs()), mean(rel), n])


def _mask(mask, n, device):
    if mask is None:
        return torch.ones(n, dtype=torch.bool, device=device)
    return row_mask("mask", mask, n, device)


def property_errors(values, targets, mask=None):
    """The reference's get_errors, with its key names and its formulas as written: d = target - value over the counted
    rows; mae = mean |d|; mse = mean d (sic); max; min; aard = mean |d / target|; amsd = mean (d / target) (a zero
    target gives what the division gives); and n, the rows counted.  No rows: zeros.  fp64 on the values' device, one
    read-back.
      values a vector [n] (a DescRows column or float view) and targets a vector [n] or a number: one dict, over the
      rows in mask (bool [n]; None: all).
      values a DescRows and targets a dict name -> vector or number (names as DescRows.column takes them): a dict
      name -> errors, over the rows that are DESC_OK and in mask."""
    if isinstance(values, DescRows):
        if not isinstance(targets, dict):
            raise ValueError("property_errors: a DescRows goes with targets = {column name: target}")
        keep = values.ok & _mask(mask, values.values.shape[0], values.values.device)
        names = list(targets)
        if not names:
            return {}
        got = torch.stack([_error_terms(values.column(k, torch.float64), targets[k], keep) for k in names]).tolist()
        return {k: dict(zip(ERROR_KEYS, row[:6]), n=int(row[6])) for k, row in zip(names, got)}
    values = torch.as_tensor(values)
    if values.dim() != 1:
        raise ValueError(f"property_errors: values must be a vector [n] or a DescRows, got {list(values.shape)}")
    row = _error_terms(values, targets, _mask(mask, values.numel(), values.device)).tolist()
    return dict(zip(ERROR_KEYS, row[:6]), n=int(row[6]))
