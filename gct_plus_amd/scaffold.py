"""Murcko scaffolds (what the reference takes from rdkit's MurckoScaffoldSmiles in Utils/smiles.py murcko_scaffold, for
preprocess.py's src_scaffold / trg_scaffold columns and for Plot/sampled_molecules.py's `df.scaffold == scaffold`,
without rdkit): the ring systems of a molecule and the linkers between them, with what is double-bonded to either, as a
spelling-independent key (molkey.SmilesKeys' rule), as a SMILES spelling (randomize.SmilesRandomizer's write-out) and as
a per-atom membership, all from the labelled graph SmilesRandomizer.parse reads from a token row.

SmilesScaffolds.scaffold is THE statement for one part, scaffold_reference the batch rule; gct_smiles_scaffold
(csrc/scaffold.hip, SmilesScaffolds.scaffold_rows) implements them and is compared with them exactly.

The rule, for one part (a molecule's tokens, no <eos>, no <sep>):
  1. Core.  Repeatedly delete every atom that has at most one live neighbour.  What is left -- ring atoms and the linkers
     between rings -- is the core; an empty core is ACYCLIC.
  2. Shell.  A non-core atom with a bond of molkey label 2 (a written `=`) to a core atom is kept too.  Not recursive:
     the shell atom's other neighbours go.  O=C1CCCCC1C -> O=C1CCCCC1, CC(C)=C1CCCC1 -> C=C1CCCC1, CC(=O)c1ccccc1 ->
     c1ccccc1 (the carbonyl carbon is no core atom), c1ccccc1C(=O)c1ccccc1 keeps its =O (it is).
  3. Tokens.  Kept atoms and the bonds between two kept atoms carry their tokens verbatim, but for a kept atom whose
     token is the bare aromatic `n` and which loses at least one neighbour: it is spelled, and labelled for the key, as
     `[nH]` (Cn1cccc1 -> c1cc[nH]c1); NO_TOKEN when the vocabulary has no `[nH]`.  An `n` that keeps all its
     neighbours stays `n`.
  4. Key.  SmilesKeys' rule, unchanged, over the induced subgraph with those labels.  ACYCLIC: 0.
  5. Spelling.  The graph compacted to the kept atoms (ascending atom order, ascending bond order, bond lists filtered in
     place), written out by SmilesRandomizer.write_out from atom 0 -- the lowest kept atom -- over the lists in parse
     order; a ring takes the lowest free number.  NO_RING and TOO_LONG as in the randomiser.
  6. SYNTAX and UNSUPPORTED are the randomiser's (stereo marks, dots, / and \\, RING_BOND closures, a ninth bond): such a
     part has no scaffold -- key 0, empty spelling, no membership.
The scaffold of a scaffold is itself, in key and in spelling.

Where rdkit differs, on purpose: a bracket atom that loses a substituent keeps its token (rdkit adjusts the H count;
only the bare `n` is mended, because `c1cccn1` would not be aromatic); there is no aromaticity perception (tokens are
compared verbatim, as in molkey); there is no stereo removal (a part with a stereo mark is UNSUPPORTED); a dotted row has
no scaffold.  Generic (atom-anonymous) frameworks, scaffold similarity and substructure search are not here."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops
from .molkey import GOLD, SmilesKeys, as_int64, mix
from .smiles import check_token_rows, launch_rows, row_spans


class ScaffoldRows(NamedTuple):
    """What scaffold_rows / scaffold_reference return.  tokens int64 [n, out_width]: the spelling, <eos>, <pad>; key int64
    [n, 2] = (key of the extracted scaffold, key of the part in front of <sep> by the plain molkey rule, or 0); info int32
    [n, 4] = (ops.SCA_* status, ops.KEY_* status of the given part or -1, atoms kept, length of the spelling); member
    int32 [n, W]: per atom of the molecule, in order, 0 dropped, 1 core, 2 shell, -1 behind the atoms.  A row without
    <eos> in its span: <pad> tokens, keys 0, info (-1, -1, 0, 0), member -1."""
    tokens: torch.Tensor
    key: torch.Tensor
    info: torch.Tensor
    member: torch.Tensor


def scaffold_match(sca: ScaffoldRows) -> torch.Tensor:
    """bool [n] on the rows' device: the molecule has the scaffold it was given -- a scaffold was extracted (SCA_OK), the
    given part has a graph (KEY_GRAPH) and the two keys are equal.  No synchronisation."""
    return (sca.info[:, 0] == ops.SCA_OK) & (sca.info[:, 1] == ops.KEY_GRAPH) & (sca.key[:, 0] == sca.key[:, 1])


class SmilesScaffolds:
    """Murcko scaffolds of SMILES token rows over a target vocabulary, next to a SmilesKeys (self.keys: its labels and
    table) and its SmilesRandomizer (self.randomizer: the parse, the UNSUPPORTED set and the write-out).  self.n_id /
    self.nh_id: the ids of the tokens `n` and `[nH]`, None without one.  keys: a SmilesKeys over the same vocabulary and
    ids to share instead of building one.  ValueError for a vocabulary the randomiser rejects."""

    def __init__(self, itos, pad_id, eos_id, sep_id=None, keys=None):
        self.keys = ks = keys if keys is not None else SmilesKeys(itos, pad_id, eos_id, sep_id)
        self.randomizer = ks.randomizer
        self.pad_id, self.eos_id, self.sep_id = ks.pad_id, ks.eos_id, ks.sep_id
        names = list(ks.grammar.itos)
        self.n_id = names.index("n") if "n" in names else None
        self.nh_id = names.index("[nH]") if "[nH]" in names else None

    def __len__(self):
        return len(self.keys)

    # ------------------------------------------------------------------------------------------------ one part
    def scaffold(self, tokens, room=None):
        """THE statement for one part: tokens = its ids (no <eos>, no <sep>); room: the tokens the spelling may take
        (None: any).  Returns (status, scaffold tokens, member, key): member[a] = 0 dropped, 1 core, 2 shell per atom
        (empty for SYNTAX and UNSUPPORTED), the key as the signed integer an int64 tensor holds.  The tokens are empty
        with any status but SCA_OK; the key is 0 unless the status is SCA_OK, SCA_NO_RING or SCA_TOO_LONG.  The module
        docstring states the rule."""
        ks, rz = self.keys, self.randomizer
        tokens = [int(t) for t in tokens]
        parsed = rz.parse(tokens)
        if parsed is None:
            return ops.SCA_SYNTAX, [], [], 0
        apos, bonds, lists, unsupported = parsed
        if unsupported:
            return ops.SCA_UNSUPPORTED, [], [], 0
        A = len(apos)
        near = [[bonds[e][0] ^ bonds[e][1] ^ a for e in lists[a]] for a in range(A)]
        live = set(range(A))
        while True:                                              # 1. the core
            gone = {a for a in live if sum(v in live for v in near[a]) <= 1}
            if not gone:
                break
            live -= gone
        member = [int(a in live) for a in range(A)]
        if not live:
            return ops.SCA_ACYCLIC, [], member, 0
        for b in bonds:                                          # 2. the shell
            if ks.bond_label(tokens, apos, b) == 2 and (b[0] in live) != (b[1] in live):
                member[b[1] if b[0] in live else b[0]] = 2
        kept = [a for a in range(A) if member[a]]
        tokens = list(tokens)
        for a in kept:                                           # 3. the tokens
            if tokens[apos[a]] == self.n_id and any(not member[v] for v in near[a]):
                if self.nh_id is None:
                    return ops.SCA_NO_TOKEN, [], member, 0
                tokens[apos[a]] = self.nh_id
        index = {a: i for i, a in enumerate(kept)}               # 5. (first) compaction
        bond_index, new_bonds = {}, []
        for e, (a, b, sym) in enumerate(bonds):
            if member[a] and member[b]:
                bond_index[e] = len(new_bonds)
                new_bonds.append((index[a], index[b], sym))
        new_apos = [apos[a] for a in kept]
        new_lists = [[bond_index[e] for e in lists[a] if e in bond_index] for a in kept]
        colours = ks.colours(tokens, (new_apos, new_bonds, new_lists, False))   # 4. the key
        key = as_int64(mix(sum(mix(c) for c in colours) + len(kept) * GOLD + len(new_bonds)))
        written = rz.write_out(tokens, new_apos, new_bonds, new_lists, 0)
        if written is None:
            return ops.SCA_NO_RING, [], member, key
        if room is not None and len(written[0]) > room:
            return ops.SCA_TOO_LONG, [], member, key
        return ops.SCA_OK, written[0], member, key

    # --------------------------------------------------------------------------------------------------- batches
    @staticmethod
    def _out_width(W, out_width):
        out_width = W if out_width is None else int(out_width)
        if out_width < 1:
            raise ValueError(f"out_width {out_width} has no column for <eos>")
        return out_width

    def scaffold_reference(self, ys, start, out_width=None):
        """THE batch rule (gct_smiles_scaffold implements it), on the CPU.  Spans, absent rows and the two parts are
        smiles.row_spans': an absent row is a row without a scaffold (ScaffoldRows says what it gets).  Otherwise the part
        in front of the first <sep>, where there is one, is the GIVEN scaffold -- keyed by SmilesKeys' plain rule,
        whatever its status -- and the molecule goes through `scaffold` with room = min(out_width, 256) - 1: the spelling
        and its <eos> fit the output row and 256 tokens."""
        ys = torch.as_tensor(ys)
        check_token_rows(ys)                                   # (here too: ys is judged before out_width, start after it)
        n, W = ys.shape
        out_width = self._out_width(W, out_width)
        spans = row_spans(ys, start, self.eos_id, self.sep_id)
        tokens = torch.full((n, out_width), self.pad_id, dtype=torch.int64)
        key = torch.zeros(n, 2, dtype=torch.int64)
        info = torch.zeros(n, 4, dtype=torch.int32)
        member = torch.full((n, W), -1, dtype=torch.int32)
        for r, sp in enumerate(spans):
            if sp.molecule is None:
                info[r, 0] = info[r, 1] = -1
                continue
            given = None if sp.scaffold is None else self.keys._part(sp.scaffold)
            status, spelt, mem, k = self.scaffold(sp.molecule, min(out_width, ops.SCA_MAX_SPAN) - 1)
            tokens[r, :len(spelt) + 1] = torch.tensor(spelt + [self.eos_id], dtype=torch.int64)
            key[r, 0] = k
            key[r, 1] = as_int64(given[1]) if given else 0
            info[r] = torch.tensor([status, given[0] if given else -1, sum(1 for m in mem if m), len(spelt)])
            member[r, :len(mem)] = torch.tensor(mem, dtype=torch.int32)
        return ScaffoldRows(tokens, key, info, member)

    def scaffold_rows(self, ys, start, out_width=None):
        """The same on the device of ys: one gct_smiles_scaffold launch, no synchronisation.  ys integers [n, W]; start
        ints [n] (on the CPU: checked there, as SmilesKeys.key_rows does) or an int32 tensor on the device (taken as it
        is: a row outside the range has no scaffold).  ValueError for a span wider than 256 columns or a start outside
        [0, W]."""
        check_token_rows(ys)                                   # (here too: ys is judged before out_width, start after it)
        out_width = self._out_width(ys.shape[1], out_width)
        ys, st = launch_rows(ys, start, "the scaffolds take")
        table, labels = self.keys.device_tables(ys.device)
        ring_ids = self.randomizer.device_tables(ys.device)[1]
        rz = self.randomizer
        none = lambda v: -1 if v is None else v
        return ScaffoldRows(*ops.smiles_scaffold(ys, st, table, labels, ring_ids, len(rz.ring_ids), rz.open_id,
                                                 rz.close_id, self.pad_id, self.eos_id, none(self.sep_id),
                                                 none(self.n_id), none(self.nh_id), out_width))
