"""SMILES randomisation (the reference's -randomize_prob, Utils/dataset.py:263-267 and Utils/smiles.py:494-502, without
rdkit): a row's molecule written out again by a random depth-first traversal of the graph that
smiles.SmilesChemistry.check reads from it.  Atom tokens are carried verbatim and every bond keeps the symbol it was
written with, or none; no stereo perception and no aromaticity model take part.

SmilesRandomizer.randomize is THE statement for one part, randomize_reference the batch rule; gct_smiles_randomize
(csrc/randomize.hip, SmilesRandomizer.randomize_rows) implements them and is compared with them token for token.

Not covered, on purpose: rdkit's own distribution over spellings (this is a root-uniform, neighbour-uniform DFS), stereo
removal (a part with a stereo mark is left as it is), dotted rows, kekulisation, and anything in the decode loop."""
from __future__ import annotations

import struct
from typing import NamedTuple

import torch

from . import ops
from .smiles import (SmilesGrammar, _CHEM_BOND_ORDERS, check_token_rows, launch_rows, on_device, row_spans,
                     smiles_walk)

MAX_DEGREE = 8                       # bonds per atom a part may have (more: UNSUPPORTED)
_M0, _M1, _W0, _W1, _M32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """The project's Philox4x32-10 (csrc/common.h gct_philox) on Python ints: 4 counter words, 2 key words -> 4 words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return c0, c1, c2, c3


def stream(seed, key, part):
    """words(index) of the randomiser's stream (seed, key, part): the four Philox words of the counter
    (key low, key high, part, index) under the key (seed low, seed high ^ site word) of site ops.RANDOMIZE_SITE --
    csrc/common.h states the convention.  key: the row's int64, taken as its 64 bits."""
    seed, key = int(seed) & 0xFFFFFFFFFFFFFFFF, int(key) & 0xFFFFFFFFFFFFFFFF
    k = (seed & _M32, (seed >> 32) ^ ((ops.RANDOMIZE_SITE * 0x9E3779B9 + 0x7F4A7C15) & _M32))
    return lambda index: philox4x32_10((key & _M32, key >> 32, part, index), k)


def coin_threshold(p):
    """floor(float32(p) * 2^32): a part is randomised iff p >= 1 or word x of call 0 is below it."""
    return int(struct.unpack("f", struct.pack("f", float(p)))[0] * 4294967296.0)


class Randomized(NamedTuple):
    """What randomize_rows / randomize_reference return.  tokens int64 [n, out_width]; info int32 [n, 4] = (status of
    the molecule part, status of the scaffold part or -1, new span length with <eos>, atoms); perm int32 [n, out_width]
    (None unless asked for) = the input atom index of the k-th output atom of the span, -1 behind them."""
    tokens: torch.Tensor
    info: torch.Tensor
    perm: torch.Tensor


class SmilesRandomizer:
    """Random spellings of SMILES token rows over a target vocabulary: a SmilesGrammar (self.grammar) and one word per
    token (self.table, gct_smiles_randomize's layout: class | ring number << 8 | bond order << 16 | unsupported << 20,
    `unsupported` on the bonds / and \\ and on an atom token whose string holds @).
    self.ring_ids: the ids of the ring numbers 1 .. 63 that the vocabulary spells, ascending by number, the
    single-character spelling where a number has both.  ValueError for a vocabulary SmilesGrammar rejects, or one without
    `(` and `)`: no branch could be written.  grammar: a SmilesGrammar over the same itos, pad_id and eos_id to share
    instead of building one."""

    def __init__(self, itos, pad_id, eos_id, sep_id=None, grammar=None):
        self.grammar = g = grammar if grammar is not None else SmilesGrammar(itos, pad_id, eos_id)
        self.pad_id, self.eos_id = g.pad_id, g.eos_id
        self.sep_id = None if sep_id is None else int(sep_id)
        if self.sep_id is not None and not (0 <= self.sep_id < len(g) and self.sep_id not in (g.pad_id, g.eos_id)):
            raise ValueError(f"the vocabulary ({len(g)} tokens) has no <sep> at id {sep_id}")
        if "(" not in g.itos or ")" not in g.itos:
            raise ValueError("the vocabulary has no `(` / `)` tokens: a randomised SMILES cannot write a branch")
        self.open_id, self.close_id = g.itos.index("("), g.itos.index(")")
        words, rings = [], {}
        for i, (t, c, r) in enumerate(zip(g.itos, g.classes, g.rings)):
            w = c | (r << 8)
            if c == ops.GRAMMAR_BOND:
                w |= (_CHEM_BOND_ORDERS[t] << 16) | (int(t in "/\\") << 20)
            elif c == ops.GRAMMAR_ATOM:
                w |= int("@" in t) << 20
            elif c == ops.GRAMMAR_RING and 1 <= r <= 63 and (r not in rings or len(t) == 1):
                rings[r] = i
            words.append(w)
        self.words = words
        self.table = torch.tensor(words, dtype=torch.int32)
        self.ring_ids = [rings[r] for r in sorted(rings)]
        self._device_tables = {}

    def __len__(self):
        return len(self.grammar)

    def device_tables(self, device):
        """(token table int32 [V], ring ids int32 [64], -1 behind the last) on `device` (copied once)."""
        def make():
            rid = torch.tensor(self.ring_ids + [-1] * (64 - len(self.ring_ids)), dtype=torch.int32)
            return self.table.to(device), rid.to(device)

        return on_device(self._device_tables, device, make)

    # ------------------------------------------------------------------------------------------------ one part
    def parse(self, tokens):
        """A part's graph as SmilesChemistry.check reads it, or None when the part followed by <eos> is not well formed
        (an id outside [0, V) included): (apos, bonds, lists, unsupported).  apos[a]: token position of atom a, atoms in
        token order; bonds[e] = (a, b, sym) with a < b and sym the POSITION of the BOND token written for it, or None --
        for a ring closure the closing end's if it has one, else the opening end's; lists[a]: the indices of a's bonds in
        parse order.  unsupported: the part holds a DOT, a token the table marks, a ring closure `check` reports as
        RING_BOND (its ends state different orders, or the two atoms are bonded already; no bond is added), or a bond
        that would be some atom's ninth (not added)."""
        apos, bonds, lists, unsupported = [], [], [], False
        for ev in smiles_walk(self.grammar, tokens, False):
            if ev[0] == "syntax":
                return None
            if ev[0] == "atom":
                apos.append(ev[1]), lists.append([])
            elif ev[0] in ("bond", "ring"):
                a, b, sym = ev[1], ev[2], ev[4]
                if len(lists[a]) >= MAX_DEGREE or len(lists[b]) >= MAX_DEGREE:
                    unsupported = True
                else:
                    lists[a].append(len(bonds)), lists[b].append(len(bonds))
                    bonds.append((a, b, sym))
            else:                                                # clash, dot
                unsupported = True
        return apos, bonds, lists, unsupported or any((self.words[t] >> 20) & 1 for t in tokens)

    def write_out(self, tokens, apos, bonds, lists, root):
        """Passes 1 and 2 of `randomize` on their own: the graph (apos, bonds, lists) of `parse`, one connected component,
        written out from `root` over the lists as they stand.  Returns (new tokens, perm), or None when no ring number
        was free.  (SmilesScaffolds spells a scaffold with it.)"""
        A = len(apos)
        other = lambda e, a: bonds[e][0] ^ bonds[e][1] ^ a
        # pass 1
        parent, opener, visited = {root: None}, {}, {root}     # parent[a]: the bond the search came by; opener[e]: an atom
        stack = [[root, 0]]
        while stack:
            u, i = stack[-1]
            if i == len(lists[u]):
                stack.pop()
                continue
            stack[-1][1] += 1
            e = lists[u][i]
            v = other(e, u)
            if e == parent[u] or e in opener:
                continue
            if v in visited:
                opener[e] = v
            else:
                visited.add(v)
                parent[v] = e
                stack.append([v, 0])
        assert len(visited) == A                               # (no DOT: the part is one component)
        # pass 2
        out, perm, number = [], [], {}
        free = list(range(len(self.ring_ids)))

        def atom(u):
            out.append(tokens[apos[u]]), perm.append(u)
            closed = []
            for e in lists[u]:
                if e not in opener:
                    continue
                if opener[e] == u:
                    if bonds[e][2] is not None:
                        out.append(tokens[bonds[e][2]])
                    if not free:
                        return False
                    number[e] = free.pop(0)
                    out.append(self.ring_ids[number[e]])
                else:
                    out.append(self.ring_ids[number[e]])
                    closed.append(number[e])
            free.extend(closed), free.sort()
            return True

        if not atom(root):
            return None
        stack = [[root, 0, False]]
        left = {u: sum(1 for e in lists[u] if e not in opener and e != parent[u]) for u in range(A)}
        while stack:
            u, i, paren = stack[-1]
            while i < len(lists[u]) and (lists[u][i] in opener or lists[u][i] == parent[u]):
                i += 1
            if i == len(lists[u]):
                stack.pop()
                if paren:
                    out.append(self.close_id)
                continue
            stack[-1][1] = i + 1
            e = lists[u][i]
            left[u] -= 1
            branch = left[u] > 0
            if branch:
                out.append(self.open_id)
            if bonds[e][2] is not None:
                out.append(tokens[bonds[e][2]])
            if not atom(other(e, u)):
                return None
            stack.append([other(e, u), 0, branch])
        return out, perm

    def randomize(self, tokens, words, p=1.0, room=None):
        """THE statement for one part: tokens = its ids (no <eos>, no <sep>), words = the part's stream -- a function
        index -> 4 words (stream()), or a dict of them (a missing index: four zeros).  p: the coin's probability; room:
        the columns the new spelling may take (None: any).  Returns (status, new tokens, perm): perm[k] = the input atom
        of the k-th output atom; with any status but RAND_OK the tokens are the input's and perm is the identity over
        the atoms (empty for SYNTAX).
          SYNTAX, then UNSUPPORTED (parse), are decided first; then the coin, call 0 word x: KEPT unless p >= 1 or
          x < coin_threshold(p).  Root = floor(y * atoms / 2^32), y word 1 of call 0.  The list of atom a (its INPUT
          index) is shuffled by Fisher-Yates from the back: for i = deg - 1 .. 1, j = floor(w * (i + 1) / 2^32), swap
          entries i and j, with w = word (i - 1) & 3 of call 1 + 2 a + ((i - 1) >> 2).
          Pass 1, a depth-first search from the root over the shuffled lists: a bond to an unvisited atom is a tree edge
          and is followed at once; a bond to a visited atom, other than the edge the search came by, is a ring bond
          whose OPENING end is that visited atom (an ancestor).
          Pass 2, emission per atom: its own token; its ring bonds in list order -- an opening writes the bond's symbol,
          if any, and the lowest free ring number, and takes it (none free: NO_RING); a closing writes the bond's number,
          which is free again from the NEXT atom on; then its children in list order, each behind its bond's symbol,
          every child but the last inside `(` `)` with the symbol behind the `(`.
          TOO_LONG when the new spelling has more than `room` tokens."""
        get = words if callable(words) else (lambda i: words.get(i, (0, 0, 0, 0)))
        tokens = [int(t) for t in tokens]
        parsed = self.parse(tokens)
        if parsed is None:
            return ops.RAND_SYNTAX, tokens, []
        apos, bonds, lists, unsupported = parsed
        A, same = len(apos), list(range(len(apos)))
        if unsupported:
            return ops.RAND_UNSUPPORTED, tokens, same
        x, y = get(0)[:2]
        if not (p >= 1 or x < coin_threshold(p)):
            return ops.RAND_KEPT, tokens, same
        root = (y * A) >> 32
        lists = [list(l) for l in lists]
        for a, l in enumerate(lists):
            for i in range(len(l) - 1, 0, -1):
                j = (get(1 + 2 * a + ((i - 1) >> 2))[(i - 1) & 3] * (i + 1)) >> 32
                l[i], l[j] = l[j], l[i]
        written = self.write_out(tokens, apos, bonds, lists, root)
        if written is None:
            return ops.RAND_NO_RING, tokens, same
        out, perm = written
        if room is not None and len(out) > room:
            return ops.RAND_TOO_LONG, tokens, same
        return ops.RAND_OK, out, perm

    # --------------------------------------------------------------------------------------------------- batches
    def _check_batch(self, ys, key, p, out_width):
        check_token_rows(ys)
        n, W = ys.shape
        key = torch.as_tensor(key)
        if key.dtype.is_floating_point or key.dim() != 1 or key.numel() != n:
            raise ValueError(f"key must be {n} integers, one per row, got {list(key.shape)} {key.dtype}")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"p must be a probability in [0, 1], got {p}")
        out_width = W if out_width is None else int(out_width)
        if out_width < W:
            raise ValueError(f"out_width {out_width} is narrower than the rows ({W} columns)")
        return key.to(torch.int64), out_width

    def randomize_reference(self, ys, start, key, seed, p=1.0, out_width=None, return_perm=True):
        """THE batch rule (gct_smiles_randomize implements it), on the CPU.  Spans, absent rows and the two parts are
        smiles.row_spans': an absent row is a row-level SYNTAX: columns [0, W) are copied and info = (SYNTAX, -1, span
        length or 0, 0).  Otherwise whatever follows the first <eos> is dropped, the molecule is part 0 and the scaffold,
        where there is one, part 1.  Each part goes through `randomize` with stream(seed, key_r, part), the scaffold
        first.  room: the row may take
        min(out_width - start_r, 256) columns, less <eos>, less -- for the scaffold -- the <sep> and the molecule's input
        length, less -- for the molecule -- the <sep> and the scaffold's new length.
        Output row: columns [0, start_r) copied, the parts with <sep> between them, <eos>, <pad> up to out_width.
        info[2] = the new span length with <eos>; info[3] = atoms of the parts that are not SYNTAX; perm numbers the atoms
        across those parts in row order."""
        ys = torch.as_tensor(ys)
        key, out_width = self._check_batch(ys, key, p, out_width)
        n, W = ys.shape
        spans = row_spans(ys, start, self.eos_id, self.sep_id)
        out = torch.full((n, out_width), self.pad_id, dtype=torch.int64)
        info = torch.zeros(n, 4, dtype=torch.int32)
        perm = torch.full((n, out_width), -1, dtype=torch.int32)
        for r, ((row, t0, length, scaffold, molecule), k) in enumerate(zip(spans, key.tolist())):
            if molecule is None:
                out[r, :W] = torch.tensor(row, dtype=torch.int64)
                info[r] = torch.tensor([ops.RAND_SYNTAX, -1, length, 0])
                continue
            parts = [(0, molecule)] if scaffold is None else [(1, scaffold), (0, molecule)]
            total = min(out_width - t0, ops.RAND_MAX_SPAN)
            new, atoms, pm, status = [], 0, [], {1: -1}
            for which, toks in parts:
                room = total - 1 - (1 + len(parts[1][1]) if which == 1 else len(new))
                st, got, pp = self.randomize(toks, stream(seed, k, which), p, room)
                status[which] = st
                new += got + ([self.sep_id] if which == 1 else [])
                pm += [atoms + a for a in pp]
                atoms += len(pp)
            new.append(self.eos_id)
            out[r, :t0] = torch.tensor(row[:t0], dtype=torch.int64)
            out[r, t0:t0 + len(new)] = torch.tensor(new, dtype=torch.int64)
            info[r] = torch.tensor([status[0], status[1], len(new), atoms])
            perm[r, :atoms] = torch.tensor(pm, dtype=torch.int32)
        return Randomized(out, info, perm if return_perm else None)

    def randomize_rows(self, ys, start, key, seed, p=1.0, out_width=None, return_perm=False):
        """The same on the device of ys: one gct_smiles_randomize launch, no synchronisation.  ys integers [n, W];
        start ints [n] (on the CPU: checked there, as SmilesChemistry.check_rows does) or an int32 tensor on the device
        (taken as it is: a row outside the range is a row-level SYNTAX); key integers [n]; seed an int.  ValueError for a
        span wider than 256 columns, a start outside [0, W], p outside [0, 1] or out_width < W."""
        key, out_width = self._check_batch(ys, key, p, out_width)
        ys, st = launch_rows(ys, start, "the randomiser takes")
        table, ring_ids = self.device_tables(ys.device)
        tokens, info, perm = ops.smiles_randomize(
            ys, st, key.to(ys.device, non_blocking=True), table, ring_ids, len(self.ring_ids), self.open_id, self.close_id,
            self.pad_id, self.eos_id, -1 if self.sep_id is None else self.sep_id, int(seed), float(p), out_width,
            return_perm=return_perm)
        return Randomized(tokens, info, perm)
