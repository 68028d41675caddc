"""The host statements about SMILES token rows, shared by everything that reads one: the grammar over a target vocabulary
(`SmilesGrammar`: grammar_step, grammar_min_finish, smiles_walk -- what KVDecoder masks logits with and what every parse
starts from), the chemistry check of finished rows (`SmilesChemistry`), and the batch rule that the SMILES kernels share
(csrc/smiles_graph.h smiles_stage_row): `row_spans` states which part of a row is the molecule and which the scaffold,
`launch_rows` is the prelude of a launch over such rows.  randomize.py, molkey.py, scaffold.py, fingerprint.py and
descriptor.py state their per-part rules over these; decode.py takes the grammar from here."""
from __future__ import annotations

import math
import re
from typing import NamedTuple

import torch

from . import ops


# ------------------------------------------------------------------------------------------------- small host helpers
def _int_vector(name, values, n, lo, hi, bound):
    """values as an int64 CPU tensor: integers of shape [n] in [lo, hi] (`bound` says in the message what hi is);
    ValueError otherwise."""
    v = torch.as_tensor(values)
    if v.dtype.is_floating_point or v.dtype.is_complex or v.dtype == torch.bool:
        raise ValueError(f"{name} must hold integers, got {v.dtype}")
    v = v.to("cpu", torch.int64)
    if v.dim() != 1 or v.numel() != n:
        raise ValueError(f"{name} must have shape [{n}], got {list(v.shape)}")
    if n and (int(v.min()) < lo or int(v.max()) > hi):
        raise ValueError(f"{name} must lie in [{lo}, {hi}] ({bound}), got [{int(v.min())}, {int(v.max())}]")
    return v


def on_device(cache, device, make):
    """cache[device], made by make() on first use: what `copied to a device once` means everywhere."""
    key = str(torch.device(device))
    if key not in cache:
        cache[key] = make()
    return cache[key]


def row_mask(name, mask, n, device):
    """mask as bool [n] on `device`: one boolean per row; ValueError otherwise (`name` is the argument's in the message)."""
    mask = torch.as_tensor(mask).to(device).reshape(-1)
    if mask.dtype != torch.bool or mask.numel() != n:
        raise ValueError(f"{name} must be {n} booleans, one per row")
    return mask


def chunked(iterable, chunk):
    """The items of `iterable` as lists of `chunk`, the last one shorter; ValueError for chunk < 1."""
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    batch = []
    for item in iterable:
        batch.append(item)
        if len(batch) == int(chunk):
            yield batch
            batch = []
    if batch:
        yield batch


# ------------------------------------------------------------------------------------- grammar-constrained decoding
# states `prev` of the grammar: what the last generated token was
(G_START, G_ATOM, G_RING, G_BOND_A, G_BOND_B, G_OPEN, G_CLOSE, G_DOT, G_END) = range(9)
GRAMMAR_START = (G_START, 0, 0, 0)                 # (prev, depth, open, here) before the first generated token
_ATOMS = frozenset("B Br C Cl N O S P F I b c n o s p *".split())
_BONDS = frozenset("= # - / \\ : ~ $".split())
_CHEM_BOND_ORDERS = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 1, "/": 1, "\\": 1, "~": 1}


def grammar_class(token):
    """(class, ring number) of a vocabulary string (ops.GRAMMAR_*): ATOM any [...] token and the organic subset, BOND,
    OPEN / CLOSE, RING a digit or %NN (ring NN; 64 and above BANNED), DOT; everything else BANNED (<eos> and <pad> are
    assigned by id, SmilesGrammar)."""
    t = str(token)
    if (len(t) >= 3 and t[0] == "[" and t[-1] == "]") or t in _ATOMS:
        return ops.GRAMMAR_ATOM, 0
    if t in _BONDS:
        return ops.GRAMMAR_BOND, 0
    if t == "(":
        return ops.GRAMMAR_OPEN, 0
    if t == ")":
        return ops.GRAMMAR_CLOSE, 0
    if t == ".":
        return ops.GRAMMAR_DOT, 0
    r = None
    if len(t) == 1 and t in "0123456789":
        r = int(t)
    elif len(t) == 3 and t[0] == "%" and t[1] in "0123456789" and t[2] in "0123456789":
        r = int(t[1:])
    if r is not None and r < ops.GRAMMAR_MAX_RINGS:
        return ops.GRAMMAR_RING, r
    return ops.GRAMMAR_BANNED, 0


def grammar_step(state, cls, ring=0):
    """The state after a token of class cls (ring number `ring`) in `state` = (prev, depth, open, here), or None when the
    grammar has no such transition.  THE statement of the transitions (gct_grammar_mask implements them):
      ATOM   from any state but END; here = {}
      BOND   from ATOM / RING (-> BOND_A) and from OPEN / CLOSE (-> BOND_B)
      OPEN   from ATOM / RING / CLOSE; depth + 1          CLOSE  from ATOM / RING / CLOSE when depth > 0; depth - 1
      RING r from ATOM / RING / BOND_A: r open -> closes it, unless r is in here (a ring does not close on the atom that
             opened it); otherwise opens it, r joins open and here
      DOT    from ATOM / RING / CLOSE when depth == 0
      EOS    from ATOM / RING / CLOSE when depth == 0 and no ring is open -> END;      from END only PAD."""
    prev, depth, open_, here = state
    if prev == G_END:
        return state if cls == ops.GRAMMAR_PAD else None
    ar = prev in (G_ATOM, G_RING)
    arc = ar or prev == G_CLOSE
    if cls == ops.GRAMMAR_ATOM:
        return G_ATOM, depth, open_, 0
    if cls == ops.GRAMMAR_BOND:
        if ar:
            return G_BOND_A, depth, open_, here
        return (G_BOND_B, depth, open_, here) if prev in (G_OPEN, G_CLOSE) else None
    if cls == ops.GRAMMAR_OPEN:
        return (G_OPEN, depth + 1, open_, here) if arc else None
    if cls == ops.GRAMMAR_CLOSE:
        return (G_CLOSE, depth - 1, open_, here) if arc and depth > 0 else None
    if cls == ops.GRAMMAR_RING:
        if not (ar or prev == G_BOND_A):
            return None
        bit = 1 << int(ring)
        if open_ & bit:
            return None if here & bit else (G_RING, depth, open_ ^ bit, here)
        return G_RING, depth, open_ | bit, here | bit
    if cls == ops.GRAMMAR_DOT:
        return (G_DOT, depth, open_, here) if arc and depth == 0 else None
    if cls == ops.GRAMMAR_EOS:
        return (G_END, 0, 0, 0) if arc and depth == 0 and open_ == 0 else None
    return None


def smiles_walk(grammar, tokens, row):
    """THE walk that reads a token span as a molecule, over a SmilesGrammar (chem_walk of csrc/chem.hip and rand_parse of
    csrc/smiles_graph.h implement it; SmilesChemistry.check and SmilesRandomizer.parse say what the events mean to them).  row: the span is a whole
    row -- the <eos> and whatever follows it included; otherwise a part, its <eos> implied behind it.  Atoms are numbered
    in token order.  An ATOM bonds to the atom the chain stands at (OPEN pushes that atom, CLOSE pops it, DOT clears it;
    the first atom has none); a BOND token directly in front states the order (- 1, = 2, # 3, $ 4, each of : / \\ ~ 1).
    A RING token belongs to the atom it follows; the first occurrence of an open number remembers the atom and the BOND
    token in front, the next one closes it.  Yields, in token order,
      ("atom", i)                    token i is the next atom
      ("bond", a, b, order, sym)     a chain bond between atoms a < b; order: the stated one or None; sym: that BOND
                                     token's position
      ("ring", a, b, order, sym)     a ring closure's bond: the closing end's order if it states one, else the opening end's
      ("clash", i)                   the closure at i adds no bond: both ends state an order and the two differ, or the two
                                     atoms are bonded already (by the chain or by an earlier closure)
      ("dot", i)
      ("syntax", i)                  the last event: the first token without a transition (grammar_step; an id outside
                                     [0, V) has none), or len(tokens) when the span lacks a good end"""
    g, tokens = grammar, [int(t) for t in tokens]
    st, atoms, cur, pend = GRAMMAR_START, 0, None, None        # pend: (order, position) of a BOND token that waits
    stack, open_rings, bonded = [], {}, set()
    for i, t in enumerate(tokens):
        st = grammar_step(st, g.classes[t], g.rings[t]) if 0 <= t < len(g) else None
        if st is None:
            yield "syntax", i
            return
        c = g.classes[t]
        if c == ops.GRAMMAR_ATOM:
            yield "atom", i
            if cur is not None:
                bonded.add((cur, atoms))
                yield ("bond", cur, atoms) + (pend or (None, None))
            cur, atoms = atoms, atoms + 1
        elif c == ops.GRAMMAR_BOND:
            pend = (_CHEM_BOND_ORDERS[g.itos[t]], i)
            continue
        elif c == ops.GRAMMAR_OPEN:
            stack.append(cur)
            continue
        elif c == ops.GRAMMAR_CLOSE:
            cur = stack.pop()
        elif c == ops.GRAMMAR_DOT:
            yield "dot", i
            cur = None
        elif c == ops.GRAMMAR_RING:
            if g.rings[t] in open_rings:
                a, first = open_rings.pop(g.rings[t])
                if (first and pend and first[0] != pend[0]) or (a, cur) in bonded:   # (a < cur: it closes on a later atom)
                    yield "clash", i
                else:
                    bonded.add((a, cur))
                    yield ("ring", a, cur) + (pend or first or (None, None))
            else:
                open_rings[g.rings[t]] = (cur, pend)
        pend = None
    if (st[0] != G_END) if row else grammar_step(st, ops.GRAMMAR_EOS) is None:
        yield "syntax", len(tokens)


def grammar_min_finish(state):
    """Length of the shortest allowed continuation of `state` that ends with <eos> (closed form; the host test checks it
    against a breadth-first search): 0 at END, otherwise depth + popcount(open) + 1 + a, where a = 1 when an atom has to
    come first -- after START / BOND_B / OPEN / DOT, after CLOSE with a ring open, after BOND_A with no ring open or one
    opened on this atom, after ATOM / RING with a ring opened on this atom."""
    prev, depth, open_, here = state
    if prev == G_END:
        return 0
    if prev in (G_START, G_BOND_B, G_OPEN, G_DOT):
        a = 1
    elif prev == G_CLOSE:
        a = int(open_ != 0)
    elif prev == G_BOND_A:
        a = int(open_ == 0 or (open_ & here) != 0)
    else:
        a = int((open_ & here) != 0)
    return depth + bin(open_).count("1") + 1 + a


def check_grammar(grammar, vocab, budget):
    """grammar None, or a SmilesGrammar over `vocab` tokens with a budget (an int, or ints [n]) of at least 2 generated
    tokens per row -- room for an atom and <eos>; ValueError otherwise."""
    if grammar is None:
        return
    if not isinstance(grammar, SmilesGrammar):
        raise ValueError(f"grammar must be a SmilesGrammar, got {type(grammar).__name__}")
    if len(grammar) != int(vocab):
        raise ValueError(f"the grammar classifies {len(grammar)} tokens, the model's vocabulary has {int(vocab)}")
    least = int(torch.as_tensor(budget).min())
    if least < 2:
        raise ValueError(f"grammar-constrained decoding needs at least 2 generated tokens per row, got {least}")


class SmilesGrammar:
    """SMILES syntax over a target vocabulary, for constrained decoding (KVDecoder.generate / generate_stream(grammar=)).
    The guarantee is SYNTACTIC: branches balance, ring-closure numbers pair up, bonds have an atom or a ring closure
    behind them, and the row ends with <eos> inside its length budget.  Chemical validity (valence, aromaticity, a ring
    bond doubling another, bond orders at the two ends of a ring closure) is not checked while decoding: SmilesChemistry
    checks finished rows for it.
    itos: the vocabulary's strings; token pad_id is PAD and token eos_id EOS whatever their strings, every other token is
    classified by grammar_class, and OPEN is BANNED in a vocabulary without CLOSE.  ValueError for a vocabulary without
    an ATOM token or without <eos> / <pad> ids inside it.
    A row may generate G tokens.  Choosing its g-th one (g = len(tokens)), a token is ALLOWED iff its transition exists
    (grammar_step) and grammar_min_finish(state') <= G - g - 1; a finished row and a row past its budget are allowed
    <pad> only.  Because min_finish is exact, the allowed set is never empty for G >= 2, and every row reaches <eos>."""

    def __init__(self, itos, pad_id, eos_id):
        self.itos = [str(t) for t in itos]
        V = len(self.itos)
        self.pad_id, self.eos_id = int(pad_id), int(eos_id)
        if not (0 <= self.eos_id < V and 0 <= self.pad_id < V and self.eos_id != self.pad_id):
            raise ValueError(f"the vocabulary ({V} tokens) has no <eos> / <pad> at ids {eos_id} / {pad_id}")
        entries = [grammar_class(t) for t in self.itos]
        entries[self.pad_id], entries[self.eos_id] = (ops.GRAMMAR_PAD, 0), (ops.GRAMMAR_EOS, 0)
        if not any(c == ops.GRAMMAR_CLOSE for c, _ in entries):
            entries = [(ops.GRAMMAR_BANNED, 0) if c == ops.GRAMMAR_OPEN else (c, r) for c, r in entries]
        if not any(c == ops.GRAMMAR_ATOM for c, _ in entries):
            raise ValueError("the vocabulary has no atom token: no SMILES can be generated from it")
        self.classes = [c for c, _ in entries]
        self.rings = [r for _, r in entries]
        self.table = torch.tensor([c | (r << 8) for c, r in entries], dtype=torch.int32)    # gct_grammar_mask's layout
        self._groups = {}                                  # (class, ring) -> the ids that share it
        for c, e in enumerate(entries):
            self._groups.setdefault(e, []).append(c)
        self._device_tables = {}

    def __len__(self):
        return len(self.itos)

    def device_table(self, device):
        """The class table on `device` (copied once)."""
        return on_device(self._device_tables, device, lambda: self.table.to(device))

    def state(self, tokens):
        """(prev, depth, open, here) after the generated token ids `tokens`; ValueError at a token the grammar forbids."""
        st = GRAMMAR_START
        for i, t in enumerate(tokens):
            nxt = grammar_step(st, self.classes[int(t)], self.rings[int(t)])
            if nxt is None:
                raise ValueError(f"token {i} ({self.itos[int(t)]!r}) is not allowed after {[self.itos[int(x)] for x in tokens[:i]]}")
            st = nxt
        return st

    def allowed(self, tokens, budget_left):
        """Sorted ids the row may choose next: tokens = its generated ids so far, budget_left = G - len(tokens), the slots
        it has left with this one.  THE reference for one row."""
        st = self.state(list(tokens))
        if st[0] == G_END or budget_left < 1:
            return [self.pad_id]
        out = []
        for (cls, ring), members in self._groups.items():
            nxt = grammar_step(st, cls, ring)
            if nxt is not None and grammar_min_finish(nxt) <= budget_left - 1:
                out += members
        return sorted(out)

    def mask_reference(self, logits, ys, starts, pos, G):
        """THE reference for a batch (gct_grammar_mask implements it): logits [n, V]; row r has generated
        ys[r, starts[r] : pos[r]] and chooses column pos[r] under the budget G[r] (starts / pos / G: ints or [n]).
        Returns a copy of logits with -inf on every token that is not allowed; a row with pos[r] < starts[r] (still
        inside its prefix) is returned as it is."""
        n = logits.shape[0]
        def per_row(v):
            v = [int(x) for x in torch.as_tensor(v).view(-1).tolist()]
            return v * n if len(v) == 1 else v
        starts, pos, G = per_row(starts), per_row(pos), per_row(G)
        out = logits.clone()
        ys = torch.as_tensor(ys).cpu()
        for r in range(n):
            if pos[r] < starts[r]:
                continue
            hist = ys[r, starts[r]:pos[r]].tolist()
            keep = torch.zeros(logits.shape[1], dtype=torch.bool)
            keep[self.allowed(hist, G[r] - len(hist))] = True
            out[r, ~keep.to(out.device)] = -math.inf
        return out

    def well_formed(self, tokens):
        """The same rules for a whole generated sequence: every token up to the first <eos> has its transition, the
        <eos> is there and allowed, and only <pad> follows it."""
        st = GRAMMAR_START
        for t in tokens:
            t = int(t)
            if not 0 <= t < len(self.itos):
                return False
            st = grammar_step(st, self.classes[t], self.rings[t])
            if st is None:
                return False
        return st[0] == G_END


# ------------------------------------------------------------------------------------------------- batches of rows
def check_token_rows(ys):
    """ys is a tensor [n, W >= 1] of an integer dtype; ValueError otherwise."""
    if ys.dim() != 2 or ys.shape[1] < 1:
        raise ValueError(f"ys must be [n, W >= 1] token rows, got {list(ys.shape)}")
    if ys.dtype.is_floating_point or ys.dtype.is_complex or ys.dtype == torch.bool:
        raise ValueError(f"ys must hold integer token ids, got {ys.dtype}")


class RowSpan(NamedTuple):
    """One row of row_spans: the row's ids, its start, its span's length, the scaffold's ids or None, the molecule's ids
    or None (an absent row)."""
    row: list
    start: int
    length: int
    scaffold: list
    molecule: list


def row_spans(ys, start, eos_id, sep_id, max_span=ops.SMILES_MAX_SPAN):
    """THE batch rule of the SMILES kernels (smiles_stage_row of csrc/smiles_graph.h implements it), on the CPU: a list
    with one RowSpan per row of ys integers [n, W >= 1], start n integers.  The row's span is row[start:], and length the
    span's -- 0 when the start lies outside [0, W] or the span is wider than max_span columns.  molecule is None for an
    absent row, one whose span holds no <eos>; otherwise the content is what stands in front of the first <eos>, and it
    is the molecule, or, with sep_id and a <sep> in it, the scaffold in front of the first <sep> and the molecule behind
    it.  scaffold is None without one.  ValueError for other shapes."""
    ys = torch.as_tensor(ys)
    check_token_rows(ys)
    n, W = ys.shape
    starts = [int(s) for s in torch.as_tensor(start).view(-1).tolist()]
    if len(starts) != n:
        raise ValueError(f"start must be {n} integers, one per row")
    out = []
    for row, t0 in zip(ys.cpu().tolist(), starts):
        span = row[t0:] if 0 <= t0 <= W and W - t0 <= max_span else []
        scaffold = molecule = None
        if eos_id in span:
            molecule = span[:span.index(eos_id)]
            if sep_id is not None and sep_id in molecule:
                s = molecule.index(sep_id)
                scaffold, molecule = molecule[:s], molecule[s + 1:]
        out.append(RowSpan(row, t0, len(span), scaffold, molecule))
    return out


def checked_starts(ys, start, what, name="start", max_span=ops.SMILES_MAX_SPAN):
    """start as int64 [n] on the CPU after the checks of a launch over ys: ys integers [n, W >= 1], then start integers in
    [0, W], no span wider than max_span columns.  `what` and `name` word the messages (`the keys take`, `start`)."""
    check_token_rows(ys)
    n, W = ys.shape
    lens = _int_vector(name, start, n, 0, W, "the row width")
    if n and W - int(lens.min()) > max_span:
        raise ValueError(f"a span of {W - int(lens.min())} columns: {what} at most {max_span}")
    return lens


def device_rows(ys, start):
    """(ys as int64 with unit column stride, start as int32 on ys's device: one copy, no synchronisation)."""
    ys = ys.to(torch.int64)
    ys = ys if ys.shape[1] == 1 or ys.stride(1) == 1 else ys.contiguous()
    if not (start.dtype == torch.int32 and start.device == ys.device):
        start = start.to(torch.int32).to(ys.device, non_blocking=True)
    return ys, start


def launch_rows(ys, start, what, name="start", max_span=ops.SMILES_MAX_SPAN):
    """THE prelude of a launch over token rows: device_rows of ys and of start -- ints [n] through checked_starts, or an
    int32 tensor on the GPU of ys, taken as it is (the kernel treats a row outside the range as absent)."""
    if torch.is_tensor(start) and start.device == ys.device and start.dtype == torch.int32 and ys.is_cuda:
        check_token_rows(ys)
    else:
        start = checked_starts(ys, start, what, name, max_span)
    return device_rows(ys, start)


# ------------------------------------------------------------------------------------------- chemical validity
_CHEM_CAPS = {"B": 3, "C": 4, "N": 3, "O": 2, "F": 1, "Si": 4, "P": 5, "S": 6, "Cl": 1, "Br": 1, "I": 5}
_CHEM_ROWS = (("B", "C", "N", "O", "F"), ("Al", "Si", "P", "S", "Cl"))
_CHEM_BRACKET = re.compile(r"\[(\d+)?([A-Z][a-z]?|[a-z][a-z]?|\*)(@{0,2})(H\d?)?(\++|-+|[+-]\d+)?\]")


def chem_atom_entry(token):
    """(cap or None, explicit H count, aromatic, carbon-like) of an ATOM token's string.
    Organic atoms: caps B 3, C 4, N 3, O 2, F 1, P 5, S 6, Cl 1, Br 1, I 5 (the largest valence of each: implicit
    hydrogens fill up to the next allowed one, so only the maximum can be exceeded); a lower-case symbol is aromatic;
    `*` has no cap.  A bracket atom reads [isotope? symbol chirality? H-count? charge?]: aromatic when the symbol is lower
    case, H the stated count (H alone: 1), and its effective element is the one `charge` places to the LEFT of it in its
    row B C N O F / Al Si P S Cl (the isoelectronic rule: [N+] is C, cap 4; [O-] is F, cap 1; [n+] is carbon-like); it
    takes that element's cap (Si 4; Al none) and has none when the shift leaves the row.  An element outside the two rows
    keeps its own cap at charge 0 and has none otherwise.  A bracket token the pattern does not match is a non-aromatic
    atom without a cap.  Carbon-like: the effective element is C."""
    t = str(token)
    if t.startswith("["):
        m = _CHEM_BRACKET.fullmatch(t)
        if not m:
            return None, 0, False, False
        sym, h, ch = m.group(2), m.group(4), m.group(5)
        if sym == "*":
            return None, (0 if not h else int(h[1:] or 1)), False, False
        q = 0 if not ch else (int(ch) if len(ch) > 1 and ch[1:].isdigit() else (len(ch) if ch[0] == "+" else -len(ch)))
        aromatic, el = sym[0].islower(), sym[0].upper() + sym[1:]
        eff = el if q == 0 else None
        for row in _CHEM_ROWS:
            if el in row:
                i = row.index(el) - q
                eff = row[i] if 0 <= i < len(row) else None
        return _CHEM_CAPS.get(eff), (0 if not h else int(h[1:] or 1)), aromatic, eff == "C"
    if t == "*":
        return None, 0, False, False
    el = t[0].upper() + t[1:]
    return _CHEM_CAPS.get(el), 0, t[0].islower(), el == "C"


class ChemReport(NamedTuple):
    """What SmilesChemistry.check_rows / check_reference return: int32 [n] each -- status (ops.CHEM_*), position of the
    first finding in the row's span (-1: none), atoms, ring_bonds."""
    status: torch.Tensor
    position: torch.Tensor
    atoms: torch.Tensor
    ring_bonds: torch.Tensor


class SmilesChemistry:
    """Chemical validity of FINISHED SMILES rows over a target vocabulary: a SmilesGrammar (self.grammar) and a second
    per-token table (self.chem, gct_smiles_check's layout: cap | H << 4 | aromatic << 8 | carbon-like << 9 |
    bond order << 12, ops.CHEM_NO_CAP for no cap; chem_atom_entry reads the atoms).  `check` is THE statement of the rules;
    gct_smiles_check (check_rows) implements it.  It is a check of decoded rows: it takes no part in the decode loop.
    The check is a NECESSARY condition.  It does not check Kekulé structure or ring membership beyond `anb`.  It does not
    check stereo marks, or a bracket atom whose valence is below its cap.  An atom without a cap is never flagged for
    valence.  grammar: a SmilesGrammar over the same itos, pad_id and eos_id to share instead of building one.  ValueError
    for a vocabulary that SmilesGrammar rejects."""

    def __init__(self, itos, pad_id, eos_id, grammar=None):
        self.grammar = grammar if grammar is not None else SmilesGrammar(itos, pad_id, eos_id)
        words = []
        for t, c in zip(self.grammar.itos, self.grammar.classes):
            w = ops.CHEM_NO_CAP
            if c == ops.GRAMMAR_ATOM:
                cap, h, aromatic, clike = chem_atom_entry(t)
                w = ((ops.CHEM_NO_CAP if cap is None else cap) | (min(h, 15) << 4) | (int(aromatic) << 8) |
                     (int(clike) << 9))
            elif c == ops.GRAMMAR_BOND:
                w |= _CHEM_BOND_ORDERS[t] << 12
            words.append(w)
        self.words = words
        self.chem = torch.tensor(words, dtype=torch.int32)
        self._device_tables = {}

    def __len__(self):
        return len(self.grammar)

    def device_tables(self, device):
        """(grammar table, chem table) on `device` (copied once)."""
        return on_device(self._device_tables, device, lambda: (self.grammar.device_table(device), self.chem.to(device)))

    def check(self, tokens):
        """(status, position, atoms, ring_bonds) of a row's generated ids `tokens` -- the <eos> and whatever follows it
        included, the prefix excluded.  Sequential, on the host.
        SYNTAX (SmilesGrammar.well_formed is false; ids outside [0, V) and an empty span included): position = the first
        token without a transition, or len(tokens) when no <eos> was reached; atoms = ring_bonds = 0.
        Otherwise the graph, atoms numbered in token order: an ATOM bonds to the atom the chain stands at (OPEN pushes
        that atom, CLOSE pops it, DOT clears it; the first atom has none) with the order of a BOND token directly in
        front of it, else 1 (- 1, = 2, # 3, $ 4, each of : / \\ ~ 1).  A RING token belongs to the atom it follows; the
        first occurrence of an open number remembers (atom, order or none), the next one closes it: both ends state an
        order and the two differ, or the two atoms are bonded already (by the chain or by an earlier closure) ->
        RING_BOND at the closing token and no bond is added; otherwise a bond of the stated order, 1 when neither end
        states one.  ring_bonds = closing ring tokens (rejected ones included), atoms = ATOM tokens.
        Per atom, with sigma the sum of its bond orders, mo the largest, anb its aromatic neighbours, H its explicit
        hydrogens and used = sigma + H + (1 if it is aromatic and carbon-like and mo < 2): VALENCE at the atom's token
        when its cap is known and used > cap; otherwise AROMATIC there when it is aromatic and anb < 2.
        The finding with the smallest position wins; OK has position -1."""
        tokens = [int(t) for t in tokens]
        atoms, findings, ring_bonds = [], [], 0                # atoms: [token position, word, sigma, mo, anb]
        for ev in smiles_walk(self.grammar, tokens, True):
            if ev[0] == "syntax":
                return ops.CHEM_SYNTAX, ev[1], 0, 0
            if ev[0] == "atom":
                atoms.append([ev[1], self.words[tokens[ev[1]]], 0, 0, 0])
            elif ev[0] in ("bond", "ring"):
                a, b, order = ev[1], ev[2], ev[3] or 1
                ring_bonds += ev[0] == "ring"
                for x, y in ((a, b), (b, a)):
                    atoms[x][2] += order
                    atoms[x][3] = max(atoms[x][3], order)
                    atoms[x][4] += (atoms[y][1] >> 8) & 1
            elif ev[0] == "clash":
                ring_bonds += 1
                findings.append((ev[1], ops.CHEM_RING_BOND))
        for pos, w, sigma, mo, anb in atoms:
            cap, h, aromatic, clike = w & 15, (w >> 4) & 15, (w >> 8) & 1, (w >> 9) & 1
            used = sigma + h + (1 if aromatic and clike and mo < 2 else 0)
            if cap != ops.CHEM_NO_CAP and used > cap:
                findings.append((pos, ops.CHEM_VALENCE))
            elif aromatic and anb < 2:
                findings.append((pos, ops.CHEM_AROMATIC))
        if findings:
            pos, status = min(findings)
            return status, pos, len(atoms), ring_bonds
        return ops.CHEM_OK, -1, len(atoms), ring_bonds

    def valid(self, tokens):
        return self.check(tokens)[0] == ops.CHEM_OK

    def check_reference(self, ys, prefix_lens):
        """THE batch rule (gct_smiles_check implements it): row r's span is ys[r, prefix_lens[r]:], handed to `check` whole,
        the <eos> and what follows it included (not row_spans' rule, on purpose).  ys integers [n, W >= 1], prefix_lens
        in [0, W], no span wider than ops.CHEM_MAX_SPAN columns.  A ChemReport on the CPU."""
        ys = torch.as_tensor(ys)
        lens = checked_starts(ys, prefix_lens, "the check takes", "prefix_lens").tolist()
        rows = ys.cpu().tolist()
        got = [self.check(row[t0:]) for row, t0 in zip(rows, lens)]
        return ChemReport(*(torch.tensor([g[k] for g in got], dtype=torch.int32) for k in range(4)))

    def check_rows(self, ys, prefix_lens):
        """The same on the device of ys (any integer dtype, [n, W]): one gct_smiles_check launch.  prefix_lens ints [n] (on
        the CPU, as DecodedRows holds them: no synchronisation; always checked there, whatever holds them).  ValueError for
        a span wider than 256 columns or prefix_lens outside [0, W]."""
        ys, lens = device_rows(ys, checked_starts(ys, prefix_lens, "the check takes", "prefix_lens"))
        return ChemReport(*ops.smiles_check(ys, lens, *self.device_tables(ys.device)).unbind(1))
