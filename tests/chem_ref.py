"""An independent oracle for smiles.SmilesChemistry: it reads token STRINGS (None for an id outside the vocabulary) by
recursive descent, builds explicit adjacency lists and judges them with its own code.  It shares nothing with
SmilesChemistry but the rule text of its docstrings: no grammar table, no transition function, no bracket pattern.

    verdict(token_strings) -> (status, position, atoms, ring_bonds)       status: 0 OK, 1 SYNTAX, 2 VALENCE, 3 RING_BOND,
                                                                                  4 AROMATIC
The parser is predictive: it never consumes a token that cannot continue a well-formed line, so the token it stops at is
the first one without a transition."""
OK, SYNTAX, VALENCE, RING_BOND, AROMATIC = range(5)

_ORGANIC = {"B": 3, "C": 4, "N": 3, "O": 2, "F": 1, "P": 5, "S": 6, "Cl": 1, "Br": 1, "I": 5}
_PERIODS = ["B C N O F".split(), "Al Si P S Cl".split()]
_PERIOD_CAPS = [[3, 4, 3, 2, 1], [None, 4, 5, 6, 1]]
_ORDERS = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 1, "/": 1, "\\": 1, "~": 1}


class Atom:
    def __init__(self, pos, cap, hydrogens, aromatic, carbon_like):
        self.pos, self.cap, self.hydrogens, self.aromatic, self.carbon_like = pos, cap, hydrogens, aromatic, carbon_like
        self.bonds = []                                   # [(neighbour Atom, order)]


def _bracket(body):
    """(cap, H, aromatic, carbon-like) of the inside of a bracket atom, or None when it does not read as
    isotope? symbol chirality? H-count? charge?"""
    i, n = 0, len(body)
    while i < n and body[i].isdigit():
        i += 1
    if i == n:
        return None
    if body[i] == "*":
        symbol, i = "*", i + 1
    elif body[i].isalpha() and body[i].isascii():
        symbol, i = body[i], i + 1
        if i < n and body[i].isascii() and body[i].islower() and body[i].isalpha():
            symbol, i = symbol + body[i], i + 1
    else:
        return None
    marks = 0
    while i < n and body[i] == "@":
        marks, i = marks + 1, i + 1
    if marks > 2:
        return None
    hydrogens = 0
    if i < n and body[i] == "H":
        hydrogens, i = 1, i + 1
        if i < n and body[i].isdigit():
            hydrogens, i = int(body[i]), i + 1
    charge = 0
    if i < n and body[i] in "+-":
        sign = 1 if body[i] == "+" else -1
        if i + 1 < n and body[i + 1].isdigit():
            j = i + 1
            while j < n and body[j].isdigit():
                j += 1
            charge, i = sign * int(body[i + 1:j]), j
        else:
            j = i
            while j < n and body[j] == body[i]:
                j += 1
            charge, i = sign * (j - i), j
    if i != n:
        return None
    if symbol == "*":
        return None, hydrogens, False, False
    aromatic = symbol[0].islower()
    element = symbol[0].upper() + symbol[1:]
    for period, caps in zip(_PERIODS, _PERIOD_CAPS):
        if element in period:
            k = period.index(element) - charge            # a positive charge: the element to the left
            if k < 0 or k >= len(period):
                return None, hydrogens, aromatic, False
            return caps[k], hydrogens, aromatic, period[k] == "C"
    return (_ORGANIC.get(element) if charge == 0 else None), hydrogens, aromatic, False


def atom_reading(tok):
    """(cap or None, H, aromatic, carbon-like) of an atom token string."""
    if tok.startswith("["):
        got = _bracket(tok[1:-1])
        return got if got is not None else (None, 0, False, False)
    if tok == "*":
        return None, 0, False, False
    element = tok[0].upper() + tok[1:]
    return _ORGANIC.get(element), 0, tok[0].islower(), element == "C"


def _kind(tok):
    if tok is None:
        return "other"
    if (len(tok) > 2 and tok[0] == "[" and tok[-1] == "]") or tok in _ORGANIC or tok in ("b", "c", "n", "o", "s", "p", "*"):
        return "atom"
    if tok in _ORDERS:
        return "bond"
    if len(tok) == 1 and tok in "0123456789":
        return "ring"
    if len(tok) == 3 and tok[0] == "%" and tok[1] in "0123456789" and tok[2] in "0123456789":
        return "ring" if int(tok[1:]) < 64 else "other"
    return {"(": "open", ")": "close", ".": "dot", "<eos>": "eos", "<pad>": "pad"}.get(tok, "other")


class _Stop(Exception):
    def __init__(self, position):
        self.position = position


class _Reader:
    """line   := chain ('.' chain)* <eos> <pad>*       no ring open and no branch open at <eos>
       chain  := unit (bond? unit)*
       unit   := atom (bond? ring)* branch*            a ring number does not open and close on one atom
       branch := '(' bond? chain ')'
    A bond is consumed first and must then be followed by an atom or, directly behind an atom or a ring, by a ring."""

    def __init__(self, toks):
        self.t, self.i = list(toks), 0
        self.atoms, self.open, self.findings, self.closures = [], {}, [], 0

    def kind(self):
        return _kind(self.t[self.i]) if self.i < len(self.t) else "end"

    def stop(self):
        raise _Stop(self.i)

    def line(self):
        self.chain(None, None)
        while self.kind() == "dot":
            self.i += 1
            self.chain(None, None)
        if self.kind() != "eos" or self.open:
            self.stop()
        self.i += 1
        while self.i < len(self.t):
            if self.kind() != "pad":
                self.stop()
            self.i += 1

    def chain(self, parent, order):
        """Atoms in a row, the first bonded to `parent` (None: nothing) with `order` (None: not stated)."""
        while True:
            atom, order = self.unit(parent, order)
            k = self.kind()
            if k == "bond" and order is None:
                order = _ORDERS[self.t[self.i]]
                self.i += 1
                if self.kind() != "atom":
                    self.stop()
            elif k != "atom" and order is None:
                return
            parent = atom

    def unit(self, parent, order):
        """One atom with its ring marks and branches.  Returns (the atom, the order of a bond that was read behind its
        ring marks and still waits for its atom, or None)."""
        if self.kind() != "atom":
            self.stop()
        atom = Atom(self.i, *atom_reading(self.t[self.i]))
        self.i += 1
        self.atoms.append(atom)
        if parent is not None:
            self.bond(parent, atom, 1 if order is None else order)
        opened_here = set()
        while True:
            stated = None
            if self.kind() == "bond":
                stated = _ORDERS[self.t[self.i]]
                self.i += 1
                if self.kind() == "atom":
                    return atom, stated
                if self.kind() != "ring":
                    self.stop()
            if self.kind() != "ring":
                break
            r = int(self.t[self.i].lstrip("%"))
            if r in self.open:
                if r in opened_here:
                    self.stop()
                other, first = self.open.pop(r)
                self.closures += 1
                if (first is not None and stated is not None and first != stated) or self.bonded(other, atom):
                    self.findings.append((self.i, RING_BOND))
                else:
                    self.bond(other, atom, stated if stated is not None else first if first is not None else 1)
            else:
                self.open[r] = (atom, stated)
                opened_here.add(r)
            self.i += 1
        while self.kind() == "open":
            self.i += 1
            inner = None
            if self.kind() == "bond":
                inner = _ORDERS[self.t[self.i]]
                self.i += 1
            self.chain(atom, inner)
            if self.kind() != "close":
                self.stop()
            self.i += 1
        return atom, None

    @staticmethod
    def bonded(a, b):
        return any(x is b for x, _ in a.bonds)

    @staticmethod
    def bond(a, b, order):
        a.bonds.append((b, order))
        b.bonds.append((a, order))


def verdict(tokens):
    """tokens: the span's token strings, "<pad>" and "<eos>" for the two special ids and None for an id outside the
    vocabulary.  (status, position, atoms, ring_bonds)."""
    rd = _Reader(tokens)
    try:
        rd.line()
    except _Stop as e:
        return SYNTAX, e.position, 0, 0
    found = list(rd.findings)
    for a in rd.atoms:
        sigma = sum(o for _, o in a.bonds)
        top = max([o for _, o in a.bonds], default=0)
        ring_mates = sum(1 for x, _ in a.bonds if x.aromatic)
        used = sigma + a.hydrogens + (1 if a.aromatic and a.carbon_like and top < 2 else 0)
        if a.cap is not None and used > a.cap:
            found.append((a.pos, VALENCE))
        elif a.aromatic and ring_mates < 2:
            found.append((a.pos, AROMATIC))
    if not found:
        return OK, -1, len(rd.atoms), rd.closures
    position, status = min(found)
    return status, position, len(rd.atoms), rd.closures
