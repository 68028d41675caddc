"""An independent oracle for gct_plus_amd.randomize: token STRINGS in, token strings out, recursive where the package
is iterative, and nothing imported from the package.  It shares with SmilesRandomizer the rule text only.

    read(tokens)                        -> (atom strings, {(a, b): bond symbol or None}, why) of one well-formed part
    same_graph(tokens_in, tokens_out, perm) -> the two parts are one labelled graph under the atom permutation
    words(seed, key, part, index)       -> the four Philox words of the randomiser's stream
    coin(seed, key, part, p)            -> the part is randomised
    spell(tokens, ring_tokens, seed, key, part) -> (status, new tokens, perm), p = 1

The streams, restated: Philox4x32-10 under the key (seed low, seed high ^ (site * 9E3779B9 + 7F4A7C15)) with site 5A11E5;
counter (key low, key high, part, index); index 0 gives the coin (word 0: randomise iff p >= 1 or word <
floor(float32(p) * 2^32)) and the root (word 1: floor(word * atoms / 2^32)); step i = deg - 1 .. 1 of the Fisher-Yates
shuffle of INPUT atom a's bond list takes word (i - 1) % 4 of index 1 + 2 a + (i - 1) // 4, j = floor(word * (i + 1) / 2^32)."""
import functools
import sys

import numpy as np

from tests import chem_ref
from tests.rng_ref import philox4x32_10, rng_key

OK, KEPT, SYNTAX, UNSUPPORTED, NO_RING, TOO_LONG = range(6)
SITE = 0x5A11E5
_ORDERS = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 1, "/": 1, "\\": 1, "~": 1}


def words(seed, key, part, index):
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    return [int(w) for w in philox4x32_10((key & 0xFFFFFFFF, key >> 32, part, index), rng_key(seed, SITE))]


def word_table(seed, key, part, count):
    """The words of indices 0 .. count - 1, one Philox evaluation over the whole range: [count][4] ints."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    cols = philox4x32_10((key & 0xFFFFFFFF, key >> 32, part, np.arange(count, dtype=np.int64)), rng_key(seed, SITE))
    return np.stack([np.broadcast_to(c, (count,)) for c in cols], 1).tolist()


def coin(seed, key, part, p):
    return p >= 1 or words(seed, key, part, 0)[0] < int(float(np.float32(p)) * 4294967296.0)


def read(tokens):
    return _read(tuple(tokens))


@functools.lru_cache(maxsize=4096)
def _read(tokens):
    """One part's token strings (no <eos>) -> (atoms, bonds, why): atoms the atom strings in token order, bonds
    {(a, b) with a < b: symbol string or None}, why = None, or what makes the part unsupported ("dot", "stereo", "ring
    bond", "degree").  ValueError when the part followed by <eos> is not well formed."""
    if chem_ref.verdict(list(tokens) + ["<eos>"])[0] == chem_ref.SYNTAX:
        raise ValueError("not well formed")
    atoms, bonds, degree, why = [], {}, {}, None
    branch, rings, here, bond = [], {}, None, None

    def join(a, b, sym):
        nonlocal why
        if degree.get(a, 0) >= 8 or degree.get(b, 0) >= 8:
            why = why or "degree"
            bonds.setdefault((a, b), "?")                      # (remembered as bonded; the part is unsupported anyway)
            return
        bonds[(a, b)] = sym
        degree[a], degree[b] = degree.get(a, 0) + 1, degree.get(b, 0) + 1

    for t in tokens:
        kind = chem_ref._kind(t)
        if kind == "atom":
            atoms.append(t)
            if "@" in t:
                why = why or "stereo"
            if here is not None:
                join(here, len(atoms) - 1, bond)
            here, bond = len(atoms) - 1, None
        elif kind == "bond":
            bond = t
            if t in "/\\":
                why = why or "stereo"
        elif kind == "open":
            branch.append(here)
        elif kind == "close":
            here, bond = branch.pop(), None
        elif kind == "dot":
            here, bond, why = None, None, why or "dot"
        elif kind == "ring":
            r = int(t.lstrip("%"))
            if r in rings:
                other, first = rings.pop(r)
                if (first and bond and _ORDERS[first] != _ORDERS[bond]) or (other, here) in bonds:
                    why = why or "ring bond"
                else:
                    join(other, here, bond or first)
            else:
                rings[r] = (here, bond)
            bond = None
    return atoms, bonds, why


def same_graph(tokens_in, tokens_out, perm):
    """The output part is the input part's graph under perm (perm[k] = the input atom of output atom k): the same atom
    strings, the same bond set, every bond with the same symbol."""
    a_in, b_in, _ = read(tokens_in)
    a_out, b_out, _ = read(tokens_out)
    perm = [int(p) for p in perm]
    if sorted(perm) != list(range(len(a_in))) or len(a_out) != len(a_in):
        return False
    if any(a_out[k] != a_in[perm[k]] for k in range(len(perm))):
        return False
    moved = {tuple(sorted((perm[a], perm[b]))): s for (a, b), s in b_out.items()}
    return moved == b_in


def spell(tokens, ring_tokens, seed, key, part=0, room=None):
    """The rule by recursion, for a part the coin lets through: (status, new token strings, perm).  ring_tokens: the
    vocabulary's spellings of the ring numbers 1 .. 63 it has, lowest number first."""
    try:
        atoms, bonds, why = read(tokens)
    except ValueError:
        return SYNTAX, list(tokens), []
    same = list(range(len(atoms)))
    if why:
        return UNSUPPORTED, list(tokens), same
    near = {a: [] for a in same}                            # atom -> [(neighbour, symbol, bond)] in parse order
    for (a, b), s in bonds.items():                        # (dicts keep insertion order: the order the bonds were read in)
        near[a].append((b, s, (a, b)))
        near[b].append((a, s, (a, b)))
    drawn = word_table(seed, key, part, 1 + 2 * len(atoms))
    root = (drawn[0][1] * len(atoms)) >> 32
    for a in same:
        lst = near[a]
        for i in range(len(lst) - 1, 0, -1):
            j = (drawn[1 + 2 * a + (i - 1) // 4][(i - 1) % 4] * (i + 1)) >> 32
            lst[i], lst[j] = lst[j], lst[i]
    opener, kids, seen = {}, {a: [] for a in same}, set()

    def visit(u, via):
        seen.add(u)
        for v, s, e in near[u]:
            if e == via or e in opener:
                continue
            if v in seen:
                opener[e] = v
            else:
                kids[u].append((v, s))
                visit(v, e)

    out, perm, free, number = [], [], list(range(len(ring_tokens))), {}

    def write(u):
        out.append(atoms[u])
        perm.append(u)
        back = []
        for v, s, e in near[u]:
            if e not in opener:
                continue
            if opener[e] == u:
                if s:
                    out.append(s)
                if not free:
                    raise OverflowError
                number[e] = min(free)
                free.remove(number[e])
            else:
                back.append(number[e])
            out.append(ring_tokens[number[e]])
        free.extend(back)
        for n, (v, s) in enumerate(kids[u]):
            inner = n < len(kids[u]) - 1
            out.extend((["("] if inner else []) + ([s] if s else []))
            write(v)
            if inner:
                out.append(")")

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * len(atoms) + 200))
    try:
        visit(root, None)
        write(root)
    except OverflowError:
        return NO_RING, list(tokens), same
    finally:
        sys.setrecursionlimit(limit)
    if room is not None and len(out) > room:
        return TOO_LONG, list(tokens), same
    return OK, out, perm
