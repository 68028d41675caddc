"""An independent oracle for gct_plus_amd.molkey: token STRINGS in, nothing imported from the package.  The graph is
randomize_ref.read's reading of a part, the aromatic flag chem_ref.atom_reading's; the key rule is written out again from
its statement, and `isomorphic` is a backtracking labelled-graph isomorphism test that knows nothing about keys.

    graph(tokens)      -> (atom strings, {atom: {neighbour: bond label}}), or None for a part without a graph
    key(tokens)        -> (status, key as an unsigned 64-bit int); status 0 GRAPH, 1 STRING_SYNTAX, 2 STRING_UNSUPPORTED
    isomorphic(g, h)   -> the two graphs are one labelled graph under some atom permutation

The rule, restated.  mix(x): x ^= x >> 30; x *= BF58476D1CE4E5B9; x ^= x >> 27; x *= 94D049BB133111EB; x ^= x >> 31, all
mod 2^64.  L(a) = FNV-1a-64 of the atom token's string.  Bond label: - 1, = 2, # 3, $ 4, : 5, ~ 6; without a symbol 5
between two aromatic atom tokens, else 1.  c0(a) = mix(L(a) + sum_b mix(L(b) ^ mix(dist(a, b) + 1))) over every b
reachable from a, a included; three rounds c'(a) = mix(3 c(a) + sum over bonds (b, o) of mix(c(b) ^ mix(o + 0x100)));
key = mix(sum_a mix(c(a)) + atoms * 9E3779B97F4A7C15 + bonds).  A part without a graph: h = A0761D6478BD642F, per token
h = mix((h + 9E3779B97F4A7C15) ^ FNV(token string)), key = mix(h + number of tokens)."""
from tests import chem_ref
from tests import randomize_ref

GRAPH, STRING_SYNTAX, STRING_UNSUPPORTED = range(3)
ROUNDS = 3
_MASK = (1 << 64) - 1
_LABELS = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 5, "~": 6}


def mix(x):
    x &= _MASK
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _MASK
    x ^= x >> 31
    return x


def fnv(text):
    h = 14695981039346656037
    for byte in text.encode("utf-8"):
        h = (h ^ byte) * 1099511628211 & _MASK
    return h


def signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _reading(tokens):
    """(atoms, {(a, b): symbol or None}) of a part, "syntax" or "unsupported"."""
    try:
        atoms, bonds, why = randomize_ref.read(tokens)
    except ValueError:
        return "syntax"
    return "unsupported" if why else (atoms, bonds)


def graph(tokens):
    got = _reading(list(tokens))
    if isinstance(got, str):
        return None
    atoms, bonds = got
    near = {a: {} for a in range(len(atoms))}
    for (a, b), symbol in bonds.items():
        if symbol is not None:
            label = _LABELS[symbol]
        else:
            label = 5 if chem_ref.atom_reading(atoms[a])[2] and chem_ref.atom_reading(atoms[b])[2] else 1
        near[a][b] = near[b][a] = label
    return atoms, near


def string_key(tokens):
    h = 0xA0761D6478BD642F
    for t in tokens:
        h = mix((h + 0x9E3779B97F4A7C15) ^ fnv(t))
    return mix(h + len(tokens))


def graph_key(atoms, near, rounds=ROUNDS, profile=True):
    """The key of a graph; rounds and profile are there so that a test can show what each step is needed for."""
    n = len(atoms)
    L = [fnv(t) for t in atoms]
    colour = []
    for a in range(n):
        total = 0
        if profile:
            dist = {a: 0}
            queue = [a]
            for u in queue:                                  # (the list grows while it is walked: breadth first)
                for v in near[u]:
                    if v not in dist:
                        dist[v] = dist[u] + 1
                        queue.append(v)
            total = sum(mix(L[b] ^ mix(d + 1)) for b, d in dist.items())
        colour.append(mix(L[a] + total))
    for _ in range(rounds):
        colour = [mix(3 * colour[a] + sum(mix(colour[b] ^ mix(o + 0x100)) for b, o in near[a].items())) for a in range(n)]
    bonds = sum(len(v) for v in near.values()) // 2
    return mix(sum(mix(c) for c in colour) + n * 0x9E3779B97F4A7C15 + bonds)


def key(tokens):
    tokens = list(tokens)
    got = _reading(tokens)
    if got == "syntax":
        return STRING_SYNTAX, string_key(tokens)
    if got == "unsupported":
        return STRING_UNSUPPORTED, string_key(tokens)
    return GRAPH, graph_key(*graph(tokens))


def isomorphic(g, h):
    """Backtracking over the atoms of g in breadth-first order: an atom goes to an unused atom of h with the same
    string and degree whose bonds to the images of g's placed neighbours exist with the same labels."""
    (atoms_g, near_g), (atoms_h, near_h) = g, h
    n = len(atoms_g)
    if n != len(atoms_h) or sorted(atoms_g) != sorted(atoms_h):
        return False
    ends = lambda atoms, near: sorted((tuple(sorted((atoms[a], atoms[b]))), o) for a in near for b, o in near[a].items() if a < b)
    if ends(atoms_g, near_g) != ends(atoms_h, near_h):
        return False                                         # (the same bond count: an injective bond-preserving map is onto)
    order, seen = [], set()
    for root in range(n):
        if root in seen:
            continue
        seen.add(root), order.append(root)
        i = len(order) - 1
        while i < len(order):
            for v in near_g[order[i]]:
                if v not in seen:
                    seen.add(v), order.append(v)
            i += 1
    image, used = {}, set()

    def place(i):
        if i == n:
            return True
        u = order[i]
        for v in range(n):
            if v in used or atoms_h[v] != atoms_g[u] or len(near_h[v]) != len(near_g[u]):
                continue
            if any(w in image and near_h[v].get(image[w]) != o for w, o in near_g[u].items()):
                continue
            image[u] = v
            used.add(v)
            if place(i + 1):
                return True
            del image[u]
            used.discard(v)
        return False

    return place(0)
