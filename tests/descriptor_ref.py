"""An independent oracle for gct_plus_amd.descriptor: token STRINGS in, nothing imported from the package.  The graph is
randomize_ref.read's reading of a part (adjacency by atom index, as chem_ref reads token strings); ring bonds are found
by brute force -- delete the bond and test whether its ends are still connected --, the smallest ring through a bond by
a second, different search (distances relaxed to a fixed point over the graph without the bond), components by
union-find; atoms are read by a small hand-written scanner of their own.

    describe(tokens) -> the 12 integers (status, heavy_atoms, hydrogens, mw_mda, charge, hbd, hba, rotatable, rings,
                        aromatic_rings, tpsa_centi, ring_bonds); status 0 OK, 1 SYNTAX, 2 UNSUPPORTED, 3 UNKNOWN_ATOM
    errors(values, targets) -> the reference's get_errors formulas over two lists, plus n

The rule, restated.  Elements B C N O F Si P S Cl Br I with masses 10810 12011 14007 15999 18998 28086 30974 32060
35450 79904 126904 mDa, H 1008; anything else, `*`, [H..], an isotope, an unreadable bracket or |charge| > 3 is unknown.
A bracket atom has its stated hydrogens; a bare atom fills up to its smallest normal valence >= sigma (B 3, C 4, N 3 5,
O 2, P 3 5, S 2 4 6, halogens 1; none: 0 hydrogens), an aromatic one to one less, never below 0.  Bond classes: - ~
single, = double, # triple, $ quadruple, : aromatic; unwritten single, but aromatic between two lower-case atoms when
the bond lies on a ring.  sigma counts an aromatic bond as 1.  Rotatable: single, not on a ring, both ends with two
bonds or more, neither end with a triple bond.  Aromatic rings: the cycle rank of the aromatic ring bonds' subgraph.
TPSA: Ertl's N and O lines in 0.01 A^2, the first match of _LINES, else the stated fallback."""
from tests import randomize_ref

OK, SYNTAX, UNSUPPORTED, UNKNOWN_ATOM = range(4)
_MASS = {"B": 10810, "C": 12011, "N": 14007, "O": 15999, "F": 18998, "Si": 28086, "P": 30974, "S": 32060, "Cl": 35450,
         "Br": 79904, "I": 126904}
_NORMAL = {"B": [3], "C": [4], "N": [3, 5], "O": [2], "P": [3, 5], "S": [2, 4, 6], "F": [1], "Cl": [1], "Br": [1], "I": [1]}
_ORDER = {"single": 1, "double": 2, "triple": 3, "quad": 4, "aromatic": 1}
_SYMBOL = {"-": "single", "~": "single", "=": "double", "#": "triple", "$": "quad", ":": "aromatic"}
# element, n, h, {class: count}, q, in a 3-ring (None: either) -> contribution
_LINES = [
    ("N", 1, 0, dict(triple=1), 0, None, 2379), ("N", 1, 1, dict(double=1), 0, None, 2385),
    ("N", 1, 2, dict(single=1), 0, None, 2602), ("N", 1, 2, dict(double=1), 1, None, 2559),
    ("N", 1, 3, dict(single=1), 1, None, 2764),
    ("N", 2, 0, dict(single=1, double=1), 0, None, 1236), ("N", 2, 0, dict(triple=1, double=1), 0, None, 1360),
    ("N", 2, 1, dict(single=2), 0, True, 2194), ("N", 2, 1, dict(single=2), 0, None, 1203),
    ("N", 2, 0, dict(triple=1, single=1), 1, None, 436), ("N", 2, 1, dict(double=1, single=1), 1, None, 1397),
    ("N", 2, 2, dict(single=2), 1, None, 1661), ("N", 2, 0, dict(aromatic=2), 0, None, 1289),
    ("N", 2, 1, dict(aromatic=2), 0, None, 1579), ("N", 2, 1, dict(aromatic=2), 1, None, 1414),
    ("N", 3, 0, dict(single=3), 0, True, 301), ("N", 3, 0, dict(single=3), 0, None, 324),
    ("N", 3, 0, dict(single=1, double=2), 0, None, 1168), ("N", 3, 0, dict(single=2, double=1), 1, None, 301),
    ("N", 3, 1, dict(single=3), 1, None, 444), ("N", 3, 0, dict(aromatic=3), 0, None, 441),
    ("N", 3, 0, dict(single=1, aromatic=2), 0, None, 493), ("N", 3, 0, dict(double=1, aromatic=2), 0, None, 410),
    ("N", 3, 0, dict(aromatic=3), 1, None, 410), ("N", 3, 0, dict(single=1, aromatic=2), 1, None, 388),
    ("N", 4, 0, dict(single=4), 1, None, 0),
    ("O", 1, 0, dict(double=1), 0, None, 1707), ("O", 1, 1, dict(single=1), 0, None, 2023),
    ("O", 1, 0, dict(single=1), -1, None, 2306),
    ("O", 2, 0, dict(single=2), 0, True, 1253), ("O", 2, 0, dict(single=2), 0, None, 923),
    ("O", 2, 0, dict(aromatic=2), 0, None, 1314)]


def read_atom(tok):
    """(element or None, charge, stated hydrogens, aromatic, bracket) of an atom token string."""
    unknown = (None, 0, 0, False, tok.startswith("["))
    if not tok.startswith("["):
        el = tok.capitalize()
        return (el, 0, 0, tok[0].islower(), False) if el in _MASS and tok in (el, el.lower()) else unknown
    if not tok.endswith("]"):
        return unknown
    body, i = tok[1:-1], 0
    if not body or body[0].isdigit() or body[0] == "*":         # an isotope, a wildcard, an empty bracket
        return unknown
    if not (body[0].isascii() and body[0].isalpha()):
        return unknown
    sym, i = body[0], 1
    if i < len(body) and body[i].isascii() and body[i].islower():
        sym, i = sym + body[i], i + 1
    marks = 0
    while i < len(body) and body[i] == "@":
        marks, i = marks + 1, i + 1
    if marks > 2:
        return unknown
    h = 0
    if i < len(body) and body[i] == "H":
        h, i = 1, i + 1
        if i < len(body) and body[i].isdigit():
            h, i = int(body[i]), i + 1
    q = 0
    if i < len(body) and body[i] in "+-":
        sign, j = (1 if body[i] == "+" else -1), i + 1
        if j < len(body) and body[j].isdigit():
            while j < len(body) and body[j].isdigit():
                j += 1
            q = sign * int(body[i + 1:j])
        else:
            while j < len(body) and body[j] == body[i]:
                j += 1
            q = sign * (j - i)
        i = j
    if i != len(body):
        return unknown
    el = sym.capitalize()
    if el not in _MASS or abs(q) > 3:
        return unknown
    return el, q, h, sym[0].islower(), True


def _connected(n, edges, a, b):
    near = {u: set() for u in range(n)}
    for u, v in edges:
        near[u].add(v), near[v].add(u)
    seen, todo = {a}, [a]
    while todo:
        for v in near[todo.pop()]:
            if v not in seen:
                seen.add(v), todo.append(v)
    return b in seen


def _distance(n, edges, a, b):
    """Path length from a to b by relaxing every edge until nothing changes (Bellman-Ford on unit weights)."""
    far = n + 1
    d = [far] * n
    d[a] = 0
    changed = True
    while changed:
        changed = False
        for u, v in edges:
            for x, y in ((u, v), (v, u)):
                if d[x] + 1 < d[y]:
                    d[y], changed = d[x] + 1, True
    return d[b]


def ring_sizes(n, edges):
    """{edge: the smallest ring through it} over the ring bonds only."""
    out = {}
    for e in edges:
        rest = [x for x in edges if x != e]
        if _connected(n, rest, *e):
            out[e] = 1 + _distance(n, rest, *e)
    return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def tpsa_term(el, n, h, counts, q, r3):
    mine = {k: v for k, v in counts.items() if v}
    for lel, ln, lh, lcounts, lq, lr3, value in _LINES:
        if (lel, ln, lh, lcounts, lq) == (el, n, h, mine, q) and (lr3 is None or r3):
            return value
    return max(0, (3050 - 820 * n if el == "N" else 2850 - 860 * n) + 150 * h)


def describe(tokens):
    tokens = list(tokens)
    if any(t is None for t in tokens):
        return [SYNTAX] + [0] * 11
    try:
        atoms, bonds, why = randomize_ref.read(tokens)
    except ValueError:
        return [SYNTAX] + [0] * 11
    n = len(atoms)
    if why:
        return [UNSUPPORTED, n] + [0] * 10
    reading = [read_atom(t) for t in atoms]
    if any(r[0] is None for r in reading):
        return [UNKNOWN_ATOM, n] + [0] * 10
    edges = list(bonds)
    size = ring_sizes(n, edges)
    kind = {}
    for e in edges:
        if bonds[e] is not None:
            kind[e] = _SYMBOL[bonds[e]]
        else:
            kind[e] = "aromatic" if e in size and reading[e[0]][3] and reading[e[1]][3] else "single"
    mine = {a: [e for e in edges if a in e] for a in range(n)}
    hydrogens, total = [], dict(mw=0, q=0, hbd=0, hba=0, tpsa=0)
    for a, (el, q, stated, aromatic, bracket) in enumerate(reading):
        sigma = sum(_ORDER[kind[e]] for e in mine[a])
        if bracket:
            h = stated
        else:
            fits = [v for v in _NORMAL.get(el, []) if v >= sigma]
            h = 0 if not fits else max(0, fits[0] - sigma - (1 if aromatic else 0))
        hydrogens.append(h)
        total["mw"] += _MASS[el] + 1008 * h
        total["q"] += q
        if el in "NO":
            total["hba"] += 1
            total["hbd"] += 1 if h else 0
            counts = {k: sum(1 for e in mine[a] if kind[e] == k) for k in _ORDER}
            total["tpsa"] += tpsa_term(el, len(mine[a]), h, counts, q, any(size.get(e) == 3 for e in mine[a]))
    has_triple = [any(kind[e] == "triple" for e in mine[a]) for a in range(n)]
    rotatable = sum(1 for e in edges if kind[e] == "single" and e not in size and all(
        len(mine[x]) >= 2 and not has_triple[x] for x in e))
    ring_arom = [e for e in edges if kind[e] == "aromatic" and e in size]
    parent = list(range(n))
    for u, v in ring_arom:
        parent[_find(parent, u)] = _find(parent, v)
    touched = {x for e in ring_arom for x in e}
    components = len({_find(parent, x) for x in touched})
    return [OK, n, sum(hydrogens), total["mw"], total["q"], total["hbd"], total["hba"], rotatable, len(edges) - n + 1,
            len(ring_arom) - len(touched) + components, total["tpsa"], len(size)]


def errors(values, targets):
    """get_errors as written: d = target - value; mae mean |d|, mse mean d, max, min, aard mean |d / target|, amsd mean
    d / target; zeros without rows."""
    d = [t - v for v, t in zip(values, targets)]
    k = len(d)
    if not k:
        return dict(mae=0.0, mse=0.0, max=0.0, min=0.0, aard=0.0, amsd=0.0, n=0)
    rel = [x / t for x, t in zip(d, targets)]
    return dict(mae=sum(abs(x) for x in d) / k, mse=sum(d) / k, max=max(d), min=min(d),
                aard=sum(abs(x) for x in rel) / k, amsd=sum(rel) / k, n=k)
