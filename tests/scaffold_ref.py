"""An independent oracle for gct_plus_amd.scaffold: token STRINGS in, nothing imported from the package.  The graph is
molkey_ref.graph's (randomize_ref.read's reading of a part); the core is found by another route than the statement's
peeling, and the shell and [nH] rules are written out again from the rule's text.  The SPELLING is not restated: the tests
check it by its properties (it parses back to the key, it is a fixed point).

    scaffold(tokens, has_nh=True) -> None for a part without a graph, else (member, atoms, key):
        member[a] 0 dropped / 1 core / 2 shell per atom; atoms: the kept atoms' token strings in order ([nH] where the
        rule substitutes it), None when the vocabulary lacks the token; key: molkey_ref.graph_key of the induced
        subgraph (unsigned), 0 for an empty core and None with atoms None.

The core, restated.  A bond is a RING bond iff its two ends stay connected when the bond is taken away (brute force: one
search per bond).  A ring atom is an end of a ring bond.  The core is the ring atoms plus every atom that lies on a path
between two ring atoms: in a tree of what is left when ring bonds are contracted that is "the atom separates two ring
atoms" -- taking the atom away leaves ring atoms in at least two of the pieces, or the atom is a ring atom itself.
The shell: a non-core atom joined to a core atom by a bond of label 2; nothing else of it is kept.  [nH]: a kept atom
whose string is exactly `n` and that has a dropped neighbour."""
from tests import molkey_ref


def _reach(near, start, without_bond=None, without_atom=None):
    seen, todo = {start}, [start]
    while todo:
        a = todo.pop()
        for b in near[a]:
            if b in seen or b == without_atom or without_bond in ((a, b), (b, a)):
                continue
            seen.add(b), todo.append(b)
    return seen


def core(near):
    atoms = sorted(near)
    ring = set()
    for a in atoms:
        for b in near[a]:
            if a < b and b in _reach(near, a, without_bond=(a, b)):
                ring |= {a, b}
    out = set(ring)
    for a in atoms:
        if a in ring:
            continue
        pieces = 0
        left = set(near[a])
        while left:
            piece = _reach(near, left.pop(), without_atom=a)
            left -= piece
            pieces += bool(piece & ring)
        if pieces >= 2:
            out.add(a)
    return out


def scaffold(tokens, has_nh=True):
    g = molkey_ref.graph(list(tokens))
    if g is None:
        return None
    atoms, near = g
    kept = core(near)
    member = [int(a in kept) for a in range(len(atoms))]
    if not kept:
        return member, [], 0
    for a in sorted(kept):
        for b, label in near[a].items():
            if b not in kept and label == 2:
                member[b] = 2
    order = [a for a in range(len(atoms)) if member[a]]
    names = []
    for a in order:
        lost = any(not member[b] for b in near[a])
        names.append("[nH]" if atoms[a] == "n" and lost else atoms[a])
    if "[nH]" in names and not has_nh:
        return member, None, None
    index = {a: i for i, a in enumerate(order)}
    sub = {index[a]: {index[b]: o for b, o in near[a].items() if member[b]} for a in order}
    # a bond without a symbol between aromatic tokens has label 5 whether the token reads n or [nH]: near's labels stand
    return member, names, molkey_ref.graph_key(names, sub)
