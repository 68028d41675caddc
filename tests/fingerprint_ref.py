"""An independent oracle for gct_plus_amd.fingerprint: token STRINGS in, nothing imported from the package.  The graph
is molkey_ref.graph's reading of a part (randomize_ref.read tells SYNTAX from UNSUPPORTED), mix and fnv are molkey_ref's;
the fingerprint rule, Tanimoto, internal diversity and SNN are written out again from their statements.

    fingerprint(tokens)  -> (status, the 1024 bits as one Python int); status 0 GRAPH, 1 SYNTAX, 2 UNSUPPORTED
    words(bits)          -> the 16 signed 64-bit words an int64 tensor holds
    tanimoto(x, y)       -> T of two non-empty fingerprints, rounded once to fp32
    aggregate(xs, ys, p) -> per x: (best T, lowest index attaining it, sum of T^p) over the non-empty ys
    int_div(xs, p)       -> 1 - mean_i((sum_j T(i, j)^p / N)^(1/p)) over the non-empty xs, self pairs counted
    snn(xs, ys)          -> mean over the non-empty xs of max_j T(x, y_j)

The rule, restated.  id_0(a) = mix(fnv(atom string) ^ mix(0x200 + number of bonds of a)); two rounds id'(a) = mix(3 id(a)
+ sum over bonds (b, o) of mix(id(b) ^ mix(o + 0x100))); every id of every round, the first included, sets bit id mod
1024.  T = |x & y| / (|x| + |y| - |x & y|), the quotient rounded to fp32 (through a double: innocuous for a division,
53 >= 2 * 24 + 2)."""
import struct

from tests import randomize_ref
from tests.molkey_ref import fnv, graph, mix

GRAPH, SYNTAX, UNSUPPORTED = range(3)
RADIUS = 2
BITS = 1024


def fingerprint(tokens):
    tokens = list(tokens)
    try:
        why = randomize_ref.read(tokens)[2]
    except ValueError:
        return SYNTAX, 0
    if why:
        return UNSUPPORTED, 0
    atoms, near = graph(tokens)
    ids = [mix(fnv(t) ^ mix(0x200 + len(near[a]))) for a, t in enumerate(atoms)]
    bits = 0
    for r in range(RADIUS + 1):
        for x in ids:
            bits |= 1 << (x % BITS)
        ids = [mix(3 * ids[a] + sum(mix(ids[b] ^ mix(o + 0x100)) for b, o in near[a].items())) for a in range(len(atoms))]
    return GRAPH, bits


def words(bits):
    out = []
    for w in range(BITS // 64):
        x = (bits >> (64 * w)) & ((1 << 64) - 1)
        out.append(x - (1 << 64) if x >> 63 else x)
    return out


def popcount(x):
    return bin(x).count("1")


def fp32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def tanimoto(x, y):
    c = popcount(x & y)
    return fp32(c / (popcount(x) + popcount(y) - c))


def aggregate(xs, ys, p=1):
    out = []
    for x in xs:
        ts = [(tanimoto(x, y), j) for j, y in enumerate(ys) if x and y]
        if not ts:
            out.append((0.0, -1, 0.0))
            continue
        best = max(t for t, _ in ts)
        total = 0.0
        for t, _ in ts:
            total += t ** p
        out.append((best, min(j for t, j in ts if t == best), total))
    return out


def int_div(xs, p=1):
    xs = [x for x in xs if x]
    if not xs:
        return 0.0
    N = len(xs)
    return 1.0 - sum((sum(tanimoto(x, y) ** p for y in xs) / N) ** (1.0 / p) for x in xs) / N


def snn(xs, ys):
    xs, ys = [x for x in xs if x], [y for y in ys if y]
    if not xs or not ys:
        return 0.0
    return sum(max(tanimoto(x, y) for y in ys) for x in xs) / len(xs)
