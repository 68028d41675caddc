#!/usr/bin/env python3
"""The host-callable parts of gct_smiles_check / _randomize / _key / _scaffold / _fp / _desc and gct_fp_tanimoto on the CPU
under AddressSanitizer and UBSan (no GPU needed): builds tools/smiles_walk_host.hip -- a stand-alone program around the
parse (csrc/smiles_graph.h), the check's walk and verdict (csrc/chem.hip), the list shuffle and the write-out
(csrc/smiles_walk.h), the key functions (csrc/smiles_key.h), the peel, marks and compaction of csrc/scaffold.hip, the
fingerprint and Tanimoto functions (csrc/smiles_fp.h) and the ring perception and per-atom descriptor functions
(csrc/smiles_desc.h), the host code sanitised -- into tools/_build/ and runs it once per
mode (--modes) over ROWS: molecules, kept rows, rows with
scaffolds, shells and [nH] substitutions, and the rows that fill the kernels' LDS records to their ends (chains of 63 ..
255, a ring of 253 atoms, branch depth 83 with and without a ring at the bottom, 84 branches on one atom, atoms with 8
and 9 bonds, 40 rings open at once).
  check      every row with <eos>, and: <pad> behind the <eos>, no <eos>, the empty span, another token behind <eos>,
             an id outside [0, V), spans of exactly 255 and 256 tokens; against SmilesChemistry.check
  randomize  every row under --keys keys with mixed room, and a two-ring vocabulary (NO_RING); against
             SmilesRandomizer.randomize
  key        every row and --spellings random spellings of it; against SmilesKeys
  scaffold   the same, every row with an `n` once more without an [nH] token, and every row with too little room;
             against SmilesScaffolds.scaffold
  fingerprint every row and --spellings random spellings of it; against SmilesFingerprints.fingerprint
  tanimoto   the pair, tile and fold functions on random fingerprints at three bit densities, with absent rows, rows
             of all 1024 bits and duplicates, for p = 1 and 2, in tiles and splits of several sizes (a few hundred
             pairs per case); against tanimoto_reference: best and arg exactly, total within m * 2^-53 * total
  descriptor every row and --spellings random spellings of it, and molecules that reach the TPSA lines, charged and
             unknown atoms; against SmilesDescriptors.describe
Exit status 1 for a sanitizer report or a line that differs."""
import argparse
import collections
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.smiles import SmilesChemistry  # noqa: E402
from gct_plus_amd.descriptor import SmilesDescriptors  # noqa: E402
from gct_plus_amd.fingerprint import FpRows, SmilesFingerprints, tanimoto_reference  # noqa: E402
from gct_plus_amd.molkey import as_int64  # noqa: E402
from gct_plus_amd.randomize import SmilesRandomizer, stream  # noqa: E402
from gct_plus_amd.scaffold import SmilesScaffolds  # noqa: E402

MODES = ("check", "randomize", "key", "scaffold", "fingerprint", "tanimoto", "descriptor")
ap = argparse.ArgumentParser()
ap.add_argument("--modes", nargs="+", choices=MODES, default=list(MODES))
ap.add_argument("--keys", type=int, default=40)
ap.add_argument("--spellings", type=int, default=4)
ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
a = ap.parse_args()

PATTERN = re.compile(r"(\[[^\]]+]|Br?|Cl?|N|O|S|P|F|I|b|c|n|o|s|p|\(|\)|\.|=|#|-|\+|\\|\/|:|~|@|\?|>|\*|\$|\%[0-9]{2}|[0-9])")
V = synthetic.CHEM_VOCAB
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
RING = [str(k) if k < 10 else f"%{k}" for k in range(40)]
ROWS = ["CCO", "c1ccccc1-c1ccccc1", "C12C3C4C1C5C2C3C45", "C1CCC2(CC1)CCCC2", "c1cc[nH]c1", "C=1CCCCC1", "C/C=C/C", "C1C1",
        "C.C", "C[C@@H](N)O", "C(", "C1CC", "", "C?C", "C=1CC#1", "C#N", "C%12CC%12", "C%64C%64", "C1CC11CC11CC1",
        "CCN1CCCC2(CCN(C(=O)c3cc(C)nc4ccccc34)C2)C1=O", "n1c2c(c(N)nc1N)c(C)c(Cc1cc(OC)ccc1OC)cn2", "c:1:c:c:c:c:c1", "C~C$C",
        "C1CCC2CCCCC2C1", "C1CCCC1C1CCCC1",
        "O=C1CCCCC1C", "CC(C)=C1CCCC1", "c1ccccc1C(=O)c1ccccc1", "CC(=O)c1ccccc1", "Cn1cccc1", "c1ccn(-c2ccccc2)c1",
        "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccccc1S(=O)(=O)c1ccccc1", "OS(=O)(=O)c1ccccc1", "c1ccccc1C(C)Cc1ccccc1",
        "C" * 63, "C" * 64, "C" * 65, "C" * 252, "C" * 255, "C1" + "C" * 251 + "C1", "CC1" + "C" * 249 + "C1C",
        "C" + "(C" * 83 + ")" * 83, "C" + "(C" * 83 + "1CC1" + ")" * 83, "C" + "(C)" * 84, "S" + "(C)" * 7 + "C",
        "S" + "(C)" * 8 + "C", "S1" + "(C)" * 6 + "CC1", "S1" + "(C)" * 7 + "CC1", "S" + "(S(C)(C)C)" * 7 + "C",
        "".join("C" + r for r in RING) * 2, "N" + "".join("C" + r for r in RING) * 2 + "O"]
SMALL = ["<unk>", "<pad>", "<sos>", "<eos>", "C", "0", "1", "2", "(", ")"]          # two usable ring numbers: NO_RING


def ids(s, vocab=V):
    return [vocab.index(t) for t in PATTERN.findall(s)]


sc = SmilesScaffolds(V, PAD, EOS)
ks, rz = sc.keys, sc.randomizer


def spellings(toks):
    """The row and --spellings random spellings of it."""
    out = [toks]
    for k in range(a.spellings):
        status, new, _ = rz.randomize(toks, stream(7, k, 0), 1.0, 255)
        if status == ops.RAND_OK:
            out.append(new)
    return out


# Per mode: (cases, lines, want, names).  A case is a token list, or a tuple that begins with one; lines(case) is what
# the harness reads for it; want(case, words of its output line) = (the line is the host statement's, the statement's
# status); names: status -> its name.
def mode_check():
    ch = SmilesChemistry(V, PAD, EOS)
    staged = lambda t: ((int(ch.grammar.table[t]) & 0xFFFF) | ch.words[t] << 16 if 0 <= t < len(V)
                        else ops.GRAMMAR_BANNED | ops.CHEM_NO_CAP << 16)
    cco = ids("CCO")
    cases = [ids(s) + [EOS] for s in ROWS if len(ids(s)) < 256]
    cases += [cco + [EOS, PAD, PAD], cco, [], ids("C.C") + [EOS], cco + [EOS, cco[0]], cco + [EOS, PAD, EOS],
              [cco[0], len(V), cco[0], EOS], [cco[0], -1, EOS], ids("cC") + [EOS], ids("C" * 254) + [EOS], ids("C" * 255) + [EOS],
              ids("C" * 256), ids("C" * 255), ids("C1" + "C" * 250 + "C1") + [EOS, PAD], ids("C" * 100) + [EOS] + [PAD] * 155]

    def want(toks, got):
        return [int(x) for x in got] == list(ch.check(toks)), ch.check(toks)[0]
    names = {getattr(ops, n): n[5:] for n in ("CHEM_OK", "CHEM_SYNTAX", "CHEM_VALENCE", "CHEM_RING_BOND", "CHEM_AROMATIC")}
    return cases, lambda toks: [[len(toks)], [staged(t) for t in toks]], want, names


def mode_randomize():
    cases = []
    for vocab, rows in ((V, ROWS), (SMALL, ["C01C2C0C12", "C1CC11CC11CC1", "C1CC1"])):
        r = SmilesRandomizer(vocab, 1, 3)
        for s in rows:
            toks = ids(s, vocab)
            rooms = [256, 255, len(toks), len(toks) + 1, len(toks) + 2]
            cases += [(toks, r, k, min(256, random.Random(k).choice(rooms))) for k in range(a.keys)]

    def lines(case):
        toks, r, k, room = case
        words, calls = stream(7, k, 0), 1 + 2 * (len(toks) + 1)
        return [[len(toks), calls, len(r.ring_ids), r.open_id, r.close_id, room], [r.words[t] for t in toks],
                [w for c in range(calls) for w in words(c)], r.ring_ids]

    def want(case, got):
        toks, r, k, room = case
        status, new, perm = r.randomize(toks, stream(7, k, 0), 1.0, room)
        same = int(got[0]) == status
        if same and status == ops.RAND_OK:
            n = int(got[1])
            entries = [int(x) for x in got[2:2 + n]]
            same = [e if e >= 0 else toks[-e - 1] for e in entries] == new and [int(x) for x in got[3 + n:]] == perm
        return same, status
    names = {getattr(ops, n): n[5:] for n in dir(ops) if n.startswith("RAND_") and n != "RAND_MAX_SPAN"}
    return cases, lines, want, names


def mode_key():
    cases = [t for s in ROWS for t in spellings(ids(s))]

    def want(toks, got):
        status, key, atoms, bonds = ks._part(toks)
        return [int(got[0]), as_int64(int(got[1])), int(got[2]), int(got[3])] == [status, as_int64(key), atoms, bonds], status
    names = {getattr(ops, n): n[4:] for n in ("KEY_GRAPH", "KEY_STRING_SYNTAX", "KEY_STRING_UNSUPPORTED")}
    return (cases, lambda toks: [[len(toks)], [ks.words[t] & 0xFFFFFF for t in toks], [ks.labels[t] for t in toks]], want,
            names)


def mode_scaffold():
    no_nh = SmilesScaffolds(V, PAD, EOS)
    no_nh.nh_id = None
    assert sc.n_id is not None and sc.nh_id is not None, "synthetic.CHEM_VOCAB spells n and [nH]"
    cases = []                                                    # (tokens, the statement to compare with, room)
    for s in ROWS:
        for t in spellings(ids(s)):
            cases.append((t, sc, 255))
            if sc.n_id in t:
                cases.append((t, no_nh, 255))
        cases.append((ids(s), sc, max(len(ids(s)) - 2, 0)))       # TOO_LONG for a row that is all scaffold

    def lines(case):
        toks, st, room = case
        nh = -1 if st.nh_id is None else st.nh_id
        return [[len(toks), len(rz.ring_ids), rz.open_id, rz.close_id, room, nh, ks.words[nh] if nh >= 0 else 0],
                [ks.labels[nh] if nh >= 0 else 0], [ks.words[t] & 0xFFFFFF | (t == sc.n_id) << 25 for t in toks],
                [ks.labels[t] for t in toks], rz.ring_ids]

    def want(case, got):
        toks, st, room = case
        status, spelt, member, key = st.scaffold(toks, room)
        head, row, mem = (part.split() for part in " ".join(got).split("|"))
        got_row = [int(v) if int(v) >= 0 else toks[-int(v) - 1] for v in row]
        return ([int(head[0]), as_int64(int(head[1])), int(head[2]), int(head[3]), got_row, [int(m) for m in mem]] ==
                [status, key, sum(1 for m in member if m), len(spelt), spelt, member]), status
    names = {getattr(ops, n): n[4:] for n in ("SCA_OK", "SCA_ACYCLIC", "SCA_SYNTAX", "SCA_UNSUPPORTED", "SCA_NO_TOKEN",
                                              "SCA_NO_RING", "SCA_TOO_LONG")}
    return cases, lines, want, names


def mode_fingerprint():
    fs = SmilesFingerprints(V, PAD, EOS, keys=ks)
    cases = [t for s in ROWS for t in spellings(ids(s))]

    def want(toks, got):
        status, words, atoms, bonds = fs._part(toks)
        return [int(x) for x in got] == [status, atoms, bonds] + words, status
    names = {getattr(ops, n): n[3:] for n in ("FP_GRAPH", "FP_SYNTAX", "FP_UNSUPPORTED")}
    return (cases, lambda toks: [[len(toks)], [ks.words[t] & 0xFFFFFF for t in toks], [ks.labels[t] for t in toks]], want,
            names)


def mode_tanimoto():
    import struct
    import torch
    rng = random.Random(5)

    def rows(n):
        """n fingerprints as lists of 32 words of 32 bits: densities 1/64, 1/8 and 1/2, row 1 full, row 2 absent, row 3
        a copy of row 0."""
        out = []
        for r in range(n):
            x = [rng.getrandbits(32) for _ in range(32)]
            for _ in range((5, 2, 0)[r % 3]):
                x = [w & rng.getrandbits(32) for w in x]
            out.append(x)
        if n >= 4:
            out[1], out[2], out[3] = [0xFFFFFFFF] * 32, [0] * 32, list(out[0])
        return out

    def fps(words):
        bits = torch.tensor([[(r[2 * k] | r[2 * k + 1] << 32) - ((r[2 * k + 1] >> 31) << 64) for k in range(16)] for r in words],
                            dtype=torch.int64).view(len(words), 16)
        info = torch.zeros(len(words), 4, dtype=torch.int32)
        info[:, 1] = torch.tensor([sum(bin(w).count("1") for w in r) for r in words], dtype=torch.int32)
        return FpRows(bits, info)

    cases = []                                                    # (a, b, p, tile, tiles per split)
    for na, nb, tile, tps in ((5, 9, 4, 1), (7, 33, 8, 2), (12, 40, 16, 1), (1, 1, 4, 1), (3, 0, 4, 1), (0, 5, 4, 1),
                              (9, 31, 32, 1), (6, 64, 5, 3), (16, 25, 128, 1), (4, 130, 128, 1)):
        for p in (1, 2):
            cases.append((rows(na), rows(nb), p, tile, tps))
    cases.append((rows(6), [[0] * 32] * 7, 1, 4, 1))              # no row of b is present

    def lines(case):
        a, b, p, tile, tps = case
        return [[len(a), len(b), p, tile, tps]] + [[sum(bin(w).count("1") for w in r)] + r for r in a + b]

    def want(case, got):
        a, b, p, tile, tps = case
        ref = tanimoto_reference(fps(a), fps(b), p)
        same = len(got) == 3 * len(a)
        for i in range(len(a) if same else 0):
            best = struct.unpack("f", struct.pack("I", int(got[3 * i])))[0]
            total = struct.unpack("d", struct.pack("Q", int(got[3 * i + 2])))[0]
            same &= best == ref.best[i].item() and int(got[3 * i + 1]) == ref.arg[i].item()
            same &= abs(total - ref.total[i].item()) <= len(b) * 2.0 ** -53 * ref.total[i].item()
        return same, p
    return cases, lines, want, {1: "p = 1:", 2: "p = 2:"}


def mode_descriptor():
    ds = SmilesDescriptors(V, PAD, EOS, keys=ks)
    more = ["CC(=O)Oc1ccccc1C(=O)O", "CC(=O)Nc1ccc(O)cc1", "c1ccccc1[N+](=O)[O-]", "C1CO1", "C1CN1", "CS(C)=O", "CS(=O)(=O)N",
            "C[N+](C)(C)C", "CC#CC", "c1ccccc1c1ccccc1", "c1ccc2ccccc2c1", "c1ccn2cccc2c1", "O=n1ccccc1", "C[n+]1ccccc1",
            "c1cc[nH+]cc1", "C[O-]", "c1ccoc1", "CN(=O)=O", "C=N#C", "C$N", "C*C", "C[2H]", "C[Si](C)C", "C[se]C", "FS(F)(F)(F)F",
            "c1" + "c" * 251 + "n1", "N" + "C" * 252 + "O"]
    cases = [t for s in ROWS + more for t in spellings(ids(s))]

    def want(toks, got):
        mine = ds.describe(toks)
        return [int(x) for x in got] == mine, mine[0]
    names = {getattr(ops, n): n[5:] for n in ("DESC_OK", "DESC_SYNTAX", "DESC_UNSUPPORTED", "DESC_UNKNOWN_ATOM")}
    return (cases, lambda toks: [[len(toks)], [ks.words[t] & 0xFFFFFF for t in toks], [ds.desc[t] for t in toks]], want,
            names)


build = os.path.join(ROOT, "tools", "_build")
os.makedirs(build, exist_ok=True)
exe = os.path.join(build, "smiles_walk_host")
san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
cmd = [a.hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result"]
cmd += [x for f in san for x in ("-Xarch_host", f)] + ["-fsanitize=address,undefined"]
subprocess.run(cmd + [os.path.join(ROOT, "tools", "smiles_walk_host.hip"), "-o", exe], check=True)

failed = False
for mode in a.modes:
    cases, lines, want, names = globals()["mode_" + mode]()
    path = os.path.join(build, f"smiles_walk_{mode}.txt")
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for case in cases:
            f.write("".join(" ".join(map(str, line)) + "\n" for line in lines(case)))
    run = subprocess.run([exe, mode, path], capture_output=True, text=True)
    if run.returncode != 0:
        print(run.stderr[-4000:])
        sys.exit(f"smiles_walk_check {mode}: the harness ended with status {run.returncode}")
    out = run.stdout.strip("\n").split("\n")
    assert len(out) == len(cases), (len(out), len(cases))
    bad, seen = 0, collections.Counter()
    for case, line in zip(cases, out):
        same, status = want(case, line.split())
        same = bool(same)
        seen[status] += 1
        if not same:
            bad += 1
            print(f"{mode} differs: ids", (case[0] if isinstance(case, tuple) else case)[:40], "->", line[:100])
    print(f"smiles_walk_check {mode}: {len(cases)} cases under ASan + UBSan, {bad} differ from the host statement; "
          + ", ".join(f"{names[s]} {c}" for s, c in sorted(seen.items())))
    failed |= bad > 0
sys.exit(1 if failed else 0)
