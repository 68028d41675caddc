#!/usr/bin/env python3
"""The host-callable parts of gct_smiles_scaffold on the CPU under AddressSanitizer and UBSan (no GPU needed): builds
tools/scaffold_walk_host.hip -- a stand-alone program around rand_parse (csrc/smiles_graph.h), the peel, the shell and
[nH] marks and the compaction of csrc/scaffold.hip, the per-atom key functions (csrc/smiles_key.h) and rand_walk
(csrc/smiles_walk.h), the host code sanitised -- into tools/_build/, feeds it tools/molkey_walk_check.py's rows, rows with
scaffolds, shells and [nH] substitutions, the rows that fill the kernel's LDS record to its ends (chains of 63 .. 255,
a ring of 253 atoms, branch depth 83 with a ring at the bottom, an atom with 8 bonds of which two are in a ring, 40 rings
open at once), --spellings random spellings of each, and every row with an `n` once more without an [nH] token, and
compares every line with SmilesScaffolds.scaffold.  Exit status 1 for a sanitizer report or a row that differs."""
import argparse
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.molkey import as_int64  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402
from gct_plus_amd.scaffold import SmilesScaffolds  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spellings", type=int, default=4)
ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
a = ap.parse_args()

PATTERN = re.compile(r"(\[[^\]]+]|Br?|Cl?|N|O|S|P|F|I|b|c|n|o|s|p|\(|\)|\.|=|#|-|\+|\\|\/|:|~|@|\?|>|\*|\$|\%[0-9]{2}|[0-9])")
V = synthetic.CHEM_VOCAB
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

sc = SmilesScaffolds(V, synthetic.PAD_ID, synthetic.EOS_ID)
no_nh = SmilesScaffolds(V, synthetic.PAD_ID, synthetic.EOS_ID)
no_nh.nh_id = None
assert sc.n_id is not None and sc.nh_id is not None, "synthetic.CHEM_VOCAB spells n and [nH]"
ks, rz = sc.keys, sc.randomizer
cases = []                                                        # (tokens, the statement to compare with, room)
for s in ROWS:
    toks = [V.index(t) for t in PATTERN.findall(s)]
    spelt = [toks]
    for k in range(a.spellings):
        status, new, _ = rz.randomize(toks, stream(7, k, 0), 1.0, 255)
        if status == ops.RAND_OK:
            spelt.append(new)
    for t in spelt:
        cases.append((t, sc, 255))
        if sc.n_id in t:
            cases.append((t, no_nh, 255))
    cases.append((toks, sc, max(len(toks) - 2, 0)))               # TOO_LONG for a row that is all scaffold

build = os.path.join(ROOT, "tools", "_build")
os.makedirs(build, exist_ok=True)
exe, path = os.path.join(build, "scaffold_walk_host"), os.path.join(build, "scaffold_walk_cases.txt")
san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
cmd = [a.hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result"]
cmd += [x for f in san for x in ("-Xarch_host", f)] + ["-fsanitize=address,undefined"]
subprocess.run(cmd + [os.path.join(ROOT, "tools", "scaffold_walk_host.hip"), "-o", exe], check=True)
with open(path, "w") as f:
    f.write(f"{len(cases)}\n")
    for toks, st, room in cases:
        nh = -1 if st.nh_id is None else st.nh_id
        f.write(f"{len(toks)} {len(rz.ring_ids)} {rz.open_id} {rz.close_id} {room} {nh} {ks.words[nh] if nh >= 0 else 0}\n")
        f.write(f"{ks.labels[nh] if nh >= 0 else 0}\n")
        f.write(" ".join(str(ks.words[t] & 0xFFFFFF | (t == sc.n_id) << 25) for t in toks) + "\n")
        f.write(" ".join(str(ks.labels[t]) for t in toks) + "\n")
        f.write(" ".join(str(r) for r in rz.ring_ids) + "\n")
run = subprocess.run([exe, path], capture_output=True, text=True)
if run.returncode != 0:
    print(run.stderr[-4000:])
    sys.exit(f"scaffold_walk_check: the harness ended with status {run.returncode}")
lines = run.stdout.strip("\n").split("\n")
assert len(lines) == len(cases), (len(lines), len(cases))
bad, seen = 0, collections.Counter()
for (toks, st, room), line in zip(cases, lines):
    status, spelt, member, key = st.scaffold(toks, room)
    seen[status] += 1
    head, row, mem = (part.split() for part in line.split("|"))
    got_row = [int(v) if int(v) >= 0 else toks[-int(v) - 1] for v in row]
    got = [int(head[0]), as_int64(int(head[1])), int(head[2]), int(head[3]), got_row, [int(m) for m in mem]]
    if got != [status, key, sum(1 for m in member if m), len(spelt), spelt, member]:
        bad += 1
        print("differs:", "".join(V[t] for t in toks)[:60], "->", line[:100], "want", status, key, len(spelt))
names = {getattr(ops, n): n[4:] for n in ("SCA_OK", "SCA_ACYCLIC", "SCA_SYNTAX", "SCA_UNSUPPORTED", "SCA_NO_TOKEN",
                                          "SCA_NO_RING", "SCA_TOO_LONG")}
print(f"scaffold_walk_check: {len(cases)} parts under ASan + UBSan, {bad} differ from the host statement; "
      + ", ".join(f"{names[s]} {c}" for s, c in sorted(seen.items())))
sys.exit(1 if bad else 0)
