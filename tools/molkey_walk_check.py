#!/usr/bin/env python3
"""The host-callable parts of gct_smiles_key on the CPU under AddressSanitizer and UBSan (no GPU needed): builds
tools/molkey_walk_host.hip -- a stand-alone program around rand_parse (csrc/smiles_graph.h) and the per-atom and
sequential parts of csrc/molkey.hip, the host code sanitised -- into tools/_build/, feeds it tools/randomize_walk_check.py's
rows (molecules, kept rows and the rows that fill the kernel's LDS record to its ends: chains of 252 and 255, branch depth
83, 84 branches on one atom, atoms with 8 and 9 bonds, 40 rings open at once) and --spellings random spellings of each,
and compares every line with SmilesKeys.key.  Exit status 1 for a sanitizer report or a row that differs."""
import argparse
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.molkey import SmilesKeys, as_int64  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402

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
        "C" * 252, "C" * 255, "C" + "(C" * 83 + ")" * 83, "C" + "(C)" * 84, "S" + "(C)" * 7 + "C", "S" + "(C)" * 8 + "C",
        "S" + "(S(C)(C)C)" * 7 + "C", "".join("C" + r for r in RING) * 2]

keys = SmilesKeys(V, synthetic.PAD_ID, synthetic.EOS_ID)
cases = []
for s in ROWS:
    toks = [V.index(t) for t in PATTERN.findall(s)]
    cases.append(toks)
    for k in range(a.spellings):
        status, new, _ = keys.randomizer.randomize(toks, stream(7, k, 0), 1.0, 255)
        if status == ops.RAND_OK:
            cases.append(new)

build = os.path.join(ROOT, "tools", "_build")
os.makedirs(build, exist_ok=True)
exe, path = os.path.join(build, "molkey_walk_host"), os.path.join(build, "molkey_walk_cases.txt")
san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
cmd = [a.hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result"]
cmd += [x for f in san for x in ("-Xarch_host", f)] + ["-fsanitize=address,undefined"]
subprocess.run(cmd + [os.path.join(ROOT, "tools", "molkey_walk_host.hip"), "-o", exe], check=True)
with open(path, "w") as f:
    f.write(f"{len(cases)}\n")
    for toks in cases:
        f.write(f"{len(toks)}\n")
        f.write(" ".join(str(keys.words[t]) for t in toks) + "\n")
        f.write(" ".join(str(keys.labels[t]) for t in toks) + "\n")
run = subprocess.run([exe, path], capture_output=True, text=True)
if run.returncode != 0:
    print(run.stderr[-4000:])
    sys.exit(f"molkey_walk_check: the harness ended with status {run.returncode}")
lines = run.stdout.strip().split("\n")
assert len(lines) == len(cases), (len(lines), len(cases))
bad, seen = 0, collections.Counter()
for toks, line in zip(cases, lines):
    status, key, atoms, bonds = keys._part(toks)
    seen[status] += 1
    got = line.split()
    if [int(got[0]), as_int64(int(got[1])), int(got[2]), int(got[3])] != [status, as_int64(key), atoms, bonds]:
        bad += 1
        print("differs:", "".join(V[t] for t in toks)[:60], "->", line[:80], "want", status, key, atoms, bonds)
names = {getattr(ops, n): n[4:] for n in ("KEY_GRAPH", "KEY_STRING_SYNTAX", "KEY_STRING_UNSUPPORTED")}
print(f"molkey_walk_check: {len(cases)} parts under ASan + UBSan, {bad} differ from the host statement; "
      + ", ".join(f"{names[s]} {c}" for s, c in sorted(seen.items())))
sys.exit(1 if bad else 0)
