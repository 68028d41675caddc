#!/usr/bin/env python3
"""The sequential walks of gct_smiles_randomize on the CPU under AddressSanitizer and UBSan (no GPU needed): builds
tools/randomize_walk_host.hip -- a stand-alone program around rand_parse / rand_walk of csrc/randomize.hip, the host
code sanitised -- into tools/_build/, feeds it molecules, kept rows and the rows that fill the kernel's LDS record to
its ends (a chain of 252, branch depth 83, 84 branches on one atom, atoms with 8 and 9 bonds, 40 rings open at once, 255
atoms) under --keys keys each with mixed room, and compares every line with SmilesRandomizer.randomize.  Exit status 1
for a sanitizer report or a row that differs."""
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
from gct_plus_amd.randomize import SmilesRandomizer, stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=40)
ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
a = ap.parse_args()

PATTERN = re.compile(r"(\[[^\]]+]|Br?|Cl?|N|O|S|P|F|I|b|c|n|o|s|p|\(|\)|\.|=|#|-|\+|\\|\/|:|~|@|\?|>|\*|\$|\%[0-9]{2}|[0-9])")
V = synthetic.CHEM_VOCAB
RING = [str(k) if k < 10 else f"%{k}" for k in range(40)]
ROWS = ["CCO", "c1ccccc1-c1ccccc1", "C12C3C4C1C5C2C3C45", "C1CCC2(CC1)CCCC2", "c1cc[nH]c1", "C=1CCCCC1", "C/C=C/C", "C1C1",
        "C.C", "C[C@@H](N)O", "C(", "C1CC", "", "C?C", "C=1CC#1", "C#N", "C%12CC%12", "C%64C%64", "C1CC11CC11CC1",
        "CCN1CCCC2(CCN(C(=O)c3cc(C)nc4ccccc34)C2)C1=O", "n1c2c(c(N)nc1N)c(C)c(Cc1cc(OC)ccc1OC)cn2",
        "C" * 252, "C" * 255, "C" + "(C" * 83 + ")" * 83, "C" + "(C)" * 84, "S" + "(C)" * 7 + "C", "S" + "(C)" * 8 + "C",
        "S" + "(S(C)(C)C)" * 7 + "C", "".join("C" + r for r in RING) * 2]
SMALL = ["<unk>", "<pad>", "<sos>", "<eos>", "C", "0", "1", "2", "(", ")"]          # two usable ring numbers: NO_RING

cases = []
for vocab, rows in ((V, ROWS), (SMALL, ["C01C2C0C12", "C1CC11CC11CC1", "C1CC1"])):
    rz = SmilesRandomizer(vocab, 1, 3)
    for s in rows:
        toks = [vocab.index(t) for t in PATTERN.findall(s)]
        for k in range(a.keys):
            cases.append((rz, toks, k, min(256, random.Random(k).choice([256, 255, len(toks), len(toks) + 1, len(toks) + 2]))))

build = os.path.join(ROOT, "tools", "_build")
os.makedirs(build, exist_ok=True)
exe, path = os.path.join(build, "randomize_walk_host"), os.path.join(build, "randomize_walk_cases.txt")
san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
cmd = [a.hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result"]
cmd += [x for f in san for x in ("-Xarch_host", f)] + ["-fsanitize=address,undefined"]
subprocess.run(cmd + [os.path.join(ROOT, "tools", "randomize_walk_host.hip"), "-o", exe], check=True)
with open(path, "w") as f:
    f.write(f"{len(cases)}\n")
    for rz, toks, k, room in cases:
        words, calls = stream(7, k, 0), 1 + 2 * (len(toks) + 1)
        f.write(f"{len(toks)} {calls} {len(rz.ring_ids)} {rz.open_id} {rz.close_id} {room}\n")
        f.write(" ".join(str(rz.words[t]) for t in toks) + "\n")
        f.write(" ".join(str(w) for c in range(calls) for w in words(c)) + "\n")
        f.write(" ".join(map(str, rz.ring_ids)) + "\n")
run = subprocess.run([exe, path], capture_output=True, text=True)
if run.returncode != 0:
    print(run.stderr[-4000:])
    sys.exit(f"randomize_walk_check: the harness ended with status {run.returncode}")
lines = run.stdout.strip().split("\n")
assert len(lines) == len(cases), (len(lines), len(cases))
bad, seen = 0, collections.Counter()
for (rz, toks, k, room), line in zip(cases, lines):
    status, new, perm = rz.randomize(toks, stream(7, k, 0), 1.0, room)
    seen[status] += 1
    got = line.split()
    same = int(got[0]) == status
    if same and status == ops.RAND_OK:
        n = int(got[1])
        entries = [int(x) for x in got[2:2 + n]]
        same = [e if e >= 0 else toks[-e - 1] for e in entries] == new and [int(x) for x in got[3 + n:]] == perm
    if not same:
        bad += 1
        print("differs:", "".join(rz.grammar.itos[t] for t in toks)[:60], "key", k, "room", room, "->", line[:80])
names = {getattr(ops, n): n[5:] for n in dir(ops) if n.startswith("RAND_") and n not in ("RAND_MAX_SPAN",)}
print(f"randomize_walk_check: {len(cases)} parts under ASan + UBSan, {bad} differ from the host statement; "
      + ", ".join(f"{names[s]} {c}" for s, c in sorted(seen.items())))
sys.exit(1 if bad else 0)
