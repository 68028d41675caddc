#!/usr/bin/env python3
"""What the chemistry check costs (recorded in the README and DESIGN, not gated): gct_smiles_check on --rows rows of 80
columns over synthetic.CHEM_VOCAB -- common molecules, most of them with one token replaced by a random one, so that
about a quarter of the rows are valid and every status occurs -- against
  * a device copy of the same tokens (rows x 80 x 8 bytes: the floor of anything that reads them once), and
  * the host loop [chem.check(r) for r in ys.cpu().tolist()] that the launch replaces in a fine-tuning round,
alternated three times in one process; the launch's report is compared with the host loop's, row by row.
The measurement runs in a child process under `timeout` (a GPU step that hangs ends there)."""
import argparse
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=32768)
ap.add_argument("--iters", type=int, default=50, help="launches per timed leg")
ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows),
           "--iters", str(a.iters)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"chem_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.smiles import SmilesChemistry  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O", "ClC(Cl)Cl.CO",
             "C12CC1C2", "N[C@@H](C)C(=O)O", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0 = synthetic.CHEM_VOCAB, 80, 4
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
chem = SmilesChemistry(V, PAD, EOS)
rng = random.Random(1)
mols = [[V.index(t) for t in tokenize(s)] for s in MOLECULES]
ys = torch.full((a.rows, W), PAD)
ys[:, :T0] = torch.randint(5, len(V), (a.rows, T0), generator=torch.Generator().manual_seed(1))   # a prefix: not read
for r in range(a.rows):
    ids = list(rng.choice(mols))
    if rng.random() < 0.87:
        ids[rng.randrange(len(ids))] = rng.randrange(5, len(V))
    ys[r, T0:T0 + len(ids) + 1] = torch.tensor(ids + [EOS])
dev = ys.cuda()
start = torch.full((a.rows,), T0, dtype=torch.int32, device="cuda")
table, words = chem.device_tables("cuda")
out = torch.empty(a.rows, 4, dtype=torch.int32, device="cuda")
copy = torch.empty_like(dev)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def host_loop():
    t0 = time.perf_counter()
    got = [chem.check(r[T0:]) for r in dev.cpu().tolist()]
    return got, (time.perf_counter() - t0) * 1e3


kern, floor, host = [], [], []
for _ in range(3):
    kern.append(timed(lambda: ops.smiles_check(dev, start, table, words, out=out), a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    ref, ms = host_loop()
    host.append(ms)
ref = torch.tensor(ref, dtype=torch.int32)
wrong = int((out.cpu() != ref).any(1).sum())
share = {name: float((ref[:, 0] == code).float().mean()) for name, code in (
    ("ok", ops.CHEM_OK), ("syntax", ops.CHEM_SYNTAX), ("valence", ops.CHEM_VALENCE), ("ring_bond", ops.CHEM_RING_BOND),
    ("aromatic", ops.CHEM_AROMATIC))}
med = lambda v: sorted(v)[1]                                                      # noqa: E731
print(f"chem_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens), spans of {W - T0}; statuses "
      + ", ".join(f"{k} {v:.3f}" for k, v in share.items()) + f"; rows that differ from the host loop: {wrong}")
print(f"  gct_smiles_check     {med(kern):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in kern)})")
print(f"  device copy (floor)  {med(floor):9.1f} us per copy    (three legs: {', '.join(f'{x:.1f}' for x in floor)})")
print(f"  host loop            {med(host) * 1e3:9.1f} us per batch   (three legs: {', '.join(f'{x * 1e3:.0f}' for x in host)}), "
      f"{med(host) * 1e3 / med(kern):.0f} x the launch")
sys.exit(1 if wrong else 0)
