#!/usr/bin/env python3
"""What Murcko scaffolds cost (recorded in the README and DESIGN, not gated): gct_smiles_scaffold on --rows rows of 80
columns of molecules over synthetic.CHEM_VOCAB (molkey_bench.py's list, every molecule in a random spelling, every row
behind a 4-token prefix) against
  * gct_smiles_key on the same rows (the launch does the key's work on the kept atoms, and the parse, the peel, the
    compaction and the randomiser's walk on one lane beside it),
  * a device copy of the same tokens (rows x 80 x 8 bytes: the floor of anything that reads them once), and
  * the host statement SmilesScaffolds.scaffold_reference on --host-rows of them, scaled to the batch,
alternated three times in one process; the launch's four tensors are compared with the host statement's.
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
ap.add_argument("--host-rows", type=int, default=2048, help="rows the host statement is timed on")
ap.add_argument("--iters", type=int, default=50, help="launches per timed leg")
ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows),
           "--host-rows", str(a.host_rows), "--iters", str(a.iters)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"scaffold_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402
from gct_plus_amd.scaffold import SmilesScaffolds  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O",
             "C12CC1C2", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0 = synthetic.CHEM_VOCAB, 80, 4
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
sc = SmilesScaffolds(V, PAD, EOS)
ks, rz = sc.keys, sc.randomizer
rng = random.Random(1)
mols = [[V.index(t) for t in tokenize(s)] for s in MOLECULES]
spellings = []                                                  # 16 spellings of every molecule, made on the host once
for m, ids in enumerate(mols):
    got = [rz.randomize(ids, stream(3, k | m << 32, 0), 1.0, W - T0 - 1) for k in range(16)]
    spellings.append([new for status, new, _ in got if status == ops.RAND_OK] + [ids])
ys = torch.full((a.rows, W), PAD)
ys[:, :T0] = torch.randint(5, len(V), (a.rows, T0), generator=torch.Generator().manual_seed(1))
for r in range(a.rows):
    ids = rng.choice(spellings[rng.randrange(len(mols))])
    ys[r, T0:T0 + len(ids) + 1] = torch.tensor(ids + [EOS])
dev = ys.cuda()
start = torch.full((a.rows,), T0, dtype=torch.int32, device="cuda")
table, labels = ks.device_tables("cuda")
ring_ids = rz.device_tables("cuda")[1]
none = lambda v: -1 if v is None else v                                           # noqa: E731
key_outs = (torch.empty(a.rows, 2, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"))
outs = (torch.empty(a.rows, W, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 2, dtype=torch.int64, device="cuda"),
        torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"), torch.empty(a.rows, W, dtype=torch.int32, device="cuda"))
copy = torch.empty_like(dev)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def launch():
    ops.smiles_scaffold(dev, start, table, labels, ring_ids, len(rz.ring_ids), rz.open_id, rz.close_id, PAD, EOS, -1,
                        none(sc.n_id), none(sc.nh_id), W, out=outs)


def host_statement():
    t0 = time.perf_counter()
    got = sc.scaffold_reference(ys[:a.host_rows], [T0] * a.host_rows)
    return got, (time.perf_counter() - t0) * 1e3 * a.rows / a.host_rows


kern, keys, floor, host = [], [], [], []
for _ in range(3):
    kern.append(timed(launch, a.iters))
    keys.append(timed(lambda: ops.smiles_key(dev, start, table, labels, PAD, EOS, -1, out=key_outs), a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    ref, ms = host_statement()
    host.append(ms)
wrong = int(sum((o[:a.host_rows].cpu() != r).any(1).sum() for o, r in zip(outs, ref)))
info = outs[2].cpu()
med = lambda v: sorted(v)[1]                                                      # noqa: E731
print(f"scaffold_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens); rows with a scaffold "
      f"{float((info[:, 0] == ops.SCA_OK).float().mean()):.3f}, acyclic {float((info[:, 0] == ops.SCA_ACYCLIC).float().mean()):.3f}, "
      f"mean atoms kept {float(info[:, 2].float().mean()):.1f}; rows that differ from the host statement (of {a.host_rows}): "
      f"{wrong}")
print(f"  gct_smiles_scaffold {med(kern):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in kern)})")
print(f"  gct_smiles_key      {med(keys):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in keys)}), "
      f"the scaffolds are {med(kern) / med(keys):.2f} x it")
print(f"  device copy (floor) {med(floor):9.1f} us per copy    (three legs: {', '.join(f'{x:.1f}' for x in floor)})")
print(f"  host statement      {med(host) * 1e3:9.1f} us per batch   (three legs: {', '.join(f'{x * 1e3:.0f}' for x in host)}, "
      f"scaled from {a.host_rows} rows), {med(host) * 1e3 / med(kern):.0f} x the launch")
sys.exit(1 if wrong else 0)
