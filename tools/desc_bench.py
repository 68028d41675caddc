#!/usr/bin/env python3
"""What molecular descriptors cost (recorded in the README and DESIGN, not gated): gct_smiles_desc on --rows rows of 80
columns of molecules over synthetic.CHEM_VOCAB (fp_bench.py's rows: every molecule in a random spelling, every row
behind a 4-token prefix) against gct_smiles_key on the same rows (the yardstick), a device copy of the tokens (the floor
of anything that reads them once) and the host statement desc_reference on --host-rows of them, scaled to the batch;
the launch's integers are compared with the host statement's.  Every comparison is alternated three times in one process,
the median is reported.  The measurement runs in a child process under `timeout` (a GPU step that hangs ends there)."""
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
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("rows", "host_rows", "iters"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"desc_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.descriptor import SmilesDescriptors  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O",
             "C12CC1C2", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0 = synthetic.CHEM_VOCAB, 80, 4
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
ds = SmilesDescriptors(V, PAD, EOS)
ks = ds.keys
rng = random.Random(1)
mols = [[V.index(t) for t in tokenize(s)] for s in MOLECULES]
spellings = []                                                  # 16 spellings of every molecule, made on the host once
for m, ids in enumerate(mols):
    got = [ks.randomizer.randomize(ids, stream(3, k | m << 32, 0), 1.0, W - T0 - 1) for k in range(16)]
    spellings.append([new for status, new, _ in got if status == ops.RAND_OK] + [ids])
ys = torch.full((a.rows, W), PAD)
ys[:, :T0] = torch.randint(5, len(V), (a.rows, T0), generator=torch.Generator().manual_seed(1))
for r in range(a.rows):
    ids = rng.choice(spellings[rng.randrange(len(mols))])
    ys[r, T0:T0 + len(ids) + 1] = torch.tensor(ids + [EOS])
dev = ys.cuda()
start = torch.full((a.rows,), T0, dtype=torch.int32, device="cuda")
table, labels = ks.device_tables("cuda")
_, desc = ds.device_tables("cuda")
values = torch.empty(a.rows, ops.DESC_COLUMNS, dtype=torch.int32, device="cuda")
key_outs = (torch.empty(a.rows, 2, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"))
copy = torch.empty_like(dev)
med = lambda v: sorted(v)[1]                                                      # noqa: E731
legs = lambda v, f=".1f": ", ".join(format(x, f) for x in v)                      # noqa: E731


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def host_statement():
    t0 = time.perf_counter()
    got = ds.desc_reference(ys[:a.host_rows], [T0] * a.host_rows)
    return got, (time.perf_counter() - t0) * 1e3 * a.rows / a.host_rows


kern, keys, floor, host = [], [], [], []
for _ in range(3):
    kern.append(timed(lambda: ops.smiles_desc(dev, start, table, desc, PAD, EOS, -1, out=values), a.iters))
    keys.append(timed(lambda: ops.smiles_key(dev, start, table, labels, PAD, EOS, -1, out=key_outs), a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    ref, ms = host_statement()
    host.append(ms)
got = values.cpu()
wrong = int((got[:a.host_rows] != ref.values).any(1).sum())
ok = got[:, 0] == ops.DESC_OK
print(f"desc_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens); rows that are DESC_OK "
      f"{float(ok.float().mean()):.3f}, mean heavy atoms {float(got[ok, 1].float().mean()):.1f}, mean TPSA "
      f"{float(got[ok, 10].float().mean()) / 100:.2f}; rows that differ from the host statement (of {a.host_rows}): {wrong}")
print(f"  gct_smiles_desc     {med(kern):9.1f} us per launch  (three legs: {legs(kern)})")
print(f"  gct_smiles_key      {med(keys):9.1f} us per launch  (three legs: {legs(keys)}), the descriptors are "
      f"{med(kern) / med(keys):.2f} x it")
print(f"  device copy (floor) {med(floor):9.1f} us per copy    (three legs: {legs(floor)})")
print(f"  host statement      {med(host) * 1e3:9.1f} us per batch   (three legs: {legs([x * 1e3 for x in host], '.0f')}, scaled "
      f"from {a.host_rows} rows), {med(host) * 1e3 / med(kern):.0f} x the launch", flush=True)
sys.exit(1 if wrong else 0)
