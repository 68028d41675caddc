#!/usr/bin/env python3
"""What molecule keys cost (recorded in the README and DESIGN, not gated): gct_smiles_key on --rows rows of 80 columns of
molecules over synthetic.CHEM_VOCAB (randomize_bench.py's list, every molecule in a random spelling, every row behind a
4-token prefix) against
  * a device copy of the same tokens (rows x 80 x 8 bytes: the floor of anything that reads them once),
  * gct_smiles_check on the same rows (one sequential walk of each row by one lane), and
  * the host statement SmilesKeys.key_reference on --host-rows of them, scaled to the batch,
alternated three times in one process; the launch's keys are compared with the host statement's.  Then the metrics end to
end: molkey.basic_metrics of (gct_smiles_check, gct_smiles_key) with an index of half the molecules -- sorts and a
search on the device, one read-back -- against what it replaces: the rows copied to the host and a Python set of tuples
(which counts distinct STRINGS; the two distinct counts are printed side by side).
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
        print(f"molkey_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.smiles import ChemReport, SmilesChemistry  # noqa: E402
from gct_plus_amd.molkey import MolKeyIndex, MolKeys, SmilesKeys, basic_metrics  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O",
             "C12CC1C2", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0 = synthetic.CHEM_VOCAB, 80, 4
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
ks, chem = SmilesKeys(V, PAD, EOS), SmilesChemistry(V, PAD, EOS)
rng = random.Random(1)
mols = [[V.index(t) for t in tokenize(s)] for s in MOLECULES]
spellings = []                                                  # 16 spellings of every molecule, made on the host once
for m, ids in enumerate(mols):
    got = [ks.randomizer.randomize(ids, stream(3, k | m << 32, 0), 1.0, W - T0 - 1) for k in range(16)]
    spellings.append([new for status, new, _ in got if status == ops.RAND_OK] + [ids])
ys = torch.full((a.rows, W), PAD)
ys[:, :T0] = torch.randint(5, len(V), (a.rows, T0), generator=torch.Generator().manual_seed(1))
which = [rng.randrange(len(mols)) for _ in range(a.rows)]
for r in range(a.rows):
    ids = rng.choice(spellings[which[r]])
    ys[r, T0:T0 + len(ids) + 1] = torch.tensor(ids + [EOS])
dev = ys.cuda()
start = torch.full((a.rows,), T0, dtype=torch.int32, device="cuda")
table, labels = ks.device_tables("cuda")
ctable, cwords = chem.device_tables("cuda")
outs = (torch.empty(a.rows, 2, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"))
report = torch.empty(a.rows, 4, dtype=torch.int32, device="cuda")
copy = torch.empty_like(dev)
index = MolKeyIndex(torch.tensor([ks.key(ids)[1] for ids in mols[::2]]))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def launch():
    ops.smiles_key(dev, start, table, labels, PAD, EOS, -1, out=outs)


def host_statement():
    t0 = time.perf_counter()
    got = ks.key_reference(ys[:a.host_rows], [T0] * a.host_rows)
    return got, (time.perf_counter() - t0) * 1e3 * a.rows / a.host_rows


def metrics_on_the_device():
    ops.smiles_check(dev, start, ctable, cwords, out=report)
    launch()
    return basic_metrics(ChemReport(*report.unbind(1)), MolKeys(*outs), index)


def metrics_on_the_host():
    """Copy to host, set of tuples: valid through the device report, distinct STRINGS among the valid rows."""
    ops.smiles_check(dev, start, ctable, cwords, out=report)
    ok = (report[:, 0] == ops.CHEM_OK).cpu().tolist()
    rows = dev[:, T0:].cpu().tolist()
    return sum(ok), len({tuple(t for t in r if t != PAD) for r, v in zip(rows, ok) if v})


kern, floor, check, host, dev_ms, host_ms = [], [], [], [], [], []
for _ in range(3):
    kern.append(timed(launch, a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    check.append(timed(lambda: ops.smiles_check(dev, start, ctable, cwords, out=report), a.iters))
    ref, ms = host_statement()
    host.append(ms)
    dev_ms.append(timed(metrics_on_the_device, 5) / 1e3)
    host_ms.append(timed(metrics_on_the_host, 1) / 1e3)
wrong = int((outs[0][:a.host_rows].cpu() != ref.key).any(1).sum() + (outs[1][:a.host_rows].cpu() != ref.info).any(1).sum())
info = outs[1].cpu()
got, (n_valid, strings) = metrics_on_the_device(), metrics_on_the_host()
written = len({m for m, v in zip(which, (report[:, 0] == ops.CHEM_OK).cpu().tolist()) if v})
med = lambda v: sorted(v)[1]                                                      # noqa: E731
print(f"molkey_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens); graph keys "
      f"{float((info[:, 0] == ops.KEY_GRAPH).float().mean()):.3f}, mean atoms {float(info[:, 2].float().mean()):.1f}; rows "
      f"that differ from the host statement (of {a.host_rows}): {wrong}")
print(f"  gct_smiles_key      {med(kern):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in kern)})")
print(f"  device copy (floor) {med(floor):9.1f} us per copy    (three legs: {', '.join(f'{x:.1f}' for x in floor)})")
print(f"  gct_smiles_check    {med(check):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in check)}), "
      f"the keys are {med(kern) / med(check):.1f} x it")
print(f"  host statement      {med(host) * 1e3:9.1f} us per batch   (three legs: {', '.join(f'{x * 1e3:.0f}' for x in host)}, "
      f"scaled from {a.host_rows} rows), {med(host) * 1e3 / med(kern):.0f} x the launch")
print(f"  basic_metrics end to end (check + keys + sorts + search, one read-back) {med(dev_ms):.2f} ms "
      f"({', '.join(f'{x:.2f}' for x in dev_ms)}); copy to host + set of tuples {med(host_ms):.1f} ms "
      f"({', '.join(f'{x:.1f}' for x in host_ms)}), {med(host_ms) / med(dev_ms):.0f} x")
print(f"  {got}; the set of tuples: {n_valid} valid rows, {strings} distinct strings for {got['n_unique']} distinct "
      f"molecules ({written} were written in valid rows)")
sys.exit(1 if wrong or got["n_unique"] != written or got["n_valid"] != n_valid else 0)
