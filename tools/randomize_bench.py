#!/usr/bin/env python3
"""What SMILES randomisation costs (recorded in the README and DESIGN, not gated): gct_smiles_randomize at p = 1 on
--rows rows of 80 columns of molecules over synthetic.CHEM_VOCAB (chem_bench.py's list without its stereo and dotted
rows; every row behind a 4-token prefix, out_width 96) against
  * a device copy of the same tokens (rows x 80 x 8 bytes: the floor of anything that reads them once),
  * gct_smiles_check on the same rows (one walk of each row by one lane; the randomiser makes three), and
  * the host statement SmilesRandomizer.randomize_reference on --host-rows of them, scaled to the batch,
alternated three times in one process; the launch's rows are compared with the host statement's.
--loader N adds a second measurement: one pass over a data.SmilesLoader of N synthetic SMILES (bench.py's frame) on the
device with randomize_prob 0 against 0.5, batches of 256, alternated three times -- the loader alone, no model step;
--epoch a third: Train.trainer1.run_epoch of a full-size vaetf (synthetic weights, batches of 512) behind the same two
loaders, ms per step, alternated three times.
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
ap.add_argument("--loader", type=int, default=0, help="also time a SmilesLoader pass over this many synthetic SMILES")
ap.add_argument("--epoch", action="store_true", help="with --loader: also time run_epoch of a full-size vaetf behind it")
ap.add_argument("--limit", type=int, default=300, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows),
           "--host-rows", str(a.host_rows), "--iters", str(a.iters), "--loader", str(a.loader)]
    cmd += ["--epoch"] if a.epoch else []
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"randomize_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import data, ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.smiles import SmilesChemistry  # noqa: E402
from gct_plus_amd.randomize import SmilesRandomizer  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O",
             "C12CC1C2", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0, OUT = synthetic.CHEM_VOCAB, 80, 4, 96
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
rz, chem = SmilesRandomizer(V, PAD, EOS), SmilesChemistry(V, PAD, EOS)
rng = random.Random(1)
mols = [[V.index(t) for t in tokenize(s)] for s in MOLECULES]
ys = torch.full((a.rows, W), PAD)
ys[:, :T0] = torch.randint(5, len(V), (a.rows, T0), generator=torch.Generator().manual_seed(1))   # a prefix: copied
for r in range(a.rows):
    ids = rng.choice(mols)
    ys[r, T0:T0 + len(ids) + 1] = torch.tensor(ids + [EOS])
dev = ys.cuda()
start = torch.full((a.rows,), T0, dtype=torch.int32, device="cuda")
key = torch.arange(a.rows, dtype=torch.int64, device="cuda")
table, ring_ids = rz.device_tables("cuda")
ctable, cwords = chem.device_tables("cuda")
outs = (torch.empty(a.rows, OUT, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"),
        None)
report = torch.empty(a.rows, 4, dtype=torch.int32, device="cuda")
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
    ops.smiles_randomize(dev, start, key, table, ring_ids, len(rz.ring_ids), rz.open_id, rz.close_id, PAD, EOS, -1, 7, 1.0,
                         OUT, out=outs)


def host_statement():
    t0 = time.perf_counter()
    got = rz.randomize_reference(ys[:a.host_rows], [T0] * a.host_rows, key[:a.host_rows].cpu(), 7, 1.0, OUT,
                                 return_perm=False)
    return got, (time.perf_counter() - t0) * 1e3 * a.rows / a.host_rows


kern, floor, check, host = [], [], [], []
for _ in range(3):
    kern.append(timed(launch, a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    check.append(timed(lambda: ops.smiles_check(dev, start, ctable, cwords, out=report), a.iters))
    ref, ms = host_statement()
    host.append(ms)
wrong = int((outs[0][:a.host_rows].cpu() != ref.tokens).any(1).sum() + (outs[1][:a.host_rows].cpu() != ref.info).any(1).sum())
info = outs[1].cpu()
med = lambda v: sorted(v)[1]                                                      # noqa: E731
print(f"randomize_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens) -> {OUT}; randomised "
      f"{float((info[:, 0] == ops.RAND_OK).float().mean()):.3f}, mean new length {float(info[:, 2].float().mean()):.1f}; "
      f"rows that differ from the host statement (of {a.host_rows}): {wrong}")
print(f"  gct_smiles_randomize {med(kern):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in kern)})")
print(f"  device copy (floor)  {med(floor):9.1f} us per copy    (three legs: {', '.join(f'{x:.1f}' for x in floor)})")
print(f"  gct_smiles_check     {med(check):9.1f} us per launch  (three legs: {', '.join(f'{x:.1f}' for x in check)}), "
      f"the randomiser is {med(kern) / med(check):.1f} x it")
print(f"  host statement       {med(host) * 1e3:9.1f} us per batch   (three legs: {', '.join(f'{x * 1e3:.0f}' for x in host)}, "
      f"scaled from {a.host_rows} rows), {med(host) * 1e3 / med(kern):.0f} x the launch")

if a.loader:
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_frame", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    frame = bench.synthetic_smiles_frame(a.loader, seed=3)
    col = frame["src"].tolist()
    SRC, TRG = data.Vocab.build(col, False, False), data.Vocab.build(col, True, False)

    def one_pass(p, epoch):
        ld = data.SmilesLoader(frame, SRC, TRG, "vaetf", [], 256, 0, 1, True, 0, torch.device("cuda"), randomize_prob=p)
        ld.set_epoch(epoch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(b["trg"].shape[0] for b in ld)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, n

    one_pass(0.5, 0)
    legs = {0.0: [], 0.5: []}
    for e in range(3):
        for p in legs:
            ms, n = one_pass(p, e + 1)
            legs[p].append(ms)
    print(f"  SmilesLoader pass over {n} synthetic SMILES, batches of 256 on the device: randomize_prob 0 "
          f"{med(legs[0.0]):.1f} ms ({', '.join(f'{x:.1f}' for x in legs[0.0])}), 0.5 {med(legs[0.5]):.1f} ms "
          f"({', '.join(f'{x:.1f}' for x in legs[0.5])})")

    if a.epoch:                         # Train.trainer1.run_epoch of a full-size vaetf behind the same two loaders
        import logging
        import types
        from gct_plus_amd.Model import model_dict
        from gct_plus_amd.Train.trainer1 import run_epoch
        from gct_plus_amd.optim import FusedAdam
        LOG = logging.getLogger("randomize_bench")
        LOG.propagate = False
        LOG.addHandler(logging.NullHandler())
        args = types.SimpleNamespace(model_type="vaetf", pad_id=synthetic.PAD_ID, use_cond2dec=False, property_list=[],
                                     lr_scheduler="WarmUpDefault", lr_WarmUpSteps=8000, d_model=512, print_every=1)
        torch.manual_seed(1)
        model = model_dict["vaetf"](len(SRC), len(TRG), dropout=0.1, nconds=0, use_cond2lat=False, N=6, d_model=512,
                                    dff=2048, h=8, latent_dim=128).cuda().train()
        opt = FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.98), eps=1e-9, model=model)
        B, cur = 512, 100000

        def epoch(p, e, rows=None):
            ld = data.SmilesLoader(frame if rows is None else frame.iloc[:rows], SRC, TRG, "vaetf", [], B, 0, 1, False, 0,
                                   torch.device("cuda"), randomize_prob=p)
            ld.set_epoch(e)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step = run_epoch(args, model, opt, ld, cur, 0.04, LOG, train=True)[1]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / len(ld), step

        for p in (0.0, 0.5):
            _, cur = epoch(p, 0, rows=3 * B)                                       # warm-up: shapes, workspaces
        legs = {0.0: [], 0.5: []}
        for e in range(3):
            for p in legs:
                ms, cur = epoch(p, e + 1)
                legs[p].append(ms)
        print(f"  run_epoch, full-size vaetf, {a.loader // B} steps of {B} behind the loader: randomize_prob 0 "
              f"{med(legs[0.0]):.2f} ms per step ({', '.join(f'{x:.2f}' for x in legs[0.0])}), 0.5 {med(legs[0.5]):.2f} "
              f"({', '.join(f'{x:.2f}' for x in legs[0.5])})")
sys.exit(1 if wrong else 0)
