#!/usr/bin/env python3
"""What fingerprints and Tanimoto aggregates cost (recorded in the README and DESIGN, not gated).
  1. gct_smiles_fp on --rows rows of 80 columns of molecules over synthetic.CHEM_VOCAB (molkey_bench.py's rows: every
     molecule in a random spelling, every row behind a 4-token prefix) against gct_smiles_key on the same rows, a device
     copy of the tokens (the floor of anything that reads them once) and the host statement fp_reference on --host-rows
     of them, scaled to the batch; the launch's bits are compared with the host statement's.
  2. gct_fp_tanimoto at --square x --square and at --small-n x --large-m (small n, many splits) on random fingerprints
     of about 64 bits, against the same three results composed in torch on the matrix pipe: both sides unpacked to 0/1
     matrices, torch.matmul for the intersection counts, an elementwise division, max, argmax and an fp64 sum, chunked
     over b to fit memory.  The matrices are fp16, not bf16: torch.matmul returns its operands' type, and a count of up
     to 1024 is exact in fp16 but not in bf16.  The two are compared: best and arg exactly, total relatively.
  3. molkey.basic_metrics with fingerprints end to end (check + keys + fingerprints + all-pairs Tanimoto + sorts) on the
     rows of 1.
Every comparison is alternated three times in one process, the median is reported.
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
ap.add_argument("--iters", type=int, default=50, help="launches per timed leg of the row kernels")
ap.add_argument("--square", type=int, default=32768)
ap.add_argument("--small-n", type=int, default=4096)
ap.add_argument("--large-m", type=int, default=1 << 20)
ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("rows", "host_rows", "iters", "square", "small_n", "large_m"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"fp_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.data import tokenize  # noqa: E402
from gct_plus_amd.smiles import ChemReport, SmilesChemistry  # noqa: E402
from gct_plus_amd.fingerprint import FpRows, SmilesFingerprints  # noqa: E402
from gct_plus_amd.molkey import MolKeyIndex, MolKeys, basic_metrics  # noqa: E402
from gct_plus_amd.randomize import stream  # noqa: E402

MOLECULES = ["CCO", "c1ccccc1", "CC(=O)O", "C1CC1", "N#N", "c1cc[nH]c1", "CS(=O)(=O)C", "O=c1cccc[nH]1",
             "CC(=O)Oc1ccccc1C(=O)O", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2ccccc2c1", "c1ccncc1", "C[N+](C)(C)C",
             "CC(=O)[O-]", "c1ccsc1", "Cn1cccc1", "c1ccoc1", "FC(F)(F)c1ccccc1", "C[n+]1ccccc1", "CP(C)(C)=O",
             "C12CC1C2", "c1ccc(-c2ccccc2)cc1", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CN1CCCC1c1cccnc1",
             "OCC(O)CO", "NC(=O)c1ccccc1", "CC(C)(C)c1ccc(O)cc1", "C1CCC2CCCCC2C1"]
V, W, T0 = synthetic.CHEM_VOCAB, 80, 4
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
fs, chem = SmilesFingerprints(V, PAD, EOS), SmilesChemistry(V, PAD, EOS)
ks = fs.keys
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
ctable, cwords = chem.device_tables("cuda")
fp_outs = (torch.empty(a.rows, 16, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"))
key_outs = (torch.empty(a.rows, 2, dtype=torch.int64, device="cuda"), torch.empty(a.rows, 4, dtype=torch.int32, device="cuda"))
report = torch.empty(a.rows, 4, dtype=torch.int32, device="cuda")
copy = torch.empty_like(dev)
index = MolKeyIndex(torch.tensor([ks.key(ids)[1] for ids in mols[::2]]))
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


# ------------------------------------------------------------------------------------------------ 1. gct_smiles_fp
def host_statement():
    t0 = time.perf_counter()
    got = fs.fp_reference(ys[:a.host_rows], [T0] * a.host_rows)
    return got, (time.perf_counter() - t0) * 1e3 * a.rows / a.host_rows


def metrics():
    ops.smiles_check(dev, start, ctable, cwords, out=report)
    ops.smiles_key(dev, start, table, labels, PAD, EOS, -1, out=key_outs)
    ops.smiles_fp(dev, start, table, labels, PAD, EOS, -1, out=fp_outs)
    return basic_metrics(ChemReport(*report.unbind(1)), MolKeys(*key_outs), index, FpRows(*fp_outs))


kern, keys, floor, host, end = [], [], [], [], []
for _ in range(3):
    kern.append(timed(lambda: ops.smiles_fp(dev, start, table, labels, PAD, EOS, -1, out=fp_outs), a.iters))
    keys.append(timed(lambda: ops.smiles_key(dev, start, table, labels, PAD, EOS, -1, out=key_outs), a.iters))
    floor.append(timed(lambda: copy.copy_(dev), a.iters))
    ref, ms = host_statement()
    host.append(ms)
    end.append(timed(metrics, 3) / 1e3)
wrong = int((fp_outs[0][:a.host_rows].cpu() != ref.bits).any(1).sum() + (fp_outs[1][:a.host_rows].cpu() != ref.info).any(1).sum())
info = fp_outs[1].cpu()
print(f"fp_bench: {a.rows} rows x {W} columns ({dev.numel() * 8 / 1e6:.1f} MB of tokens); rows with a fingerprint "
      f"{float((info[:, 0] == ops.FP_GRAPH).float().mean()):.3f}, mean bits {float(info[:, 1].float().mean()):.1f}; rows "
      f"that differ from the host statement (of {a.host_rows}): {wrong}")
print(f"  gct_smiles_fp       {med(kern):9.1f} us per launch  (three legs: {legs(kern)})")
print(f"  gct_smiles_key      {med(keys):9.1f} us per launch  (three legs: {legs(keys)}), the fingerprints are "
      f"{med(kern) / med(keys):.2f} x it")
print(f"  device copy (floor) {med(floor):9.1f} us per copy    (three legs: {legs(floor)})")
print(f"  host statement      {med(host) * 1e3:9.1f} us per batch   (three legs: {legs([x * 1e3 for x in host], '.0f')}, scaled "
      f"from {a.host_rows} rows), {med(host) * 1e3 / med(kern):.0f} x the launch")
print(f"  basic_metrics with intDiv end to end (check + keys + fingerprints + {a.rows} x {a.rows} Tanimoto + sorts) "
      f"{med(end):.2f} ms ({legs(end, '.2f')}): {metrics()}", flush=True)


# ------------------------------------------------------------------------------------------------ 2. gct_fp_tanimoto
SHIFTS = torch.arange(64, device="cuda")


def unpack(bits):
    """int64 [k, 16] -> fp16 [k, 1024] of 0 / 1."""
    return ((bits[:, :, None] >> SHIFTS) & 1).reshape(bits.shape[0], 1024).to(torch.float16)


def random_rows(k, seed):
    """k random fingerprints at bit density 1/16 (the AND of four random words) and their counts."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (k, 16), generator=g, device="cuda")
    for _ in range(3):
        bits &= torch.randint(-2 ** 63, 2 ** 63 - 1, (k, 16), generator=g, device="cuda")
    cnt = torch.cat([unpack(bits[i:i + 65536]).float().sum(1) for i in range(0, k, 65536)]).to(torch.int32)
    return bits, cnt


def composed(abits, ca, bbits, cb, chunk):
    """(best, arg, total) through torch.matmul, chunk rows of b at a time."""
    A = unpack(abits)
    n = abits.shape[0]
    best = torch.full((n,), -1.0, device="cuda")
    arg = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    total = torch.zeros(n, dtype=torch.float64, device="cuda")
    caf = ca.float()[:, None]
    for lo in range(0, bbits.shape[0], chunk):
        c = torch.matmul(A, unpack(bbits[lo:lo + chunk]).t()).float()
        cbf = cb[lo:lo + chunk].float()[None, :]
        t = c / (caf + cbf - c)
        t = torch.where((cbf > 0) & (caf > 0), t, torch.full_like(t, -1.0))
        total += t.clamp(min=0).double().sum(1)
        b, j = t.max(1)
        take = b > best
        best, arg = torch.where(take, b, best), torch.where(take, j + lo, arg)
    return best.clamp(min=0), arg, total


for n, m, chunk, iters in ((a.square, a.square, 8192, 5), (a.small_n, a.large_m, 65536, 2)):
    abits, ca = random_rows(n, 1)
    bbits, cb = random_rows(m, 2)
    outs = (torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
            torch.empty(n, dtype=torch.float64, device="cuda"))
    mine, theirs = [], []
    for _ in range(3):
        mine.append(timed(lambda: ops.fp_tanimoto(abits, ca, bbits, cb, 1, out=outs), iters))
        theirs.append(timed(lambda: composed(abits, ca, bbits, cb, chunk), 1))
    want = composed(abits, ca, bbits, cb, chunk)
    rel = float(((outs[2] - want[2]).abs() / want[2].clamp(min=1e-300)).max())
    tile_b, splits = ops.fp_tanimoto_plan(n, m)
    print(f"fp_bench: gct_fp_tanimoto {n} x {m} ({n * m / 1e9:.2f} G pairs, tiles of {tile_b}, {splits} splits): "
          f"{med(mine) / 1e3:.3f} ms ({legs([x / 1e3 for x in mine], '.3f')}), {med(mine) * 1e6 / (n * m):.2f} ps per pair; "
          f"torch composition on the matrix pipe {med(theirs) / 1e3:.1f} ms ({legs([x / 1e3 for x in theirs])}), "
          f"{med(theirs) / med(mine):.1f} x the kernel; best differs on {int((outs[0] != want[0]).sum())} rows, arg on "
          f"{int((outs[1] != want[1]).sum())}, total by at most {rel:.1e} relatively", flush=True)
    del abits, bbits, want
    torch.cuda.empty_cache()
sys.exit(1 if wrong else 0)
