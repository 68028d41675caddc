#!/usr/bin/env python3
"""Stochastic beam search measurements (recorded in the README, not gated).  Full-size pscavaetf, synthetic weights,
graph replay: --scaffolds prefixes (<sos>, five tokens, <sep>), one latent each, up to 79 tokens.
  unique       KVDecoder.generate_sbs with k = --k: k DISTINCT token rows per scaffold, by construction;
  multinomial  KVDecoder.generate of the same scaffolds x k rows (every scaffold's latent repeated k times), the rows
               of a scaffold de-duplicated on the host.
Alternated three times in one process.  Prints distinct SMILES (token rows up to <eos>) per second and the distinct count
of both.  --sharpen multiplies the output layer: the synthetic weights give a near-uniform next-token distribution, under
which a multinomial decode never repeats itself, whereas a fine-tuned policy is sharp -- the case the feature is for.
The measurement runs in a child process under `timeout` (a GPU step that hangs ends there)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--scaffolds", type=int, default=64)
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--sharpen", type=float, default=6.0, help="factor on the output layer's weight and bias")
ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--scaffolds",
           str(a.scaffolds), "--k", str(a.k), "--sharpen", str(a.sharpen)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"sbs_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import KVDecoder  # noqa: E402

mtype = "pscavaetf"
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
PAD, SOS, EOS, SEP = synthetic.PAD_ID, synthetic.SOS_ID, synthetic.EOS_ID, synthetic.SEP_ID
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()
with torch.no_grad():
    model.out.weight.mul_(a.sharpen)
    model.out.bias.mul_(a.sharpen)
    model.out.bias[PAD] = -1e9                      # <pad> is never a token of a molecule

S, K, Le = a.scaffolds, a.k, 40 + nc
g = torch.Generator().manual_seed(2)
z = torch.randn(S, Le, 128, generator=g).cuda()
dconds = torch.randn(S, nc, generator=g).cuda()
src_mask = torch.ones(S, 1, Le, dtype=torch.bool, device="cuda")
ys0 = torch.cat([torch.full((S, 1), SOS), torch.randint(5, vt, (S, 5), generator=g), torch.full((S, 1), SEP)], 1).cuda()
t0 = ys0.shape[1]
rep = lambda x: x.repeat_interleave(K, 0)          # noqa: E731
kd_u, kd_m = KVDecoder(model, PAD, SOS, EOS), KVDecoder(model, PAD, SOS, EOS)


def molecules(rows):
    """The rows' generated tokens up to <eos> as tuples, [S][K]."""
    out = []
    for s in range(S):
        mols = []
        for r in rows[s].tolist():
            gen = r[t0:]
            mols.append(tuple(gen[:gen.index(EOS) + 1] if EOS in gen else gen))
        out.append(mols)
    return out


def unique(seed):
    kd_u.start(z, src_mask, dconds, max_total_len=t0 + 80, beams=K)
    ys = kd_u.generate_sbs(ys0, K, 80, seed=seed, use_graphs=True).ys.cpu()
    return sum(len(set(m)) for m in molecules(ys))


def multinomial(seed):
    kd_m.start(rep(z), rep(src_mask), rep(dconds), max_total_len=t0 + 80)
    ys = kd_m.generate(rep(ys0), 80, algo="multinomial", seed=seed, use_graphs=True).cpu()
    return sum(len(set(m)) for m in molecules(ys.view(S, K, -1)))


def timed_once(fn, seed):
    torch.cuda.synchronize()
    start = time.perf_counter()
    distinct = fn(seed)                             # (ends with the copy to the host and the de-duplication)
    return distinct, time.perf_counter() - start


unique(1), multinomial(1)                           # warm-up / capture of both graphs
best, count = {}, {}
for r in range(3):
    for name, fn in (("unique", unique), ("multinomial", multinomial)):
        distinct, dt = timed_once(fn, 10 + r)
        if name not in best or distinct / dt > best[name]:
            best[name] = distinct / dt
        count.setdefault(name, []).append(distinct)
        print(f"rep {r}: {name:11} {dt * 1e3:8.1f} ms, {distinct} distinct of {S * K} rows -> {distinct / dt:7.0f} "
              f"distinct SMILES/s", flush=True)
print(f"{S} scaffolds x k = {K}, output layer x {a.sharpen:g}, max_strlen 80: decode_unique {best['unique']:.0f} distinct "
      f"SMILES/s ({count['unique']} distinct of {S * K}), multinomial + host de-duplication {best['multinomial']:.0f} "
      f"({count['multinomial']} distinct of {S * K}); best of 3 each; replay: unique "
      f"{'graph' if kd_u.graph_replay else 'eager'}, multinomial {'graph' if kd_m.graph_replay else 'eager'}")
