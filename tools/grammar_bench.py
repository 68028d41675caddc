#!/usr/bin/env python3
"""Grammar-constrained decoding measurements (recorded in the README, not gated).  Full-size pscavaetf, synthetic
weights, the hand-made 31-token SMILES vocabulary synthetic.GRAMMAR_VOCAB: generate_stream of --pool items through
--rows rows, multinomial, up to 79 tokens each, with and without grammar=SmilesGrammar, alternated three times in one
process.  Prints SMILES/s for both
(what the one extra launch per step, gct_grammar_mask, costs -- and what rows that end by themselves give back) and the
share of rows SmilesGrammar.well_formed accepts in each run.
The measurement runs in a child process under `timeout` (a GPU step that hangs ends there)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pool", type=int, default=8192)
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--pool", str(a.pool),
           "--rows", str(a.rows)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"grammar_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import KVDecoder, generated_tokens  # noqa: E402
from gct_plus_amd.smiles import SmilesGrammar  # noqa: E402

mtype = "pscavaetf"
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
PAD, SOS, EOS = synthetic.PAD_ID, synthetic.SOS_ID, synthetic.EOS_ID
assert len(synthetic.GRAMMAR_VOCAB) == vt
grammar = SmilesGrammar(synthetic.GRAMMAR_VOCAB, PAD, EOS)
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()

N, R, Le = a.pool, a.rows, 40 + nc
z = torch.randn(N, Le, 128, device="cuda")
dconds = torch.randn(N, nc, device="cuda")
src_mask = torch.ones(N, 1, Le, dtype=torch.bool, device="cuda")
ys0 = torch.full((N, 1), SOS, dtype=torch.long, device="cuda")
kd = KVDecoder(model, PAD, SOS, EOS)


def run(gr):
    kd.start_stream(z, src_mask, dconds, rows=R, max_total_len=80)
    return kd.generate_stream(ys0, 80, algo="multinomial", seed=3, use_graphs=True, grammar=gr)


def timed_once(gr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(gr)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def share_well_formed(ys):
    gen = generated_tokens(ys.cpu(), torch.ones(N, dtype=torch.long)).tolist()
    return sum(grammar.well_formed(row) for row in gen) / N


run(None), run(grammar)                                                      # warm-up / capture of both graphs
t, share, units = {False: [], True: []}, {}, {}
for rep in range(3):
    for on in (False, True):
        (ys, rec), dt = timed_once(grammar if on else None)
        t[on].append(dt)
        share[on], units[on] = share_well_formed(ys), rec["launched"]
        print(f"rep {rep}: grammar={on!s:5} {dt * 1e3:8.1f} ms ({rec['launched']} step units, "
              f"{dt / rec['launched'] * 1e3:.3f} ms each) -> {N / dt:7.0f} SMILES/s, well formed {share[on]:.4f}",
              flush=True)
b0, b1 = min(t[False]), min(t[True])
print(f"generate_stream {N} items / {R} rows, multinomial, max_strlen 80: {N / b0:.0f} SMILES/s without the grammar "
      f"({units[False]} step units, {b0 / units[False] * 1e3:.3f} ms each, well formed {share[False]:.4f}), {N / b1:.0f} "
      f"with it ({units[True]} step units, {b1 / units[True] * 1e3:.3f} ms each, well formed {share[True]:.4f}); best of 3 "
      f"each, spread without {(max(t[False]) - b0) / b0:.3f}; replay: {'graph' if kd.graph_replay else 'eager'}")
