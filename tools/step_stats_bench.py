#!/usr/bin/env python3
"""What return_stats costs a sampling run (recorded in the README, not gated).  Full-size pscavaetf, synthetic weights,
the hand-made 31-token SMILES vocabulary synthetic.GRAMMAR_VOCAB: generate_stream of --pool items through --rows rows,
multinomial with top_p = 0.9 and the grammar, up to 79 tokens each, with and without return_stats=True, alternated three
times in one process.  Prints SMILES/s and ms per step unit for both: the difference is one more launch per step
(gct_step_stats) and the [rows, V] store of the draw's distribution (gct_select_token's probs_out).
--without-only runs the leg without statistics alone and passes no return_stats argument, so the same file measures a
checkout from before the feature.
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
ap.add_argument("--without-only", action="store_true", help="only the leg without statistics (any checkout)")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--pool", str(a.pool),
           "--rows", str(a.rows)] + ["--without-only"] * a.without_only
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"step_stats_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import KVDecoder  # noqa: E402
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


def run(stats):
    kd.start_stream(z, src_mask, dconds, rows=R, max_total_len=80)
    kw = dict(return_stats=True) if stats else {}
    return kd.generate_stream(ys0, 80, algo="multinomial", seed=3, top_p=0.9, use_graphs=True, grammar=grammar, **kw)


def timed_once(stats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(stats)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


legs = (False,) if a.without_only else (False, True)
for on in legs:
    run(on)                                                                  # warm-up / capture of the leg's graph
t, units, tokens = {on: [] for on in legs}, {}, {}
for rep in range(3):
    for on in legs:
        out, dt = timed_once(on)
        t[on].append(dt)
        units[on], tokens[on] = out[1]["launched"], int(out[1]["out_len"].sum())
        extra = f", mean model entropy {float(out[2].model_entropy.sum()) / tokens[on]:.3f} nat / token, mean " \
                f"behaviour KL {float(out[2].behaviour_kl.sum()) / tokens[on]:.3f}" if on else ""
        print(f"rep {rep}: return_stats={on!s:5} {dt * 1e3:8.1f} ms ({units[on]} step units, "
              f"{dt / units[on] * 1e3:.3f} ms each) -> {N / dt:7.0f} SMILES/s{extra}", flush=True)
best = {on: min(t[on]) for on in legs}
line = (f"generate_stream {N} items / {R} rows, multinomial, top_p 0.9, grammar, max_strlen 80: {N / best[False]:.0f} "
        f"SMILES/s without return_stats ({units[False]} step units, {best[False] / units[False] * 1e3:.3f} ms each, "
        f"spread {(max(t[False]) - best[False]) / best[False]:.3f})")
if True in legs:
    line += (f", {N / best[True]:.0f} with it ({units[True]} step units, {best[True] / units[True] * 1e3:.3f} ms each, "
             f"spread {(max(t[True]) - best[True]) / best[True]:.3f}): {(best[True] / best[False] - 1) * 100:+.2f} %")
print(line + f"; best of 3 each; replay: {'graph' if kd.graph_replay else 'eager'}")
