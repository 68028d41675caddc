#!/usr/bin/env python3
"""Sequential Monte Carlo decoding measurements (recorded in the README and DESIGN section 4, not gated).  Full-size
pscavaetf, synthetic weights, graph replay: --scaffolds prefixes (<sos>, five tokens, <sep>), one latent each, k = --k
particles, up to 79 tokens, the grammar of synthetic.GRAMMAR_VOCAB.
  smc          KVDecoder.generate_smc at ess_threshold 0 / 0.5 / 1: ms per step unit (decode time over the token columns
               written), exp(log_z) averaged over the scaffolds, the ESS of the final weights, resampling events;
  constrained  KVDecoder.generate(algo="multinomial", grammar=) of the same scaffolds x k rows: ms per step unit;
  free         the same rows without a grammar: the share that happens to be well formed -- what the average of
               exp(log_z) estimates.
Alternated three times in one process; best of three per leg.  The measurement runs in a child process under `timeout`
(a GPU step that hangs ends there)."""
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
ap.add_argument("--limit", type=int, default=420, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--scaffolds",
           str(a.scaffolds), "--k", str(a.k)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"smc_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import torch  # noqa: E402

from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import KVDecoder  # noqa: E402
from gct_plus_amd.smiles import SmilesGrammar  # noqa: E402

mtype = "pscavaetf"
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
PAD, SOS, EOS, SEP = synthetic.PAD_ID, synthetic.SOS_ID, synthetic.EOS_ID, synthetic.SEP_ID
grammar = SmilesGrammar(synthetic.GRAMMAR_VOCAB, PAD, EOS)
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()

S, K, Le, STRLEN = a.scaffolds, a.k, 40 + nc, 80
g = torch.Generator().manual_seed(2)
z = torch.randn(S, Le, 128, generator=g).cuda()
dconds = torch.randn(S, nc, generator=g).cuda()
src_mask = torch.ones(S, 1, Le, dtype=torch.bool, device="cuda")
ys0 = torch.cat([torch.full((S, 1), SOS), torch.randint(5, vt, (S, 5), generator=g), torch.full((S, 1), SEP)], 1).cuda()
t0 = ys0.shape[1]
rep = lambda x: x.repeat_interleave(K, 0)          # noqa: E731
kd_s, kd_m = KVDecoder(model, PAD, SOS, EOS), KVDecoder(model, PAD, SOS, EOS)
kd_s.start(z, src_mask, dconds, max_total_len=t0 + STRLEN, beams=K)
kd_m.start(rep(z), rep(src_mask), rep(dconds), max_total_len=t0 + STRLEN)


def timed(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    out, cols = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - start) * 1e3 / cols


def smc(tau, seed):
    out = kd_s.generate_smc(ys0, K, grammar, STRLEN, seed=seed, ess_threshold=tau, use_graphs=True)
    return out, out.ys.shape[2] - t0


def constrained(seed):
    ys = kd_m.generate(rep(ys0), STRLEN, algo="multinomial", seed=seed, grammar=grammar, use_graphs=True)
    return ys, ys.shape[1] - t0


def free(seed):
    ys = kd_m.generate(rep(ys0), STRLEN, algo="multinomial", seed=seed, use_graphs=True)
    return ys, ys.shape[1] - t0


smc(0.5, 1), constrained(1), free(1)                # warm-up / capture of the graphs
best, zs, ess, res, wf = {}, {}, {}, {}, []
for r in range(3):
    for tau in (0.0, 0.5, 1.0):
        out, ms = timed(lambda: smc(tau, 10 + r))
        best[tau] = min(best.get(tau, ms), ms)
        zs.setdefault(tau, []).append(float(torch.exp(out.log_z).mean()))
        ess.setdefault(tau, []).append(float(out.ess.mean()))
        res.setdefault(tau, []).append(float(out.resamples.float().mean()))
        print(f"rep {r}: smc tau={tau:.1f} {ms:7.3f} ms/step, mean Z^ {zs[tau][-1]:.3e}, mean ESS {ess[tau][-1]:.2f} of {K}, "
              f"{res[tau][-1]:.1f} resamplings per scaffold", flush=True)
    _, ms = timed(lambda: constrained(10 + r))
    best["constrained"] = min(best.get("constrained", ms), ms)
    print(f"rep {r}: constrained multinomial {ms:7.3f} ms/step", flush=True)
    ys, ms = timed(lambda: free(10 + r))
    best["free"] = min(best.get("free", ms), ms)
    rows = ys[:, t0:].tolist()
    wf.append(sum(grammar.well_formed(row[:row.index(EOS) + 1]) for row in rows if EOS in row) / len(rows))
    print(f"rep {r}: unconstrained multinomial {ms:7.3f} ms/step, {100 * wf[-1]:.2f} % of {len(rows)} rows well formed",
          flush=True)
mean = lambda v: sum(v) / len(v)                    # noqa: E731
print(f"{S} scaffolds x k = {K} ({S * K} rows), max_strlen {STRLEN}, best of 3: generate_smc "
      + ", ".join(f"tau {t:g}: {best[t]:.3f} ms/step" for t in (0.0, 0.5, 1.0))
      + f"; generate(multinomial, grammar) {best['constrained']:.3f} ms/step; unconstrained {best['free']:.3f} ms/step.  "
      + "mean Z^ " + ", ".join(f"tau {t:g}: {mean(zs[t]):.3e}" for t in (0.0, 0.5, 1.0))
      + f" against {100 * mean(wf):.2f} % well-formed unconstrained rows.  Final ESS of {K}: "
      + ", ".join(f"tau {t:g}: {mean(ess[t]):.2f} ({mean(res[t]):.1f} resamplings)" for t in (0.0, 0.5, 1.0))
      + f".  replay: smc {'graph' if kd_s.graph_replay else 'eager'}, multinomial {'graph' if kd_m.graph_replay else 'eager'}")
