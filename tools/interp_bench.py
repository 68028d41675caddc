#!/usr/bin/env python3
"""Molecule interpolation measurements (recorded in the README, not gated).  Full-size pscavaetf, synthetic weights,
--pairs pairs x --alphas interior alphas, well_formed=True and graph replay.  Two
variants of the same work, alternated three times in one process, the median of each reported as cells resolved per
second:
  batched   one Sampling.interpolate_smiles call of a sampler with stream_rows=512: the tries of every (pair, alpha)
            cell are rows of one decode per round
  one row   the reference's loop: per pair two encodes, per cell one latent and ONE decoded row per try until one is
            accepted (ops.latent_interp with R = 1, Sampling.decode with one row on a sampler WITHOUT stream_rows: a
            plain batch-1 generate, graph replay); timed on the first --single-cells cells
            (the rate does not depend on how many cells there are: every try is a decode of its own)
Both accept with the default rule (SmilesGrammar.well_formed and a non-empty string).
The measurement runs in a child process under `timeout` (a GPU step that hangs ends there)."""
import argparse
import itertools
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--alphas", type=int, default=8)
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--chunk", type=int, default=16)
ap.add_argument("--single-cells", type=int, default=64, help="cells the one-row variant is timed on")
ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take")
ap.add_argument("--child", action="store_true", help="run the measurement in this process")
a = ap.parse_args()

if not a.child:
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"]
    for k in ("pairs", "alphas", "rows", "chunk", "single_cells"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print(f"interp_bench: the measurement ended with status {rc}", flush=True)
    sys.exit(rc)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gct_plus_amd import data, ops  # noqa: E402
from gct_plus_amd.Inference.mol_interpolation import interior_alphas, interp_plan, lerp, noise_ladder  # noqa: E402
from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import generated_tokens  # noqa: E402
from gct_plus_amd.smiles import SmilesGrammar  # noqa: E402

# well-known drug-like molecules (public SMILES), all carrying a benzene ring: the scaffold of every row
MOLS = ["CC(=O)Oc1ccccc1C(=O)O", "CC(C)Cc1ccc(cc1)C(C)C(=O)O", "CC(=O)Nc1ccc(O)cc1", "CN1CCCC1c1cccnc1",
        "COc1ccc2[nH]cc(CCNC(C)=O)c2c1", "CN(C)CCc1c[nH]c2ccc(O)cc12", "NC(Cc1ccccc1)C(=O)O", "OC(=O)c1ccccc1O",
        "Cc1ccc(cc1)S(N)(=O)=O", "CCN(CC)C(=O)c1ccccc1", "Clc1ccc(cc1)C(c1ccccc1)N1CCNCC1", "CC(N)Cc1ccccc1",
        "COc1cc(C=O)ccc1O", "CCOC(=O)c1ccc(N)cc1", "O=C(O)Cc1ccccc1Nc1c(Cl)cccc1Cl", "CC(C)NCC(O)c1ccc(O)c(O)c1"]
SCAFFOLD = "c1ccccc1"
pairs = list(itertools.combinations(range(len(MOLS)), 2))[:a.pairs]
if len(pairs) < a.pairs:
    raise SystemExit(f"at most {len(pairs)} pairs")
src0, src1 = [MOLS[i] for i, _ in pairs], [MOLS[j] for _, j in pairs]
strs = [SCAFFOLD + "<sep>" + s for s in MOLS]
SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
torch.manual_seed(1)
model = model_dict["pscavaetf"](len(SRC), len(TRG), N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1,
                                nconds=3, use_cond2lat=True).cuda().eval()
sp = PscavaetfSampling(model, SRC, TRG, latent_dim=128, max_strlen=80, cond_dim=3, decode_algo="greedy", seed=1,
                       use_graphs=True, stream_rows=a.rows, well_formed=True)
# the one-row leg decodes on a sampler of its own WITHOUT stream_rows: a plain batch-1 generate under graph replay, not
# one live row of a 512-row step
sp1 = PscavaetfSampling(model, SRC, TRG, latent_dim=128, max_strlen=80, cond_dim=3, decode_algo="greedy", seed=1,
                        use_graphs=True, well_formed=True)
P, A = a.pairs, a.alphas
g = np.random.default_rng(0)
props0, props1 = g.uniform(0, 1, (P, 3)), g.uniform(0, 1, (P, 3))
sca = [SCAFFOLD] * P
alphas, ladder = interior_alphas(A), noise_ladder()
grammar = SmilesGrammar(TRG.itos, sp.pad_id, sp.eos_id)


def batched():
    res = sp.interpolate_smiles(src0, src1, A, scaffolds0=sca, scaffolds1=sca, props0=props0, props1=props1,
                                chunk=a.chunk, transform=False)
    return int((res.tries >= 0).sum()), res.rows_decoded, P * A


TMAX = 96                                                                    # latent rows of every one-row decode: one
                                                                             # geometry, so its captured graph is replayed


@torch.no_grad()
def one_row(cells):
    """The reference's order of work on the first `cells` cells: (resolved, rows decoded, cells)."""
    resolved = rows = done = 0
    ys0, plens, extras = sp1._scaffold_prefixes([SCAFFOLD])
    for p in range(P):
        if done >= cells:
            break
        enc = [sp1.encode_smiles([s], [SCAFFOLD], pr[p:p + 1], transform=False) for s, pr in ((src0[p], props0), (src1[p], props1))]
        lens = [e[1].shape[1] for e in enc]
        stats = torch.cat([ops.latent_stats(e[1].contiguous(), e[2].contiguous(), [e[1].shape[1]]) for e in enc])
        toklen = interp_plan(lens[:1], lens[1:], alphas, extras)[0]
        for i, al in enumerate(alphas):
            if done >= cells:
                break
            done += 1
            dconds = torch.as_tensor(lerp(props0[p:p + 1], props1[p:p + 1], al), dtype=torch.float32)
            T = int(toklen[i])
            assert T <= TMAX
            mask = (torch.arange(TMAX) < T).view(1, 1, TMAX)
            for k, std in enumerate(ladder):
                z = ops.latent_interp(stats, [0], [1], [al], [std], [T], [(p * A + i) * len(ladder) + k], TMAX,
                                      sp1.latent_seed)
                out = sp1.decode(z, ys0, mask, dconds, prefix_lens=plens, return_rows=True)
                gen = generated_tokens(out[1].ys, out[1].prefix_lens)[0].cpu().numpy()
                rows += 1
                if sp1.id_to_smi(gen) and grammar.well_formed(gen):
                    resolved += 1
                    break
    return resolved, rows, done


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


timed(batched), timed(one_row, 2)                                            # warm-up: code objects, graph capture
t = {"batched": [], "one row": []}
info = {}
for rep in range(3):
    for name, fn, args in (("batched", batched, ()), ("one row", one_row, (a.single_cells,))):
        (resolved, rows, cells), dt = timed(fn, *args)
        t[name].append(resolved / dt)
        info[name] = (resolved, rows, cells)
        print(f"rep {rep}: {name:8} {dt * 1e3:9.1f} ms, {resolved} of {cells} cells resolved, {rows} rows decoded -> "
              f"{resolved / dt:8.1f} cells/s", flush=True)
mb, mo = statistics.median(t["batched"]), statistics.median(t["one row"])
print(f"interpolate_smiles {P} pairs x {A} alphas, full-size pscavaetf, stream_rows {a.rows}, well_formed, chunk {a.chunk}: "
      f"{mb:.1f} cells/s batched ({info['batched'][1]} rows decoded for {info['batched'][2]} cells), {mo:.1f} cells/s one "
      f"row per decode on a batch-1 sampler without stream_rows (timed on {info['one row'][2]} cells, {info['one row'][1]} rows); medians of 3, alternated; "
      f"spread batched {(max(t['batched']) - min(t['batched'])) / mb:.3f}, one row "
      f"{(max(t['one row']) - min(t['one row'])) / mo:.3f}; replay: {'graph' if sp.kv.graph_replay else 'eager'} / {'graph' if getattr(sp1.kv, 'graph_replay', False) else 'eager'}")
