#!/usr/bin/env python3
"""Log-likelihood measurements (recorded in the README, not gated).  Full-size pscavaetf, synthetic weights.
  decode  generate_stream of --pool items through --rows rows (lengths imposed as in decode_bench.py --stream-rows:
          eos_id = -1, caps clip(round(N(35, 8)), 15, 78) + 1), with and without return_logp, alternated three times
          in one process: what the one extra launch per step (gct_chosen_logp) costs;
  score   score_tokens on --molecules full rows of the same MOSES-like lengths, molecules/s, next to the same rows
          rescored by model.decode + torch.log_softmax + gather in chunks of the same size.
Without an argument both parts run, each in a child process of its own under `timeout` (a GPU step that hangs ends
there and nothing is started after it)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("part", nargs="?", choices=["decode", "score"], help="one part, in this process (default: both)")
ap.add_argument("--pool", type=int, default=8192)
ap.add_argument("--rows", type=int, default=512)
ap.add_argument("--molecules", type=int, default=32768)
ap.add_argument("--chunk", type=int, default=512)
ap.add_argument("--limit", type=int, default=420, help="seconds each part may take")
a = ap.parse_args()

if a.part is None:
    for part in ("decode", "score"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), part, "--pool", str(a.pool),
               "--rows", str(a.rows), "--molecules", str(a.molecules), "--chunk", str(a.chunk)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"score_bench: part {part!r} ended with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.Model.modules import get_trg_mask  # noqa: E402
from gct_plus_amd.decode import KVDecoder, score_tokens  # noqa: E402

mtype = "pscavaetf"
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
PAD, SOS, EOS = synthetic.PAD_ID, synthetic.SOS_ID, synthetic.EOS_ID
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()


def timed_once(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def moses_lengths(n):
    return np.clip(np.rint(np.random.default_rng(0).normal(35, 8, n)), 15, 78).astype(np.int64)


if a.part == "decode":
    N, R, Le = a.pool, a.rows, 40 + nc
    z = torch.randn(N, Le, 128, device="cuda")
    dconds = torch.randn(N, nc, device="cuda")
    src_mask = torch.ones(N, 1, Le, dtype=torch.bool, device="cuda")
    ys0 = torch.full((N, 1), SOS, dtype=torch.long, device="cuda")
    caps = torch.from_numpy(moses_lengths(N) + 1)
    kd = KVDecoder(model, PAD, SOS, eos_id=-1)

    def run(logp):
        kd.start_stream(z, src_mask, dconds, rows=R, max_total_len=80)
        return kd.generate_stream(ys0, 80, max_new_tokens=caps, use_graphs=True, return_logp=logp)

    run(False), run(True)                                                    # warm-up / capture of both graphs
    t = {False: [], True: []}
    for rep in range(3):
        for logp in (False, True):
            out, dt = timed_once(lambda: run(logp))
            t[logp].append(dt)
            print(f"rep {rep}: return_logp={logp!s:5} {dt * 1e3:8.1f} ms ({out[1]['launched']} step units, "
                  f"{dt / out[1]['launched'] * 1e3:.3f} ms each) -> {N / dt:7.0f} molecules/s", flush=True)
    b0, b1 = min(t[False]), min(t[True])
    print(f"generate_stream {N} items / {R} rows: {N / b0:.0f} molecules/s without, {N / b1:.0f} with return_logp "
          f"(best of 3 each; with / without time {b1 / b0:.4f}; spread without {(max(t[False]) - b0) / b0:.3f}); replay: "
          f"{'graph' if kd.graph_replay else 'eager'}")
    sys.exit(0)

n, CH, Le = a.molecules, a.chunk, 80 + nc
ln = moses_lengths(n)                                                        # molecule tokens; row = <sos> tokens <eos>
W = int(ln.max()) + 2
g = torch.Generator().manual_seed(3)
ys = torch.randint(5, vt, (n, W), generator=g)
ys[:, 0] = SOS
cols = torch.arange(W)[None, :]
end = torch.from_numpy(ln)[:, None] + 1
ys[cols == end] = EOS
ys[cols > end] = PAD
ys = ys.cuda()
z = torch.randn(n, Le, 128, device="cuda")
dconds = torch.randn(n, nc, device="cuda")
src_mask = (torch.arange(Le, device="cuda")[None, :] < (torch.from_numpy(ln).cuda() + nc)[:, None]).unsqueeze(1)


def scored():
    return score_tokens(model, z, src_mask, dconds, ys, pad_id=PAD, chunk=CH)[0]


@torch.no_grad()
def torch_rescore():
    out = torch.empty(n, device="cuda")
    for lo in range(0, n, CH):
        y = ys[lo:lo + CH]
        trg = y[:, :-1]
        logits = model.decode(trg, z[lo:lo + CH], src_mask[lo:lo + CH], get_trg_mask(trg, PAD, False, dconds[lo:lo + CH]),
                              dconds[lo:lo + CH])
        lp = torch.log_softmax(logits.float(), -1).gather(-1, y[:, 1:].unsqueeze(-1)).squeeze(-1)
        out[lo:lo + CH] = (lp * (y[:, 1:] != PAD)).sum(1)
    return out


a_, b_ = scored(), torch_rescore()                                           # warm-up
print(f"{n} molecules, rows of {W} tokens, chunks of {CH}; max |score_tokens - torch rescoring| "
      f"{float((a_ - b_).abs().max()):.3e} at |logp| up to {float(b_.abs().max()):.1f}", flush=True)
ts, tt = [], []
for rep in range(3):
    ts.append(timed_once(scored)[1])
    tt.append(timed_once(torch_rescore)[1])
    print(f"rep {rep}: score_tokens {ts[-1] * 1e3:8.1f} ms -> {n / ts[-1]:8.0f} molecules/s | model.decode + log_softmax "
          f"+ gather {tt[-1] * 1e3:8.1f} ms -> {n / tt[-1]:8.0f} molecules/s", flush=True)
print(f"score_tokens {n / min(ts):.0f} molecules/s, torch rescoring {n / min(tt):.0f} molecules/s (best of 3 each; ratio "
      f"{min(tt) / min(ts):.2f})")
