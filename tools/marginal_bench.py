#!/usr/bin/env python3
"""Marginal-likelihood measurements (recorded in the README, not gated).  Full-size pscavaetf, synthetic weights,
MOSES-like lengths (synthetic.make_dataset: clip(round(N(35, 8)), 15, 78), molecule 0 at full length).
  estimate  one encoder forward + decode.marginal_logp (what Sampling.marginal_smiles runs behind the tokenizer) on
            --molecules molecules at K = 16 and K = 64, next to the same estimator composed in torch over the same
            blocks: torch.randn + the elementwise reparameterisation and log-weight terms + a masked reduction +
            score_tokens + torch.logsumexp.  Alternated three times in one process, host clock around a synchronise.
  kernel    gct_latent_iw alone on --rows output rows x 64 latent rows x 128 dimensions against a device copy of the
            same bytes (torch's vectorised copy_), HIP-event timed as tools/kernel_bench.py times, three rounds in turn.
Without an argument both parts run, each in a child process of its own under `timeout` (a GPU step that hangs ends
there and nothing is started after it)."""
import argparse
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("part", nargs="?", choices=["estimate", "kernel"], help="one part, in this process (default: both)")
ap.add_argument("--molecules", type=int, default=256)
ap.add_argument("--chunk", type=int, default=4096)
ap.add_argument("--rows", type=int, default=4096)
ap.add_argument("--limit", type=int, default=420, help="seconds each part may take")
a = ap.parse_args()

if a.part is None:
    for part in ("kernel", "estimate"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), part, "--molecules",
               str(a.molecules), "--chunk", str(a.chunk), "--rows", str(a.rows)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"marginal_bench: part {part!r} ended with status {rc}; stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402

from gct_plus_amd import ops, synthetic  # noqa: E402
from gct_plus_amd.decode import latent_rows, marginal_blocks, marginal_logp, score_tokens  # noqa: E402

if a.part == "kernel":
    R, Le, D = a.rows, 64, 128
    n, Kc = max(1, R // 16), 16
    R = n * Kc
    g = torch.Generator(device="cuda").manual_seed(0)
    mu = torch.randn(n, Le, D, device="cuda", generator=g)
    lv = 0.3 * torch.randn(n, Le, D, device="cuda", generator=g)
    tab = torch.stack([torch.randint(15, Le + 1, (n,)), torch.arange(n)]).to(torch.int32).cuda()
    z, logw, src = torch.empty(R, Le, D, device="cuda"), torch.empty(R, device="cuda"), torch.randn(R, Le, D, device="cuda")
    lib, p = ops._L(), ops._p

    def iw():
        ops.check(lib.gct_latent_iw(p(mu), p(lv), n, Le, D, p(tab[0]), p(tab[1]), 0, Kc, p(z), p(logw), None, 5, ops._st()),
                  "gct_latent_iw")

    def timeit(fn, reps=20, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        ts.sort()
        return ts[len(ts) // 2]

    nbytes = z.numel() * 4
    for rnd in range(3):
        tk, tc = timeit(iw), timeit(lambda: z.copy_(src))
        print(f"round {rnd}: gct_latent_iw {R} x {Le} x {D} ({nbytes / 1e6:.0f} MB of latents) {tk * 1e6:8.1f} us = "
              f"{nbytes / tk / 1e9:6.0f} GB/s written | copy of the same bytes {tc * 1e6:8.1f} us = {nbytes / tc / 1e9:6.0f} GB/s "
              f"written (and as much read) | time ratio {tk / tc:.2f}", flush=True)
    sys.exit(0)

from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.Model.modules import get_src_mask  # noqa: E402

mtype = "pscavaetf"
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
PAD = synthetic.PAD_ID
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()
n, CH = a.molecules, a.chunk
ds = {k: v.cuda() for k, v in synthetic.make_dataset(n, 78, mtype, seed=3).items()}
src_mask = get_src_mask(ds["src"], PAD, ds["econds"])
ys, dconds = ds["trg"], ds["dconds"]


@torch.no_grad()
def encode():
    _, mu, log_var = model.encode(src=ds["src"], src_mask=src_mask, econds=ds["econds"])
    return mu.contiguous(), log_var.contiguous()


def ours(K):
    mu, log_var = encode()
    return marginal_logp(model, mu, log_var, src_mask, dconds, ys, K=K, seed=7, chunk=CH, pad_id=PAD).iwae


@torch.no_grad()
def composed(K):
    """The same estimator in torch over the same blocks; its random stream depends on the blocks."""
    mu, log_var = encode()
    rows = latent_rows(src_mask, n, mu.shape[1]).cuda()
    own = (torch.arange(mu.shape[1], device="cuda").view(1, -1) < rows.view(-1, 1)).unsqueeze(-1)
    a_ = torch.empty(n, K, device="cuda", dtype=torch.float64)
    for i0, i1, k0, k1 in marginal_blocks(n, K, CH):
        Kc = k1 - k0
        rep = lambda x: x[i0:i1].repeat_interleave(Kc, 0)                      # noqa: E731
        m, lv, o = rep(mu), rep(log_var), rep(own)
        eps = torch.randn_like(m)
        z = torch.where(o, eps * torch.exp(0.5 * lv) + m, 0.0)
        logw = torch.where(o, 0.5 * ((eps - z) * (eps + z) + lv), 0.0).sum((1, 2), dtype=torch.float64)
        lp = score_tokens(model, z, rep(src_mask), rep(dconds), rep(ys), pad_id=PAD)[0]
        a_[i0:i1, k0:k1] = (lp.double() + logw).view(-1, Kc)
    return (torch.logsumexp(a_, 1) - math.log(K)).float()


def timed_once(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


for K in (16, 64):
    x, y = ours(K), composed(K)                                              # warm-up
    print(f"K = {K}: {n} molecules, {n * K} decoder rows in blocks of {CH}; mean IWAE bound {float(x.mean()):.2f} (device "
          f"draws) / {float(y.mean()):.2f} (torch draws), nats per molecule", flush=True)
    to, tc = [], []
    for r in range(3):
        to.append(timed_once(lambda: ours(K))[1])
        tc.append(timed_once(lambda: composed(K))[1])
        print(f"rep {r}: marginal_logp {to[-1] * 1e3:8.1f} ms -> {n / to[-1]:7.0f} molecules/s | composed in torch "
              f"{tc[-1] * 1e3:8.1f} ms -> {n / tc[-1]:7.0f} molecules/s", flush=True)
    print(f"K = {K}: marginal_logp {n / min(to):.0f} molecules/s, composed in torch {n / min(tc):.0f} molecules/s (best of 3 "
          f"each; time ratio {min(tc) / min(to):.2f})", flush=True)
