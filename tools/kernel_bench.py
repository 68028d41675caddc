#!/usr/bin/env python3
"""Micro-benchmarks of the hot kernels at the BASELINE shapes (B=512): per-shape time and
TFLOP/s (GEMMs) or GB/s (bandwidth kernels), HIP-event timed, interleaved rounds."""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gct_plus_amd import ops  # noqa: E402


def timeit(fn, reps=10, warm=3):
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
    return ts[len(ts) // 2], ts[0]


GEMM_MODES = {"f32": ops.GEMM_F32, "x6": ops.GEMM_BF16X6, "x3": ops.GEMM_BF16X3}


def gemm_suite(reps, only=None, modes=None, rounds=3):
    """modes: names of GEMM_MODES to time (None: the process mode).  With several, every call is timed in each mode in
    `rounds` interleaved rounds (median of `reps` per round) and the line gives the median over rounds and their spread."""
    dev = "cuda"
    shapes = [("qkv", 40960, 512, 512, 3), ("out", 40960, 512, 512, 1), ("ffn1", 40960, 512, 2048, 1),
              ("ffn2", 40960, 2048, 512, 1), ("kv", 40960, 512, 512, 2), ("mulv", 40960, 512, 128, 2),
              ("sq4k", 4096, 4096, 4096, 1)]
    for name, M, K, nper, nseg in shapes:
        if only and name not in only:
            continue
        N = nper * nseg
        x = torch.randn(M, K, device=dev)
        wflat = torch.randn(nseg * nper * K, device=dev) * K ** -0.5      # one buffer, as flat.py lays weights out
        ws = [wflat[s * nper * K:(s + 1) * nper * K].view(nper, K) for s in range(nseg)]
        ops.register_planes(wflat, ops.split_planes(wflat))   # read in the bf16 modes only (both use the same planes)
        bs = [torch.randn(nper, device=dev) for _ in range(nseg)]
        y = torch.empty(M, N, device=dev)
        outs = [y[:, s * nper:] for s in range(nseg)]
        dy = torch.randn(M, N, device=dev)
        dys = [dy[:, s * nper:] for s in range(nseg)]
        dx = torch.empty(M, K, device=dev)
        dws = [torch.empty(nper, K, device=dev) for _ in range(nseg)]
        dbs = [torch.empty(nper, device=dev) for _ in range(nseg)]
        fl = 2.0 * M * K * N
        for kind, fn in (("fwd", lambda: ops.linear_fwd(x, ws, bs, outs, N)),
                         ("dgrad", lambda: ops.linear_dgrad(dys, N, M, ws, dx)),
                         ("wgrad", lambda: ops.linear_wgrad(dys, N, x, dws, dbs))):
            if not modes:
                med, best = timeit(fn, reps)
                print(f"gemm {name:5s} {kind:5s} M={M} K={K} N={N}: {med*1e6:8.1f} us  {fl/med/1e12:6.1f} TF  (best {fl/best/1e12:6.1f})",
                      flush=True)
                continue
            keep = ops.gemm_get_mode()
            per = {m: [] for m in modes}
            for _ in range(rounds):
                for m in modes:
                    ops.gemm_set_mode(GEMM_MODES[m])
                    per[m].append(timeit(fn, reps)[0])
            ops.gemm_set_mode(keep)
            for m in modes:
                ts = sorted(per[m])
                med = ts[len(ts) // 2]
                print(f"gemm {name:5s} {kind:5s} {m:3s} M={M} K={K} N={N}: {med*1e6:8.1f} us  {fl/med/1e12:6.1f} TF  "
                      f"(rounds {ts[0]*1e6:.1f}..{ts[-1]*1e6:.1f} us)", flush=True)
            if len(modes) > 1:
                meds = {m: sorted(per[m])[rounds // 2] for m in modes}
                print(f"gemm {name:5s} {kind:5s} " + "  ".join(f"{m}/{modes[0]} {meds[m] / meds[modes[0]]:.3f}"
                                                              for m in modes[1:]), flush=True)


def bwdpair_suite(reps, rounds=5):
    """One Linear's backward as gct_linear_bwd's paired launch against the two separate calls (ops.PAIR_BWD off), the two
    ways alternated call by call in one process: the five Linear shapes of a layer at the headline's dense and compact
    row counts, with the dgrad epilogues the training step uses.  Also the separate wgrad / dgrad times (the planner's
    model constants are fitted to them) and the planner's own figures."""
    dev = "cuda"
    shapes = [("out", 512, 512, 1, ops.DEPI_STORE), ("qkv", 512, 512, 3, ops.DEPI_ACCUM), ("q", 512, 512, 1, ops.DEPI_ACCUM),
              ("kv", 512, 512, 2, ops.DEPI_STORE), ("ffn2", 2048, 512, 1, ops.DEPI_MUL_SAVED),
              ("ffn1", 512, 2048, 1, ops.DEPI_ACCUM)]
    keep = ops.PAIR_BWD
    for M in (40960, 18016, 10432):
        for name, K, nper, nseg, depi in shapes:
            N = nper * nseg
            x = torch.randn(M, K, device=dev)
            wflat = torch.randn(N * K, device=dev) * K ** -0.5
            ws = [wflat[s * nper * K:(s + 1) * nper * K].view(nper, K) for s in range(nseg)]
            ops.register_planes(wflat, ops.split_planes(wflat))
            dy = torch.randn(M, N, device=dev)
            dys = [dy[:, s * nper:] for s in range(nseg)]
            dx = torch.zeros(M, K, device=dev)
            pre = torch.randn(M, K, device=dev) if depi == ops.DEPI_MUL_SAVED else None
            dws = [torch.empty(nper, K, device=dev) for _ in range(nseg)]
            dbs = [torch.empty(nper, device=dev) for _ in range(nseg)]
            kw = dict(depi=depi, pre=pre, p=0.1, seed=3, site=1)

            def both(pair):
                ops.PAIR_BWD = pair
                ops.linear_bwd(dys, N, x, ws, dws, dbs, dx, **kw)

            route = ops.linear_bwd_route(M, nseg, nper, K, N, K, K, K, depi)
            sep_route = ops.wgrad_route(M, nseg, nper, K, N, K)
            per = {False: [], True: []}
            for _ in range(rounds):
                for pair in (False, True):
                    per[pair].append(timeit(lambda: both(pair), reps)[0])
            tw = timeit(lambda: ops.linear_wgrad(dys, N, x, dws, dbs), reps)[0]
            td = timeit(lambda: ops.linear_dgrad(dys, N, M, ws, dx, **kw), reps)[0]
            ops.PAIR_BWD = keep
            sep, pr = sorted(per[False]), sorted(per[True])
            ms, mp = sep[rounds // 2], pr[rounds // 2]
            print(f"bwdpair {name:5s} M={M} K={K} N={N} depi={depi}: separate {ms*1e6:7.1f} us ({sep[0]*1e6:.1f}..{sep[-1]*1e6:.1f})  "
                  f"linear_bwd {mp*1e6:7.1f} us ({pr[0]*1e6:.1f}..{pr[-1]*1e6:.1f})  ratio {mp/ms:.3f}  "
                  f"[wgrad alone {tw*1e6:.1f} us s={sep_route[1]}, dgrad alone {td*1e6:.1f} us]  "
                  f"plan paired={route[0]} s={route[1]} rows={route[2]} blocks={route[4]}+{route[5]} "
                  f"model pair {route[6]:.1f} separate {route[7]:.1f} K-tiles", flush=True)


def kvfold_suite(reps, rounds=5):
    """Cross-attention K | V of one decoder layer from the 512-wide memory e (today: forward, dgrad + wgrad pair with
    K = 512) against the same from the 128-wide latent rows z through A = W_kv W_z (folded: K = 128 forward, a 128-wide
    dgrad with accumulate, a weight gradient whose X operand is 128 wide), alternated call by call in one process at
    the headline's and fixed_len_80's memory row counts.  Also the pieces of the folded backward on their own: the
    dgrad, the weight gradient as it stands and with the roles swapped (P^T = z^T dkv: the 128 side as the tile's 128
    rows), and what the planner chose for each."""
    dev = "cuda"
    d, lat = 512, 128
    N = 2 * d
    for M in (18432, 40960):
        e, z = torch.randn(M, d, device=dev), torch.randn(M, lat, device=dev)
        wf, af = torch.randn(N * d, device=dev) * d ** -0.5, torch.randn(N * lat, device=dev) * lat ** -0.5
        ops.register_planes(wf, ops.split_planes(wf))
        ops.register_planes(af, ops.split_planes(af))
        W = [wf[s * d * d:(s + 1) * d * d].view(d, d) for s in range(2)]
        A = [af[s * d * lat:(s + 1) * d * lat].view(d, lat) for s in range(2)]
        bs = [torch.randn(d, device=dev) for _ in range(2)]
        kvb = torch.empty(M, N, device=dev)
        outs = [kvb, kvb[:, d:]]
        dkv = torch.randn(M, N, device=dev)
        dys = [dkv, dkv[:, d:]]
        de, dz = torch.zeros(M, d, device=dev), torch.zeros(M, lat, device=dev)
        dW, dbs = [torch.empty(d, d, device=dev) for _ in range(2)], [torch.empty(d, device=dev) for _ in range(2)]
        P = [torch.empty(d, lat, device=dev) for _ in range(2)]
        PT = torch.empty(lat, N, device=dev)
        cases = {
            "fwd": (lambda: ops.linear_fwd(e, W, bs, outs, N), lambda: ops.linear_fwd(z, A, bs, outs, N)),
            "bwd": (lambda: ops.linear_bwd(dys, N, e, W, dW, dbs, de, depi=ops.DEPI_ACCUM),
                    lambda: ops.linear_bwd(dys, N, z, A, P, dbs, dz, depi=ops.DEPI_ACCUM)),
        }
        tot = [0.0, 0.0]
        for kind, fns in cases.items():
            per = ([], [])
            for _ in range(rounds):
                for i in (0, 1):
                    per[i].append(timeit(fns[i], reps)[0])
            t = [sorted(p) for p in per]
            m0, m1 = t[0][rounds // 2], t[1][rounds // 2]
            tot[0] += m0
            tot[1] += m1
            print(f"kvfold {kind} Mv={M}: today {m0*1e6:7.1f} us ({t[0][0]*1e6:.1f}..{t[0][-1]*1e6:.1f})  folded {m1*1e6:7.1f} us "
                  f"({t[1][0]*1e6:.1f}..{t[1][-1]*1e6:.1f})  ratio {m1/m0:.3f}", flush=True)
        print(f"kvfold trio Mv={M}: today {tot[0]*1e6:7.1f} us  folded {tot[1]*1e6:7.1f} us  saved per layer "
              f"{(tot[0]-tot[1])*1e6:.1f} us", flush=True)
        td = timeit(lambda: ops.linear_dgrad(dys, N, M, A, dz, depi=ops.DEPI_ACCUM), reps)[0]
        rd = ops.gemm_last_route()
        tw = timeit(lambda: ops.linear_wgrad(dys, N, z, P, dbs), reps)[0]
        ts = timeit(lambda: ops.linear_wgrad([z], lat, dkv, [PT], [None]), reps)[0]
        rf = ops.linear_fwd_route(M, lat, 2, d)
        rp = ops.linear_bwd_route(M, 2, d, lat, N, lat, lat, lat, ops.DEPI_ACCUM)
        rw, rs = ops.wgrad_route(M, 2, d, lat, N, lat), ops.wgrad_route(M, 1, lat, N, lat, N, want_bias=False)
        print(f"kvfold pieces Mv={M}: dgrad N=128 {td*1e6:.1f} us route {rd[0]} launches {rd[5]}; wgrad X 128 wide "
              f"{tw*1e6:.1f} us kind {rw[0]} s={rw[1]}; wgrad roles swapped {ts*1e6:.1f} us kind {rs[0]} s={rs[1]}; "
              f"fwd K=128 route {rf[0]} tail {rf[2]}; pair plan paired={rp[0]} s={rp[1]} blocks={rp[4]}+{rp[5]} "
              f"model pair {rp[6]:.1f} separate {rp[7]:.1f} K-tiles", flush=True)


def decgemm_suite(reps):
    """Forward GEMMs of a KV-cached decode step (n rows) and of small training batches."""
    dev = "cuda"
    for M in (1024, 2048, 4096, 5184):
        for name, K, N in (("out", 512, 512), ("q'", 512, 1024), ("out'", 1024, 512), ("qkv", 512, 1536),
                           ("ffn1", 512, 2048), ("ffn2", 2048, 512)):
            x = torch.randn(M, K, device=dev)
            w = torch.randn(N * K, device=dev) * K ** -0.5
            if ops.gemm_get_mode() != ops.GEMM_F32:
                ops.register_planes(w, ops.split_planes(w))
            b, y = torch.randn(N, device=dev), torch.empty(M, N, device=dev)
            wsb = torch.empty(int(ops._L().gct_linear_fwd_ws_bytes(M, K, N)) // 4 + 64, device=dev)
            med, best = timeit(lambda: ops.linear_fwd(x, [w.view(N, K)], [b], [y], N, ws=wsb), reps)
            fl = 2.0 * M * K * N
            print(f"gemm {name:5s} fwd M={M} K={K} N={N}: {med*1e6:8.1f} us  {fl/med/1e12:6.1f} TF  (best {fl/best/1e12:6.1f})", flush=True)


def epi_suite(reps):
    """What the fused epilogues cost per forward / dgrad GEMM at the training shapes: bias only vs GELU (+ dropout) vs
    dropout + residual, p = 0 against p = 0.1 (the Philox share)."""
    dev = "cuda"
    M = 40960
    for name, K, N in (("out", 512, 512), ("ffn1", 512, 2048), ("ffn2", 2048, 512)):
        x = torch.randn(M, K, device=dev)
        w = torch.randn(N * K, device=dev) * K ** -0.5
        if ops.gemm_get_mode() != ops.GEMM_F32:
            ops.register_planes(w, ops.split_planes(w))
        W = w.view(N, K)
        b, y = torch.randn(N, device=dev), torch.empty(M, N, device=dev)
        resid, pre = torch.randn(M, N, device=dev), torch.empty(M, N, device=dev)
        fl = 2.0 * M * K * N
        cases = [("bias", dict())]
        for p in (0.0, 0.1):
            cases.append((f"gelu_drop p={p}", dict(epi=ops.EPI_GELU_DROP, pre=pre, p=p, seed=3, site=1)))
            cases.append((f"drop_resid p={p}", dict(epi=ops.EPI_DROP_RESID, resid=resid, p=p, seed=3, site=1)))
        for label, kw in cases:
            med, best = timeit(lambda: ops.linear_fwd(x, [W], [b], [y], N, **kw), reps)
            print(f"epi {name:5s} fwd   {label:18s}: {med*1e6:8.1f} us  {fl/med/1e12:6.1f} TF", flush=True)
        dy, dx = torch.randn(M, N, device=dev), torch.empty(M, K, device=dev)
        prek = torch.randn(M, K, device=dev)
        cases = [("store", dict())] + [(f"gelu_bwd p={p}", dict(depi=ops.DEPI_GELU_BWD, pre=prek, p=p, seed=3, site=1))
                                       for p in (0.0, 0.1)]
        for label, kw in cases:
            med, best = timeit(lambda: ops.linear_dgrad([dy], N, M, [W], dx, **kw), reps)
            print(f"epi {name:5s} dgrad {label:18s}: {med*1e6:8.1f} us  {fl/med/1e12:6.1f} TF", flush=True)


def attn_suite(reps, fixed=False):
    dev = "cuda"
    shapes = [("enc", 512, 8, 80, 80, 64, False), ("dec", 512, 8, 81, 81, 64, True), ("cross", 512, 8, 81, 80, 64, False)]
    if os.environ.get("ATTN_LAYOUT_PROBE"):
        # same work per (batch, head) pair, but every pair's q / k / v slice is CONTIGUOUS (H = 1): what the
        # head-sliced 256-B-per-row access of the [M, 3d] projection buffer costs
        shapes = [("enc", 512, 8, 80, 80, 64, False), ("encH1", 4096, 1, 80, 80, 64, False)]
    for name, B, H, Lq, Lk, dk, causal in shapes:
        d = H * dk
        qkv = torch.randn(B * max(Lq, Lk), 3 * d, device=dev)
        # MOSES-like ragged lengths: l ~ N(35,8) clipped to [15, L]
        lens = torch.clamp(torch.round(torch.randn(B, device=dev) * 8 + 35), 15, Lk).long()
        lens[0] = Lk
        if fixed:
            lens[:] = Lk
        pad = (torch.arange(Lk, device=dev)[None, :] < lens[:, None])
        if causal:
            mask = (pad[:, None, :] & torch.ones(Lq, Lk, dtype=torch.bool, device=dev).tril_()[None]).to(torch.uint8).contiguous()
        else:
            mask = pad.to(torch.uint8).contiguous()
        q, k, v = qkv, qkv[:, d:], qkv[:, 2 * d:]
        ld = 3 * d
        if name == "encH1":
            q, k, v = (torch.randn(B * Lq, d, device=dev) for _ in range(3))
            ld = d
        mask = ops.pack_mask(mask, B, Lq, Lk)        # packed once per forward in the engine, not per call
        o, lse, _ = ops.attn_fwd(q, k, v, ld, ld, ld, mask, B, H, Lq, Lk, dk, 0.1, 1, 1)
        do = torch.randn_like(o)
        dqkv = torch.empty_like(qkv)
        dq_, dk__, dv_ = (dqkv, dqkv[:, d:], dqkv[:, 2 * d:]) if name != "encH1" else (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))
        fl = 4.0 * B * H * Lq * Lk * dk
        med, best = timeit(lambda: ops.attn_fwd(q, k, v, ld, ld, ld, mask, B, H, Lq, Lk, dk, 0.1, 1, 1), reps)
        gb = 4.0 * B * max(Lq, Lk) * d * 4
        print(f"attn {name:5s} fwd{' fixed' if fixed else ''}: {med*1e6:8.1f} us  {fl/med/1e12:6.2f} TF  {gb/med/1e9:7.0f} GB/s", flush=True)
        med, best = timeit(lambda: ops.attn_bwd(q, k, v, ld, ld, ld, mask, o, do, lse, dq_, dk__, dv_, ld, ld, ld,
                                                B, H, Lq, Lk, dk, 0.1, 1, 1), reps)
        print(f"attn {name:5s} bwd{' fixed' if fixed else ''}: {med*1e6:8.1f} us  {2.5*fl/med/1e12:6.2f} TF  {2*gb/med/1e9:7.0f} GB/s", flush=True)


def bw_suite(reps):
    dev = "cuda"
    M, d = 40960, 512
    x = torch.randn(M, d, device=dev)
    a, b = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    y, mean, rstd = ops.norm_fwd(x, a, b)
    med, _ = timeit(lambda: ops.norm_fwd(x, a, b, out=y), reps)
    print(f"norm fwd: {med*1e6:7.1f} us {2*M*d*4/med/1e9:7.0f} GB/s", flush=True)
    da, db = torch.empty(d, device=dev), torch.empty(d, device=dev)
    dx = torch.empty_like(x)
    med, _ = timeit(lambda: ops.norm_bwd(y, x, a, mean, rstd, da, db, dres=x, out=dx), reps)
    print(f"norm bwd: {med*1e6:7.1f} us {4*M*d*4/med/1e9:7.0f} GB/s", flush=True)
    n = 44_514_334
    p, g, m, v = (torch.randn(n, device=dev) for _ in range(4))
    v.abs_()
    med, _ = timeit(lambda: ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.98, 1e-9, 3), reps)
    print(f"adam    : {med*1e6:7.1f} us {28*n/med/1e9:7.0f} GB/s", flush=True)
    clip_lines(p, g, m, v, reps)


def clip_lines(p, g, m, v, reps):
    """gct_grad_norm (both launches) and the clipped Adam step as FusedAdam(max_grad_norm=...) issues them: in turn,
    each between its own pair of events, behind an untimed plain Adam launch -- its 1.25 GB push the gradient buffer
    out of the Infinity Cache, as a training step's backward does, and while it runs the host queues the timed
    launches, so the events see the device's time and not the host's launch latency."""
    n = g.numel()
    state, ws = ops.new_clip_state(g.device), ops.grad_norm_ws(n, g.device)
    max_norm = 0.5 * float(g.double().norm())
    tn, ta = [], []
    for it in range(3 + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.98, 1e-9, 3)
        ev[0].record()
        ops.grad_norm(g, state, ws, max_norm)
        ev[1].record()
        ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.98, 1e-9, 3, clip_state=state)
        ev[2].record()
        ev[2].synchronize()
        if it >= 3:
            tn.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            ta.append(ev[1].elapsed_time(ev[2]) * 1e-3)
    tn.sort()
    ta.sort()
    mn, ma = tn[len(tn) // 2], ta[len(ta) // 2]
    print(f"gradnorm: {mn*1e6:7.1f} us {4*n/mn/1e9:7.0f} GB/s", flush=True)
    print(f"adamclip: {ma*1e6:7.1f} us {28*n/ma/1e9:7.0f} GB/s", flush=True)


def adam_suite(reps):
    """The three optimizer lines alone, three alternated rounds."""
    n = 44_514_334
    p, g, m, v = (torch.randn(n, device="cuda") for _ in range(4))
    v.abs_()
    for _ in range(3):
        med, _ = timeit(lambda: ops.adam_step(p, g, m, v, 1e-4, 0.9, 0.98, 1e-9, 3), reps)
        print(f"adam    : {med*1e6:7.1f} us {28*n/med/1e9:7.0f} GB/s", flush=True)
        clip_lines(p, g, m, v, reps)


def kld_suite(reps, rounds=3, batch=20):
    """The KL term of a training step, R = 512 * 64 latent rows of D = 128 (the bench step's order of size): gct_kld_fwd
    + gct_kld_bwd against gct_kld_dims_fwd + gct_kld_dims_bwd (free bits 0.25, every fourth row masked out), alternated,
    next to a device copy that moves the same 24 B per element (the forward reads mu and log_var, the backward reads
    them again and writes two gradients).  `batch` calls between one pair of events: a call is a few microseconds."""
    dev = "cuda"
    B, Le, D = 512, 64, 128
    n = B * Le * D
    mu, lv = torch.randn(B, Le, D, device=dev), torch.randn(B, Le, D, device=dev) * 0.1
    live = (torch.arange(B * Le, device=dev) % 4 != 0).view(B, Le)
    g = torch.tensor(0.04, device=dev)
    src, dst = torch.empty(3 * n, device=dev), torch.empty(3 * n, device=dev)

    def plain():
        ops.kld_fwd(mu, lv)
        ops.kld_bwd(mu, lv, g)

    def dims(mask):
        _, _, gate = ops.kld_dims_fwd(mu, lv, mask, 0.25, B)
        ops.kld_dims_bwd(mu, lv, mask, gate, g)

    variants = (("kld plain        ", plain), ("kld dims         ", lambda: dims(None)),
                ("kld dims + mask  ", lambda: dims(live)), ("copy, same bytes ", lambda: dst.copy_(src)))
    for _ in range(rounds):
        for name, fn in variants:
            def many():
                for _ in range(batch):
                    fn()
            med, best = timeit(many, reps)
            print(f"{name}: {med/batch*1e6:7.2f} us (best {best/batch*1e6:7.2f}) {24*n/(med/batch)/1e9:7.0f} GB/s",
                  flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--suite", default="gemm,attn,bw")
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gemm-mode", default="",
                    help="gemm suite: comma-separated modes to time, interleaved (f32, x6, x3; e.g. x6,x3). "
                         "Default: the process mode")
    a = ap.parse_args()
    gmodes = [m for m in a.gemm_mode.split(",") if m]
    for m in gmodes:
        if m not in GEMM_MODES:
            ap.error(f"--gemm-mode: unknown mode {m!r} (f32, x6, x3)")
    if "gemm" in a.suite.split(","):
        gemm_suite(a.reps, a.only.split(",") if a.only else None, gmodes or None)
    if "decgemm" in a.suite:
        decgemm_suite(a.reps)
    if "bwdpair" in a.suite.split(","):
        bwdpair_suite(a.reps)
    if "kvfold" in a.suite.split(","):
        kvfold_suite(a.reps)
    if "epi" in a.suite.split(","):
        epi_suite(a.reps)
    if "attn" in a.suite:
        attn_suite(a.reps)
        attn_suite(a.reps, fixed=True)
    if "bw" in a.suite:
        bw_suite(a.reps)
    if "adam" in a.suite.split(","):
        adam_suite(a.reps)
    if "kld" in a.suite.split(","):
        kld_suite(a.reps)
