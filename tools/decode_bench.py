#!/usr/bin/env python3
"""Decoded SMILES/s (BASELINE config 5 shape: pscavaetf-style decode, batch 512, max_strlen 80):
KV-cached decode (eager and graph replay) vs the reference-style full re-run loop.
--beam K: beam search of n samples x K beams against greedy decode of the same n*K rows (ms per token step, SMILES/s),
ids checked against reference_style_beam_decode on the first --ref-n samples.
--scaffolds K [--per-scaffold M]: K scaffold prefixes (<sos> scaffold <sep>, 3..30 tokens) x M rows each, greedy with
graph replay, decoded SMILES/s of three schedules of the same rows: one batch per scaffold (chunks of <= 512 rows, the
reference's per-scaffold sampling loop), one batch per prefix length (host-side grouping), and ONE mixed-prefix batch
(KVDecoder.generate(prefix_lens=)); plus a uniform-prefix batch of the same n at the mean prefix length for scale.  The
mixed batch's ids are checked against the per-length runs first.
--top-k K / --top-p P / --temperature T: filtered multinomial sampling against plain multinomial on the same rows (ms per
token step and SMILES/s, eager and graph replay, all 79 steps).
--stream-rows R --pool N: continuous batching (KVDecoder.generate_stream) of a pool of N items through R rows against
the plain path on the same items: chunks of R items in pool order through start + generate.  Lengths are imposed
(eos_id = -1, caps clip(round(N(35, 8)), 15, 78) + 1 from numpy default_rng(0)), so both legs do known work: the stream
gets them as max_new_tokens, a plain chunk runs max_strlen = its longest cap + 1 (the best its early stop could do).
The stream's step count must equal stream_schedule_reference's (exit status 1 otherwise).  The two legs alternate three
times (start / start_stream inside the timing); printed: steps, ms per step of both and of the plain mixed-prefix
(ragged) step at R rows, SMILES/s, their ratio next to the ratio of the step counts, the replay guard's verdicts.
--prefix T gives every item a T-token prefix (the scaffold models' <sos> scaffold <sep>)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gct_plus_amd import synthetic  # noqa: E402
from gct_plus_amd.Model import model_dict  # noqa: E402
from gct_plus_amd.decode import KVDecoder, reference_style_beam_decode, reference_style_decode  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--model-type", default="vaetf")
ap.add_argument("--ref-n", type=int, default=64, help="batch for the (slow) reference-style loop")
ap.add_argument("--ragged", action="store_true", help="latent length 80 with MOSES-like valid lengths N(35,8) (padded "
                "memory, as Inference/*_sampling.py batches it) instead of 40 fully valid positions")
ap.add_argument("--beam", type=int, default=0, help="beam search with K beams per sample (see the docstring)")
ap.add_argument("--scaffolds", type=int, default=0, help="mixed-scaffold schedules over K scaffolds (see the docstring)")
ap.add_argument("--per-scaffold", type=int, default=64, help="rows per scaffold with --scaffolds")
ap.add_argument("--top-k", type=int, default=None, help="filtered multinomial: top-k (see the docstring)")
ap.add_argument("--top-p", type=float, default=None, help="filtered multinomial: nucleus mass")
ap.add_argument("--temperature", type=float, default=1.0, help="filtered multinomial: temperature")
ap.add_argument("--stream-rows", type=int, default=0, help="continuous batching with R decode rows (see the docstring)")
ap.add_argument("--pool", type=int, default=8192, help="items of the pool with --stream-rows")
ap.add_argument("--prefix", type=int, default=1, help="prefix tokens per item with --stream-rows")
ap.add_argument("--eager", action="store_true", help="--stream-rows: eager launches instead of graph replay")
a = ap.parse_args()
mtype = a.model_type
vs, vt = synthetic.vocab_sizes(mtype)
nc = synthetic.n_conds(mtype)
torch.manual_seed(1)
model = model_dict[mtype](vs, vt, N=6, d_model=512, dff=2048, h=8, latent_dim=128, dropout=0.1, nconds=nc,
                          use_cond2lat=True).cuda().eval()
n, Le = (a.pool if a.stream_rows else a.n), (80 if a.ragged else 40) + nc
z = torch.randn(n, Le, 128, device="cuda")
dconds = torch.randn(n, nc, device="cuda") if nc else None
src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
if a.ragged:
    lens = (torch.randn(n, device="cuda") * 8 + 35).round().clamp(15, 80).long() + nc
    src_mask = (torch.arange(Le, device="cuda")[None, :] < lens[:, None]).unsqueeze(1)
ys0 = torch.full((n, 1), synthetic.SOS_ID, dtype=torch.long, device="cuda")


def timed(run):
    run()                                                                  # warm-up / capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def timed_once(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


if a.stream_rows:
    import numpy as np
    from gct_plus_amd.decode import stream_schedule_reference
    R, N, t0, graphs = a.stream_rows, n, a.prefix, not a.eager
    caps = torch.from_numpy(np.clip(np.rint(np.random.default_rng(0).normal(35, 8, N)), 15, 78).astype(np.int64) + 1)
    if t0 > 1:
        g = torch.Generator().manual_seed(5)
        pre = torch.cat([torch.tensor([synthetic.SOS_ID]), torch.randint(5, 30, (t0 - 2,), generator=g), torch.tensor([4])])
        ys0 = pre.view(1, -1).repeat(N, 1).cuda()
    total = t0 + 79
    _, _, want = stream_schedule_reference(t0 + caps - 1, R)
    chunks = [(lo, min(lo + R, N)) for lo in range(0, N, R)]
    plain_steps = sum(int(caps[lo:hi].max()) for lo, hi in chunks)          # a chunk's prefill counted as one step
    ks = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)
    kp = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)
    kr = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)
    cut = lambda x, lo, hi: None if x is None else x[lo:hi]                  # noqa: E731

    def stream():
        ks.start_stream(z, src_mask, dconds, rows=R, max_total_len=total)
        return ks.generate_stream(ys0, 80, max_new_tokens=caps, use_graphs=graphs)[1]

    def plain():
        for lo, hi in chunks:
            kp.start(z[lo:hi], src_mask[lo:hi], cut(dconds, lo, hi), max_total_len=total)
            kp.generate(ys0[lo:hi], int(caps[lo:hi].max()) + 1, use_graphs=graphs, check_every=0)

    def ragged_step():                                                       # the plain mixed-prefix step at R rows
        m = min(R, N)
        y2 = torch.cat([ys0[:m], ys0[:m, -1:]], dim=1)
        kr.start(z[:m], src_mask[:m], cut(dconds, 0, m), max_total_len=total + 1)
        kr.generate(y2, 80, use_graphs=graphs, check_every=0, prefix_lens=t0 + torch.arange(m) % 2)

    print(f"pool {N} items, {R} rows, prefix {t0}, caps {int(caps.min())}..{int(caps.max())} (mean "
          f"{float(caps.float().mean()):.1f}); steps: stream {want} (schedule reference), plain {plain_steps} in "
          f"{len(chunks)} chunks -> predicted ratio {plain_steps / want:.3f}", flush=True)
    ts, tp, tr, ok = [], [], [], True
    stream(); plain(); ragged_step()                                         # warm-up / capture          # noqa: E702
    for rep in range(3):
        rec, dt = timed_once(stream)
        ts.append(dt)
        ok &= rec["steps"] == want and rec["harvested"] == N and bool((rec["out_len"] == caps).all())
        _, dt = timed_once(plain)
        tp.append(dt)
        _, dt = timed_once(ragged_step)
        tr.append(dt)
        print(f"rep {rep}: stream {ts[-1] * 1e3:8.1f} ms ({rec['steps']} steps, {rec['launched']} launched, "
              f"{ts[-1] / rec['launched'] * 1e3:.3f} ms/step) -> {N / ts[-1]:7.0f} SMILES/s | plain {tp[-1] * 1e3:8.1f} ms "
              f"({tp[-1] / plain_steps * 1e3:.3f} ms/step) -> {N / tp[-1]:7.0f} SMILES/s | ragged step at {min(R, N)} rows "
              f"{tr[-1] / 79 * 1e3:.3f} ms", flush=True)
    bs, bp = min(ts), min(tp)
    print(f"stream / plain SMILES/s {bp / bs:.3f} (step counts predict {plain_steps / want:.3f}); stream step / ragged step "
          f"{(bs / rec['launched']) / (min(tr) / 79):.3f}; plain spread {(max(tp) - min(tp)) / min(tp):.3f}; replay: stream "
          f"{'graph' if graphs and ks.graph_replay else 'eager'}, plain {'graph' if graphs and kp.graph_replay else 'eager'}")
    print("step count equals the schedule reference:", ok)
    sys.exit(0 if ok else 1)

if a.scaffolds:
    from gct_plus_amd.decode import generated_tokens
    K, M = a.scaffolds, a.per_scaffold
    n = K * M
    g = torch.Generator().manual_seed(5)
    t0s = torch.randint(3, 31, (K,), generator=g)                          # prefix lengths <sos> + scaffold + <sep>
    pres = [torch.cat([torch.tensor([synthetic.SOS_ID]), torch.randint(5, 30, (int(t) - 2,), generator=g),
                       torch.tensor([4])]) for t in t0s]
    lens = t0s.repeat_interleave(M)                                          # rows scaffold-major
    ys0 = torch.full((n, int(t0s.max())), synthetic.PAD_ID, dtype=torch.long)
    for r in range(n):
        ys0[r, :int(lens[r])] = pres[r // M]
    ys0 = ys0.cuda()
    z = torch.randn(n, Le, 128, generator=g).cuda()
    dconds = torch.randn(n, nc, generator=g).cuda() if nc else None
    src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
    sub = lambda x, i: None if x is None else x[i]                           # noqa: E731
    decs = {}

    def run_batches(name, batches):
        """batches: [(row idx, prefix length)]; one KVDecoder per schedule, greedy, graph replay, all 79 steps."""
        kd = decs.setdefault(name, KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1))
        gen = torch.empty(n, 79, dtype=torch.long, device="cuda")
        for idx, t0 in batches:
            kd.start(z[idx], src_mask[idx], sub(dconds, idx), max_total_len=112)
            ys = kd.generate(ys0[idx, :t0], 80, use_graphs=True, check_every=0)
            gen[idx] = ys[:, t0:]
        return gen

    def run_mixed():
        kd = decs.setdefault("mixed", KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1))
        kd.start(z, src_mask, dconds, max_total_len=112)
        return generated_tokens(kd.generate(ys0, 80, use_graphs=True, check_every=0, prefix_lens=lens), lens)

    rows = torch.arange(n, device="cuda")
    per_sca = [(rows[s * M + c:s * M + min(c + 512, M)], int(t0s[s])) for s in range(K) for c in range(0, M, 512)]
    per_len = [(rows[(lens == t).cuda()], int(t)) for t in torch.unique(lens).tolist()]
    tu = int(round(float(lens.float().mean())))
    uniform = [(rows, tu)]
    print(f"{K} scaffolds x {M} rows = {n} rows, prefix lengths {int(t0s.min())}..{int(t0s.max())} "
          f"(mean {float(lens.float().mean()):.1f}), {len(per_sca)} per-scaffold batches, {len(per_len)} length groups",
          flush=True)
    g_len = run_batches("per_length", per_len)
    g_mix = run_mixed()
    same = (g_len == g_mix).all(1)
    print(f"mixed batch ids equal to the per-length runs: {int(same.sum())}/{n} rows", flush=True)
    res = {}
    for name, fn in (("per_scaffold", lambda: run_batches("per_scaffold", per_sca)),
                     ("per_length", lambda: run_batches("per_length", per_len)),
                     ("mixed", run_mixed),
                     (f"uniform_t0={tu}", lambda: run_batches("uniform", uniform))):
        _, dt = timed(fn)
        res[name] = n / dt
        print(f"{name:>16}: {dt * 1e3:8.1f} ms -> {n / dt:7.0f} SMILES/s", flush=True)
    print(f"mixed / uniform {res['mixed'] / res[f'uniform_t0={tu}']:.3f}, mixed / per-scaffold "
          f"{res['mixed'] / res['per_scaffold']:.2f}x, mixed / per-length {res['mixed'] / res['per_length']:.2f}x")
    sys.exit(0 if bool(same.all()) else 1)

if a.top_k is not None or a.top_p is not None or a.temperature != 1.0:
    filt = dict(top_k=a.top_k, top_p=a.top_p, temperature=a.temperature)
    kd = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)   # never stop early: worst case
    for graphs in (False, True):
        res = {}
        for name, kw in (("multinomial", {}), ("filtered", filt)):
            def run():
                kd.start(z, src_mask, dconds, max_total_len=96)
                return kd.generate(ys0, 80, algo="multinomial", seed=5, use_graphs=graphs, check_every=0, **kw)
            ys, dt = timed(run)
            res[name] = dt
            print(f"graphs={graphs}: {name:>11} n={n} {dt / 79 * 1e3:.3f} ms/step ({n / dt:.0f} SMILES/s)", flush=True)
        print(f"graphs={graphs}: filtered / multinomial step {res['filtered'] / res['multinomial']:.3f} "
              f"({', '.join(f'{k}={v}' for k, v in filt.items())})", flush=True)
    sys.exit(0)

if a.beam:
    k = a.beam
    rep = lambda x: None if x is None else x.repeat_interleave(k, 0)     # noqa: E731
    kg = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)   # never stop early: worst case
    kb = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)
    for graphs in (False, True):
        def greedy():
            kg.start(rep(z), rep(src_mask), rep(dconds), max_total_len=96)
            return kg.generate(rep(ys0), 80, use_graphs=graphs, check_every=0)

        def beam():
            kb.start(z, src_mask, dconds, max_total_len=96, beams=k)
            return kb.generate_beam(ys0, k, 80, use_graphs=graphs, check_every=0)
        _, tg = timed(greedy)
        (ys, scores, _), tb = timed(beam)
        print(f"graphs={graphs}: greedy n={n * k} rows {tg / 79 * 1e3:.3f} ms/step ({n * k / tg:.0f} SMILES/s) | "
              f"beam {n} x {k} {tb / 79 * 1e3:.3f} ms/step ({n / tb:.0f} SMILES/s) | beam/greedy {tb / tg:.3f}",
              flush=True)
    m = min(a.ref_n, n)
    if m:
        ref, rsc, _ = reference_style_beam_decode(model, z[:m], src_mask[:m], None if dconds is None else dconds[:m],
                                                  ys0[:m], synthetic.PAD_ID, -1, k, 80)
        print("beam token ids equal:", bool(torch.equal(ref, ys[:m])),
              f"max score diff {float((rsc - scores[:m]).abs().max()):.2e}")
    sys.exit(0)

kd = KVDecoder(model, synthetic.PAD_ID, synthetic.SOS_ID, eos_id=-1)       # never stop early: worst case
for graphs in (False, True):
    kd.start(z, src_mask, dconds, max_total_len=96)
    kd.generate(ys0, 80, use_graphs=graphs, check_every=0)                 # warm-up / capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kd.start(z, src_mask, dconds, max_total_len=96)                        # prefill of the cross K/V is inside
    ys = kd.generate(ys0, 80, use_graphs=graphs, check_every=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"kv-cached decode graphs={graphs}: n={n} 79 steps {dt*1e3:.1f} ms -> {n/dt:.0f} SMILES/s "
          f"({dt/79*1e3:.2f} ms/step)", flush=True)
m = a.ref_n
torch.cuda.synchronize()
t0 = time.perf_counter()
ref = reference_style_decode(model, z[:m], src_mask[:m], None if dconds is None else dconds[:m], ys0[:m],
                             synthetic.PAD_ID, -1, 80)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"reference-style full re-run (same kernels, no cache): n={m} {dt*1e3:.1f} ms -> {m/dt:.0f} SMILES/s")
print("token ids equal:", bool(torch.equal(ref, ys[:m])))
