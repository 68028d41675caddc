#!/usr/bin/env python3
"""Whole-step time of the benchmark's training step (bench.py's workload: vaetf 6+6/d512, B=512, dropout 0.1, MOSES-like
lengths, the trainer's forward / backward / FusedAdam step) in bf16x6 and bf16x3 GEMM mode, alternating in one process:
every round runs `--steps` steps per mode between HIP events, after `--warmup` steps of each mode.  Prints ms/step and
SMILES/s per mode (median over rounds, with the round spread) and the x3 / x6 ratio.
  python tools/step_time_modes.py [--rounds 6 --steps 10 --warmup 5]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gct_plus_amd import ops, synthetic  # noqa: E402

MODES = (("x6", ops.GEMM_BF16X6), ("x3", ops.GEMM_BF16X3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10, help="steps per mode and round")
    ap.add_argument("--warmup", type=int, default=5, help="steps per mode before the first round")
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    ba = bench.parse_args(["--gpus", "1", "--batch", str(a.batch)])     # the benchmark's own workload settings
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    inner, opt, fwd_loss = bench.hip_workload(ba, dev, 1, 0)
    ds = synthetic.make_dataset(a.batch * 4, 80, ba.model_type, seed=0, fixed_len=False)
    pool = [{k: v.to(dev) for k, v in b.items()} for b in synthetic.batches(ds, a.batch)]
    it = [0]

    def step():
        i = it[0]
        it[0] += 1
        loss = fwd_loss(pool[i % len(pool)])
        fwd_loss.prefetch(pool[(i + 1) % len(pool)])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    keep = ops.gemm_get_mode()
    ms = {name: [] for name, _ in MODES}
    launches = {name: 0 for name, _ in MODES}
    try:
        for name, mode in MODES:
            ops.gemm_set_mode(mode)
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, mode in MODES:
                ops.gemm_set_mode(mode)
                k3, k6 = ops.gemm_x3_launches(), ops._L().gct_gemm_x6_kernel_launches()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.steps):
                    loss = step()
                e1.record()
                e1.synchronize()
                assert torch.isfinite(loss).item()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
                launches[name] = (ops.gemm_x3_launches() - k3) if mode == ops.GEMM_BF16X3 else \
                    (ops._L().gct_gemm_x6_kernel_launches() - k6)
    finally:
        ops.gemm_set_mode(keep)
    med = {}
    for name, _ in MODES:
        t = ms[name]
        med[name] = statistics.median(t)
        print(f"{name}: {med[name]:7.2f} ms/step  {a.batch / med[name] * 1e3:8.0f} SMILES/s  "
              f"(rounds {min(t):.2f}..{max(t):.2f} ms, {a.rounds} x {a.steps} steps; "
              f"{launches[name] // a.steps} bf16 GEMM kernel launches per step)", flush=True)
    print(f"x3 / x6 step time {med['x3'] / med['x6']:.3f}  (speed-up {med['x6'] / med['x3']:.3f}x)", flush=True)


if __name__ == "__main__":
    main()
