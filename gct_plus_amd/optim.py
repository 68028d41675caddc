"""Fused Adam (K8) with a torch.optim.Adam-compatible state_dict.

train1.py:116-119 of the reference builds torch.optim.Adam(lr=1e-4, betas=(0.9,0.98),
eps=1e-9) and Train/trainer1.py:33-46 checkpoints optimizer.state_dict(); resume
(train1.py:125-129) loads it back.  This class keeps that layout -- state[p] = {step,
exp_avg, exp_avg_sq}, param_groups with torch's keys, indexed in parameters() order -- while
the update itself is ONE launch of gct_adam_step over the model's flat parameter / gradient /
moment buffers (28 B of HBM traffic per parameter).

max_grad_norm (None: off) clips by the global L2 norm with torch.nn.utils.clip_grad_norm_'s rule, on the device:
gct_grad_norm reads the flat gradient buffer once more (4 B per parameter, two launches) and leaves
norm = ||grad_scale * g||, coef = min(1, max_grad_norm / (norm + 1e-6)) and running counters in `clip_state`; the Adam
launch then consumes grad_scale * g * coef.  The gradients themselves are not rewritten and nothing returns to the
host: grad_norm_stats() is the one call that synchronises.  One difference from torch: a norm that is not finite skips
the step on the device -- parameters and moments stay bit-unchanged.  Such a skipped step still advances the host's
step count t (the bias correction of the steps after it), exactly as a step skipped by the row guard of
ops.adam_step does.  The setting is not part of state_dict(): the checkpoint layout stays torch Adam's."""
from __future__ import annotations

import math
import numbers

import torch

from . import ops

_F32_MAX = 3.4028234663852886e38


def check_max_grad_norm(value, what="max_grad_norm"):
    """None (off) or a finite number > 0 that fp32 holds, as a float; anything else: ValueError."""
    if value is None:
        return None
    if (isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value)
            or not 0 < value <= _F32_MAX):
        raise ValueError(f"{what} must be None or a finite number > 0, got {value!r}")
    return float(value)


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, model=None, max_grad_norm=None):
        max_grad_norm = check_max_grad_norm(max_grad_norm)
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False)
        super().__init__(params, defaults)
        self.model = model
        self.grad_scale = 1.0          # 1/W when gradients arrive SUM-reduced (see dp.py)
        self.max_grad_norm = max_grad_norm
        self.clip_state = None         # device tensor, 8 words (ops.grad_norm); allocated at the first clipped step
        self._clip_ws = None           # (flat gradient buffer it was sized for, slab of fp64 partials)
        self._flat = None
        self._t = 0

    # ---- gradient-norm clipping ------------------------------------------------------
    def _clip_state_on(self, device):
        if self.clip_state is None or self.clip_state.device != device:
            self.clip_state = ops.new_clip_state(device)
        return self.clip_state

    def _flat_grad_norm(self, g, max_norm):
        state = self._clip_state_on(g.device)
        if self._clip_ws is None or self._clip_ws[0] is not g:
            self._clip_ws = (g, ops.grad_norm_ws(g.numel(), g.device))
        ops.grad_norm(g, state, self._clip_ws[1], max_norm, self.grad_scale)
        return state

    def _generic_grad_norm(self, grads, max_norm):
        """The state of ops.grad_norm written with torch ops (fp64 sum of squares; no host read)."""
        state = self._clip_state_on(grads[0].device)
        words = state.view(torch.int32)
        norm_d = abs(float(self.grad_scale)) * torch.stack([g.double().pow(2).sum() for g in grads]).sum().sqrt()
        norm = norm_d.float()
        finite = torch.isfinite(norm)
        coef = torch.where(finite, (max_norm / (norm_d + 1e-6)).clamp(max=1.0).float(), torch.zeros_like(norm))
        state[0], state[1] = norm, coef
        words[2] = (~finite).int()
        words[3] += 1
        words[4] += (finite & (coef < 1)).int()
        words[5] += (~finite).int()
        state[6] = torch.where(finite, torch.maximum(state[6], norm), state[6])
        return state

    def grad_norm_stats(self, reset=False):
        """dict(norm, coef, steps, clipped_steps, nonfinite_steps, max_norm) read from clip_state in ONE transfer (the
        only synchronising call of the clipping path): norm / coef of the latest step (pre-clip, of the scaled
        gradient; coef 0: skipped as non-finite), the three counts and max_norm, the largest finite norm, since the
        last reset.  reset=True zeroes those running totals afterwards."""
        if self.clip_state is None:
            return dict(norm=0.0, coef=1.0, steps=0, clipped_steps=0, nonfinite_steps=0, max_norm=0.0)
        host = self.clip_state.cpu()
        f, i = host.tolist(), host.view(torch.int32).tolist()
        if reset:
            self.clip_state[3:7].zero_()
        return dict(norm=f[0], coef=f[1], steps=i[3], clipped_steps=i[4], nonfinite_steps=i[5], max_norm=f[6])

    # ---- flat fast path --------------------------------------------------------------
    def _try_flat(self):
        m = self.model
        if m is None or getattr(m, "_gct_flat", None) is None or len(self.param_groups) != 1:
            return None
        order = m._gct_flat["order"]
        mine = self.param_groups[0]["params"]
        if len(order) != len(mine) or any(a is not b for a, b in zip(order, mine)):
            return None
        if self._flat is None or self._flat["pbuf"] is not m._gct_flat["params"]:
            n = m._gct_flat["numel"]
            dev = m._gct_flat["params"].device
            ea = torch.zeros(n, dtype=torch.float32, device=dev)
            es = torch.zeros(n, dtype=torch.float32, device=dev)
            for p, o in zip(order, m._gct_flat["offsets"]):
                st = self.state[p]
                va, vs = ea[o:o + p.numel()].view(p.shape), es[o:o + p.numel()].view(p.shape)
                if "exp_avg" in st:                   # adopt loaded / earlier state
                    va.copy_(st["exp_avg"])
                    vs.copy_(st["exp_avg_sq"])
                    self._t = max(self._t, int(float(st["step"])))
                st["exp_avg"], st["exp_avg_sq"] = va, vs
                st.setdefault("step", torch.tensor(float(self._t)))
            self._flat = {"pbuf": m._gct_flat["params"], "m": ea, "v": es}
        return self._flat

    @torch.no_grad()
    def step(self, closure=None):
        max_norm = check_max_grad_norm(self.max_grad_norm)     # before any device work
        loss = closure() if closure is not None else None
        flat = self._try_flat()
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        if flat is not None:
            self.model.sync_grads_to_flat()
            self._t += 1
            grads = self.model.flat_grads()
            clip = None if max_norm is None else self._flat_grad_norm(grads, max_norm)
            ops.adam_step(flat["pbuf"], grads, flat["m"], flat["v"],
                          float(g["lr"]), b1, b2, g["eps"], self._t, self.grad_scale, clip_state=clip)
            self.model.invalidate_weight_planes()      # bf16 planes are re-split at the next forward
            step_t = torch.tensor(float(self._t))
            for p in g["params"]:
                self.state[p]["step"] = step_t
            return loss
        # generic path: one launch per parameter tensor (non-flattened models)
        clip = None
        if max_norm is not None:
            grads = [p.grad for group in self.param_groups for p in group["params"] if p.grad is not None]
            if grads:
                clip = self._generic_grad_norm(grads, max_norm)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                t = int(float(st["step"])) + 1
                st["step"] = torch.tensor(float(t))
                ops.adam_step(p.data, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"],
                              float(group["lr"]), b1, b2, group["eps"], t, self.grad_scale, clip_state=clip)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat = None                              # re-adopt the loaded moments lazily
        steps = [int(float(s["step"])) for s in self.state.values() if "step" in s]
        self._t = max(steps) if steps else 0
