"""Shared references of the sequential Monte Carlo tests (tests/test_smc_host.py, tests/test_smc_gpu.py): the host
restatement of gct_smc_select's two Philox streams over tests/rng_ref.py, written from the comment in
include/gctplus_hip.h and not from the kernel; the toy model with an exactly known answer; and the cases of the selection
kernel's test with their near-tie bounds.  Everything here is computed once, shared, and never written.

The draw streams (one step, token position p, sample s of k particles):
  child c's uniform   = word 0 of Philox4x32-10 at (s*k + c, p, 452821E6, 38D01377) under the key of (seed, site DEC0DE)
                        -- gct_select_token's draw of the physical row s*k + c (rng_ref.select_uniform);
  the resampling one  = word 0 at (s, p, the same two constants) under the key of (seed, site 53C0DE);
  both through u = (float32(x >> 8) + 0.5f) * 2^-24 (rng_ref.draw_uniform_of_word).
"""
import functools
import math

import numpy as np
import torch

from gct_plus_amd import decode as D
from gct_plus_amd.smiles import SmilesGrammar
from tests import rng_ref as R

SMC_SITE = 0x53C0DE


def smc_uniforms(seed, n, k, pos, site=SMC_SITE, word=0):
    """float32 [n, k + 1]: smc_step_reference's uniforms of n samples of k particles at token position pos.  site / word
    exist for the tests that show a wrong site or output word of the resampling stream would be noticed."""
    rows = np.arange(n * k, dtype=np.int64)
    draws = R.select_uniform(seed, rows, np.full(n * k, pos, dtype=np.int64)).reshape(n, k)
    s = np.arange(n, dtype=np.int64)
    words = R.philox4x32_10((s, np.full(n, pos, dtype=np.int64), R.DRAW_C2, R.DRAW_C3), R.rng_key(seed, site))
    return np.concatenate([draws, R.draw_uniform_of_word(words[word]).reshape(n, 1)], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the toy model
# A first-order "model": logits by (generated position, previous token) over 11 tokens -- atoms, a bond, branches, a ring
# digit, the dot, <eos>, <pad> -- under a budget of G = 5 generated tokens.  Small enough to enumerate every string.
TOY_VOCAB = ["<pad>", "<eos>", "C", "N", "c", "O", "=", "(", ")", "1", "."]
TOY_PAD, TOY_EOS, TOY_G = 0, 1, 5
TOY_SEED = 1          # the table's seed (test_smc_host.py states why this one and the margins it gives)
TOY_SCALE = 2.0


class Toy:
    def __init__(self, seed=TOY_SEED):
        self.gr = SmilesGrammar(TOY_VOCAB, TOY_PAD, TOY_EOS)
        V = len(TOY_VOCAB)
        self.V = V
        g = torch.Generator().manual_seed(seed)
        self.table = (torch.randn(TOY_G, V + 1, V, generator=g) * TOY_SCALE).double()     # prev = V: no token yet
        self.table[:, :, TOY_PAD] = -30.0                                       # (a model that has learnt not to pad)
        self.logp = torch.log_softmax(self.table, -1)
        self._mask = {}
        self.strings = {}                                                       # well-formed string -> (pi, q)
        self._enumerate((), 0.0, 0.0)
        self.Z = sum(p for p, _ in self.strings.values())

    def allowed(self, hist):
        if hist not in self._mask:
            keep = torch.zeros(self.V, dtype=torch.bool)
            keep[self.gr.allowed(list(hist), TOY_G - len(hist))] = True
            self._mask[hist] = keep
        return self._mask[hist]

    def _enumerate(self, hist, lp, lq):
        """Depth first over the allowed tokens: lp the model's log-probability of the string, lq its log-probability
        under the locally renormalised sampler (each step divided by the allowed mass A_t)."""
        if hist and hist[-1] == TOY_EOS:
            self.strings[hist] = (math.exp(lp), math.exp(lq))
            return
        row = self.logp[len(hist), hist[-1] if hist else self.V]
        keep = self.allowed(hist)
        logA = float(torch.logsumexp(row[keep], 0))
        for t in torch.nonzero(keep).view(-1).tolist():
            self._enumerate(hist + (t,), lp + float(row[t]), lq + float(row[t]) - logA)

    def rows(self, ys):
        """(logits, masked) fp64 [rows, V] of the token rows ys int64 [rows, g] (pad behind a finished row)."""
        g = ys.shape[1]
        prev = ys[:, -1] if g else torch.full((ys.shape[0],), self.V, dtype=torch.long)
        x = self.table[min(g, TOY_G - 1), prev].clone()
        keep = torch.stack([self.allowed(tuple(h[:h.index(TOY_EOS) + 1] if TOY_EOS in h else h)) for h in ys.tolist()])
        return x, torch.where(keep, x, torch.full_like(x, -math.inf))

    def run(self, N, k, tau, seed):
        """N independent samples of k particles through smc_step_reference (fp64), uniforms from torch's CPU generator
        under `seed`.  Returns SmcSamples with ys [N, k, G] (no prefix)."""
        gen = torch.Generator().manual_seed(seed)
        logw, logp, fin, lens, log_z, res = D.smc_init(N, k)
        logw, logp = logw.double(), logp.double()
        ys = torch.zeros(N * k, 0, dtype=torch.long)
        base = torch.arange(N).view(N, 1) * k
        for _ in range(TOY_G):
            x, y = self.rows(ys)
            u = torch.rand(N, k + 1, generator=gen, dtype=torch.float64).clamp(min=2.0 ** -25)
            anc, tok, logw, logp, fin, lens, log_z, res = D.smc_step_reference(
                logw, logp, fin, lens, x, y, u, k, TOY_PAD, TOY_EOS, tau, log_z, res)
            ys = torch.cat([ys[(base + anc).view(-1)], tok.view(-1, 1)], 1)
        assert bool(fin.all())
        norm, log_z, ess = D.smc_finalize(logw, log_z)
        return D.SmcSamples(ys.view(N, k, -1), norm, logp, log_z, lens, ess, res)


@functools.lru_cache(maxsize=None)
def toy(seed=TOY_SEED):
    return Toy(seed)


def string_of(row):
    row = list(row)
    return tuple(row[:row.index(TOY_EOS) + 1])


# ------------------------------------------------------------------- the cases of the selection kernel's test
# Shared by tests/test_smc_gpu.py (the kernel against the fp64 rules) and tests/test_smc_host.py (the share of the cases
# that sits on a near tie, a condition on the generator that needs no GPU).
KERNEL_KS, KERNEL_VS, KERNEL_TAUS = (1, 3, 16), (30, 64, 301), (0.0, 0.5, 1.0)
KERNEL_N, KERNEL_T, KERNEL_OFF, KERNEL_P = 3, 40, 3, 17          # samples per launch; p = index of the token chosen now
KERNEL_VARIANTS = ("mixed", "edge")
UNDECIDABLE_CAP = 0.25

# How far the device's fp32 evaluation may sit from the fp64 one.  The exponent of a weight, logw + a with a = (my - mx) +
# (log sy - log sx): the maxima are exact; each sum of V <= 301 terms carries a relative error of about 1e-6 (one ulp per
# exp, a six-level wave reduction, V / 64 carries), so each log about 1e-6 absolute, and |a| <= 16 rounds to within 1e-6:
# 4e-6 in all.  A weight exp(logw - M) therefore has a relative error of 4e-6 (plus one ulp of expf).
LOGW_ERR = 4e-6


def ess_bound(k):
    """ESS = S1^2 / S2 is a ratio of four such sums: relative 4 x 4e-6, absolute at most 1.6e-5 k; rounded up to 2e-5 k."""
    return 2e-5 * k


def sys_bound(k):
    """A cumulative sum of at most k weights <= 1 and a systematic position (u + c) S1 / k <= S1 <= k each sit within
    k x 4e-6 of their fp64 values (the k - 1 fp32 additions add 6e-8 k each): 1e-5 k between the two."""
    return 1e-5 * k


# logw: two chained logsumexp per step on top of test_beam_decode_gpu.py's rtol 1e-6 of the value itself; logp: one
# (the raw row's) and the rounding of the sum; log_z gains M + log(S1 / k) from fp32 inputs: M as logw, S1 relative 4e-6.
LOGW_TOL = dict(rtol=1e-6, atol=LOGW_ERR)
LOGP_TOL = dict(rtol=1e-6, atol=2e-6)
LOGZ_TOL = dict(rtol=1e-6, atol=2 * LOGW_ERR)


def kernel_params():
    return [(k, V, tau) for k in KERNEL_KS for V in KERNEL_VS for tau in KERNEL_TAUS]


@functools.lru_cache(maxsize=None)
def kernel_case(k, V, variant, pad_id, eos_id):
    """CPU tensors of one launch: n = 3 samples x k particles over V tokens.
    "mixed": sample 0 all live with spread weights; sample 1 finished particles (every other one), a dead particle
             (its masked row all -inf) and live ones; sample 2 every particle dead.
    "edge":  sample 0 rows with a single allowed token (<eos> for particle 0); sample 1 every particle finished on entry
             (idle); sample 2 live with near-equal weights, so that the thresholds 0.5 k sits far from the ESS."""
    n, T, off, p = KERNEL_N, KERNEL_T, KERNEL_OFF, KERNEL_P
    rows = n * k
    g = torch.Generator().manual_seed(7000 + 100 * k + V + (0 if variant == "mixed" else 50000))
    logits = (torch.randn(rows, V, generator=g) * 3).contiguous()
    hide = torch.rand(rows, V, generator=g) < 0.6
    hide[torch.arange(rows), torch.randint(0, V, (rows,), generator=g)] = False        # every row keeps a token
    hide[:, pad_id] = True
    logw = (torch.randn(n, k, generator=g) * 1.5).float()
    logp = -(torch.rand(n, k, generator=g) * 20).float()
    fin = torch.zeros(n, k, dtype=torch.bool)
    lens = torch.randint(1, p, (n, k), generator=g)
    if variant == "mixed":
        fin[1, ::2] = True
        if k > 1:
            hide[k + 1] = True                                                       # sample 1, particle 1: dead
        hide[2 * k:3 * k] = True                                                      # sample 2: all dead
        logw[1, -1] = -math.inf                                                       # (and one dead since earlier)
        fin[1, -1] = True
    else:
        only = torch.randint(2, V, (k,), generator=g)
        only[0] = eos_id
        hide[0:k] = True
        hide[torch.arange(k), only] = False
        fin[1] = True
        logw[2] = logw[2] * 0.05
    masked = torch.where(hide, torch.full_like(logits, -math.inf), logits)
    ys = torch.randint(2, V, (rows, T - off), generator=g)
    valid = (torch.rand(rows, T, generator=g) < 0.9).to(torch.uint8)
    kv_src = (torch.arange(n).view(n, 1, 1) * k + torch.randint(0, k, (n, k, T), generator=g)).reshape(rows, T).int()
    u = torch.rand(n, k + 1, generator=g).float().clamp(min=2.0 ** -25)
    return dict(logits=logits, masked=masked, logw=logw, logp=logp, fin=fin, lens=lens, ys=ys, valid=valid, kv_src=kv_src,
                u=u, log_z=-torch.rand(n, generator=g).double(), res=torch.randint(0, 5, (n,), generator=g))


def kernel_reference(case, k, tau, pad_id, eos_id):
    """smc_step_reference in fp64 on a case, and which samples are undecidable in fp32: |ESS - tau k| within ess_bound
    (when the threshold decides: 0 < tau < 1), a systematic position within sys_bound of a cumulative boundary, or a
    draw whose uniform lies within decode_step_ref.delta(V) of a boundary of the child's cumulative distribution.
    Returns (outputs of the step, undecidable bool [n])."""
    from tests.decode_step_ref import delta
    info = {}
    out = D.smc_step_reference(case["logw"].double(), case["logp"].double(), case["fin"], case["lens"],
                               case["logits"].double(), case["masked"].double(), case["u"].double(), k, pad_id, eos_id,
                               tau, case["log_z"], case["res"], info=info)
    n, V = case["logw"].shape[0], case["logits"].shape[1]
    weighted = info["ess"] > 0
    und = weighted & (info["ess_margin"] <= ess_bound(k)) & (0.0 < tau < 1.0)
    und |= info["sys_gap"] <= sys_bound(k)
    probs, drew = info["probs"].numpy(), info["drew"].numpy()
    for s in range(n):
        rows = [c for c in range(k) if drew[s, c]]
        if rows:
            gap = R.draw(probs[s, rows], case["u"][s, rows].double().numpy())[1]
            und[s] |= bool((gap <= delta(V)).any())
    return out, und
