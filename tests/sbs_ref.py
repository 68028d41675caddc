"""Host restatement of the Gumbel draw of stochastic beam search: plain numpy over tests/rng_ref.py, written from the
comment of gct_beam_select_gumbel in include/gctplus_hip.h, not from the kernel.

The rule:
  noise of (row r, token position p, token v) = word v & 3 of Philox4x32-10 at the counter (r, p, v >> 2, BE5466CF)
  under the key of (seed, site 5B5BEA); u = (float32(x >> 9) + 0.5f) * 2^-23, exact in float32 and strictly inside
  (0, 1); noise = -log(-log(u)).  r is the PHYSICAL row s*k + b of the decode.
"""
import numpy as np

from tests.rng_ref import _u64, philox4x32_10, rng_key

SBS_SITE = 0x5B5BEA
SBS_C3 = 0xBE5466CF


def sbs_uniform_of_word(x):
    """float32 array: u = (float32(x >> 9) + 0.5f) * 2^-23 -- 23 bits and a half fit a float32, so nothing rounds."""
    hi = (_u64(x) >> _u64(9)).astype(np.float32)
    return (hi + np.float32(0.5)) * np.float32(2.0 ** -23)


def sbs_uniform(seed, rows, pos, V, word_shift=0, swap=False):
    """float32 [len(rows), V]: the uniforms of the rows `rows` (ints) at token position pos.
    word_shift / swap exist for the tests that show a mistake would be noticed: the output word (v + word_shift) & 3
    instead of v & 3; the counter words row and position swapped."""
    r = np.asarray(rows, dtype=np.int64).reshape(-1, 1)
    v = np.arange(V, dtype=np.int64).reshape(1, -1)
    c0, c1 = r + 0 * v, np.int64(pos) + 0 * (r + v)
    if swap:
        c0, c1 = c1, c0
    words = philox4x32_10((c0, c1, (v >> 2) + 0 * r, SBS_C3), rng_key(seed, SBS_SITE))
    x = np.choose(((v + word_shift) & 3) + 0 * r, words)
    return sbs_uniform_of_word(x)


def sbs_noise(seed, rows, pos, V, **kw):
    """float64 [len(rows), V]: the standard Gumbel variates -log(-log(u)), evaluated in float64 on the float32 u."""
    u = sbs_uniform(seed, rows, pos, V, **kw).astype(np.float64)
    return -np.log(-np.log(u))


# ------------------------------------------------------------------- the cases of the selection kernel's test
# Shared by tests/test_sbs_gpu.py (the kernel against the fp64 rules) and tests/test_sbs_host.py (the share of those
# cases that sits on a near tie, a condition on the generator that needs no GPU).
GAP = 1e-3                      # candidate values closer than this may order either way in fp32 (see test_sbs_host.py)
KERNEL_KS, KERNEL_VS = (1, 2, 5, 16), (5, 30, 64, 301, 4096)
KERNEL_N, KERNEL_T, KERNEL_OFF, KERNEL_P = 5, 40, 3, 17          # p = index of the token chosen now (pos = p - 1)


def kernel_cases():
    return [(k, V) for k in KERNEL_KS for V in KERNEL_VS if k <= V]


def kernel_case(k, V, pad_id, eos_id):
    """CPU tensors of one selection: n = 5 samples x k beams over V tokens.  Sample 0: the first expansion after the
    prefill; 1: every beam finished; 2: live and frozen beams mixed; 3: -inf logits on half the tokens of every row;
    4: <eos> certain for beam 0.  Beams are in drawing order (descending Gumbel value), as a decode leaves them."""
    import torch
    from gct_plus_amd.decode import sbs_init
    g = torch.Generator().manual_seed(1000 * k + V)
    n, T = KERNEL_N, KERNEL_T
    rows = n * k
    logits = torch.randn(rows, V, generator=g) * 3
    scores = -torch.rand(n, k, generator=g) * 20
    gum = scores - torch.log(-torch.log(torch.rand(n, k, generator=g).clamp(1e-6, 1 - 1e-6)))
    order = torch.sort(gum, dim=1, descending=True).indices
    scores, gum = scores.gather(1, order), gum.gather(1, order)
    fin = torch.zeros(n, k, dtype=torch.bool)
    lens = torch.randint(1, 15, (n, k), generator=g)
    s0, g0, f0, l0 = sbs_init(1, k)
    scores[0], gum[0], fin[0], lens[0] = s0[0], g0[0], f0[0], l0[0]
    fin[1] = True
    fin[2] = torch.arange(k) % 2 == 1                       # beams 1, 3, ... frozen
    logits[3 * k:4 * k, 0::2] = -float("inf")
    logits[4 * k, eos_id] = 50.0
    noise = -torch.log(-torch.log(torch.rand(rows, V, generator=g).clamp(1e-7, 1 - 1e-7)))
    ys = torch.randint(0, V, (rows, T), generator=g)
    valid = torch.randint(0, 2, (rows, T), generator=g).to(torch.uint8)
    kv_src = torch.randint(0, rows, (rows, T), generator=g).to(torch.int32)
    return dict(logits=logits, scores=scores, gumbels=gum, fin=fin, lens=lens, noise=noise, ys=ys, valid=valid,
                kv_src=kv_src)


def kernel_reference(case, k, pad_id, eos_id):
    """The fp64 rules on a case: (children of sbs_step_reference, top [n, k+1] candidate values, their flat indices)."""
    import torch
    from gct_plus_amd.decode import beam_log_softmax, sbs_candidates, sbs_step_reference
    logp = beam_log_softmax(case["logits"].double())
    sc, gu, noise = case["scores"].double(), case["gumbels"].double(), case["noise"].double()
    want = sbs_step_reference(sc, gu, case["fin"], case["lens"], logp, noise, k, pad_id, eos_id)
    val = sbs_candidates(sc, gu, case["fin"], logp, noise, k, pad_id)[0]
    srt = torch.sort(val, dim=1, descending=True, stable=True)
    m = min(k + 1, val.shape[1])
    return want, srt.values[:, :m], srt.indices[:, :m]


def near_tie(top):
    """bool [n]: two adjacent values among the sample's k+1 best finite candidate values lie closer than GAP -- the k-th and
    the (k+1)-th, which may swap a child in or out, or two inside the k best, which may swap their order."""
    import torch
    d = top[:, :-1] - top[:, 1:]
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return (d < GAP).any(1) if d.shape[1] else torch.zeros(top.shape[0], dtype=torch.bool)
