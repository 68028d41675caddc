"""Host references of dense attention (gct_attn_mask_pack, gct_attn_fwd, gct_attn_bwd): plain numpy / torch fp64 on the
CPU, written from the statements in include/gctplus_hip.h (packed bits, the tile-word rule, the lse convention) and the
reference's attention() (Model/sublayers.py:29-41: masked_fill(mask == 0, -1e9), softmax, dropout on the probabilities),
not from the kernels.  tests/test_attention_ref_host.py holds them to independent restatements; the masks, shapes and
inputs of tests/test_attention_dense_gpu.py are built here so that the host tests can show they discriminate."""
import math

import numpy as np
import torch

from tests import rng_ref

MASK_WORDS = 8                       # packed words per query row (Lk <= 256)

# tolerances of test_attention / test_attention_dropout (tests/test_kernels_gpu.py): atol, rtol
TOL_PROBS = (1e-6, 1e-5)
TOL_O = (1e-5, 1e-5)
TOL_GRAD = (2e-5, 1e-4)
TOL_GRAD_DROP = (3e-5, 1e-4)
# lse: worst |fp32 - fp64| / (1 + |fp64|) of torch.logsumexp over the scaled masked scores, scores and sum in fp32 against
# both in fp64, over all cases of sections B and C of tests/test_attention_dense_gpu.py, rows without a visible key left
# out: 1.62e-7 over B, 4.52e-7 over C sized for 256 compute units (its worst: L = 130, dk = 64, 1032 pairs).  The kernels
# are allowed 8 x that (fast exp / log intrinsics, sums in tile order).  test_attention_ref_host.py re-measures the B cases.
LSE_FP32_ERR = 4.53e-7
TOL_LSE = 8 * LSE_FP32_ERR


# ------------------------------------------------------------------------------------------------ mask packing
def pack_bits(mask_u8, Lk):
    """uint8 mask [.., >= Lk] -> uint32 [.., 8]: bit k & 31 of word k >> 5 set iff mask[.., k] != 0 and k < Lk."""
    m = np.asarray(mask_u8)[..., :Lk] != 0
    full = np.zeros(m.shape[:-1] + (32 * MASK_WORDS,), dtype=np.uint64)
    full[..., :Lk] = m
    full = full.reshape(m.shape[:-1] + (MASK_WORDS, 32))
    return (full << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def tile_words(mask_u8):
    """uint8 [B, Lq, Lk] -> uint32 [B, ceil(Lq / 16)]; [B, Lk] (key padding: the single row is the tile) -> [B, 1].
    Every real row of the query tile sees a key: bit t set iff some real row sees one of keys 16t .. 16t+15; otherwise
    all ceil(Lk / 16) bits.  Bits at and above ceil(Lk / 16) are 0."""
    m = np.asarray(mask_u8) != 0
    if m.ndim == 2:
        m = m[:, None, :]
    B, Lq, Lk = m.shape
    nqt, nkt = (Lq + 15) // 16, (Lk + 15) // 16
    out = np.zeros((B, nqt), dtype=np.uint32)
    for b in range(B):
        for u in range(nqt):
            rows = m[b, 16 * u:min(Lq, 16 * u + 16)]
            if rows.any(1).all():
                word = sum(1 << t for t in range(nkt) if rows[:, 16 * t:16 * t + 16].any())
            else:
                word = (1 << nkt) - 1
            out[b, u] = word
    return out


# ------------------------------------------------------------------------------------------------ attention
def full_mask(mask, B, Lq, Lk):
    """None | uint8 [B, Lk] | [B, Lq, Lk] -> bool [B, 1, Lq, Lk] (None: everything visible)."""
    if mask is None:
        return torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    m = torch.as_tensor(mask) != 0
    if m.dim() == 2:
        m = m[:, None, :].expand(B, Lq, Lk)
    return m[:, None]


def attention(q, k, v, mask, scale, keep=None, pkeep=1.0):
    """q [B, H, Lq, dk], k / v [B, H, Lk, dk] fp64; mask bool, broadcastable to [B, H, Lq, Lk] (False = masked) or None;
    keep (bool, same shape as the scores) / pkeep: dropout on the probabilities.  Returns (o, probs before dropout,
    lse): lse = logsumexp of the scaled scores with masked ones at -1e9; a row that sees no key is uniform over its Lk
    keys and its lse is stated as log(Lk) (the -1e9 every score shares is left out).  Differentiable."""
    s = q @ k.transpose(-1, -2) * scale
    Lk = s.shape[-1]
    if mask is not None:
        s = s.masked_fill(~mask, -1e9)
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    den = e.sum(-1, keepdim=True)
    pr = e / den
    lse = (m + den.log()).squeeze(-1)
    if mask is not None:
        sees = mask.expand(s.shape).any(-1)
        lse = torch.where(sees, lse, torch.full_like(lse, math.log(Lk)))
    pd = pr if keep is None else pr * keep / pkeep
    return pd @ v, pr, lse


def attention_with_grads(q, k, v, mask, scale, do, keep=None, pkeep=1.0, chunk=64, want_probs=False):
    """attention() and its gradients for the output gradient `do`, in chunks of `chunk` samples (autograd per chunk) so
    that no [B, H, Lq, Lk] tensor of a large case exists at once.  q, k, v, do: fp64 [B, H, L, dk]; mask: bool
    [B, 1, Lq, Lk] or None; keep: bool [B, H, Lq, Lk], or a function (b0, b1) -> that of samples b0 .. b1 - 1.  Returns a dict o, lse, dq, dk, dv (and probs when asked for)."""
    B = q.shape[0]
    out = {n: [] for n in ("o", "lse", "dq", "dk", "dv", "probs")}
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        qc, kc, vc = (t[sl].detach().clone().requires_grad_() for t in (q, k, v))
        kp = None if keep is None else (keep(sl.start, sl.stop) if callable(keep) else keep[sl])
        o, pr, lse = attention(qc, kc, vc, None if mask is None else mask[sl], scale, kp, pkeep)
        o.backward(do[sl])
        for n, t in (("o", o), ("lse", lse), ("dq", qc.grad), ("dk", kc.grad), ("dv", vc.grad)):
            out[n].append(t.detach())
        if want_probs:
            out["probs"].append(pr.detach())
    return {n: torch.cat(ts) for n, ts in out.items() if ts}


def attn_keep(seed, site, p, B, H, Lq, Lk, b0=0, b1=None):
    """bool tensor [b1 - b0, H, Lq, Lk]: the kept probabilities of samples b0 .. b1 - 1 (all by default) of a
    [B, H, Lq, Lk] call, for every key: visible, masked or in a skipped tile alike.  The rule of tests/rng_ref.py (key
    16t + 4g + r of row (b H + h) Lq + q takes 16-bit lane 4 (t & 1) + r of the Philox call (row, 4 (t >> 1) + g)), one
    call per 8 keys; test_attention_ref_host.py holds it to rng_ref.attn_keep."""
    b1 = B if b1 is None else min(b1, B)
    rows = np.arange(b0 * H * Lq, b1 * H * Lq, dtype=np.int64)[:, None]
    nc = 4 * ((Lk + 31) // 32)                                          # calls per row: (t >> 1, g)
    c = np.arange(nc, dtype=np.int64)[None, :]
    words = rng_ref.philox4x32_10((rows + 0 * c, c + 0 * rows, rng_ref.ATTN_C2, rng_ref.ATTN_C3),
                                  rng_ref.rng_key(seed, site))
    lanes = np.stack([(w >> np.uint64(16 * h)) & np.uint64(0xFFFF) for w in words for h in (0, 1)], -1)   # [rows, nc, 8]
    k = np.arange(Lk)
    t, g, r = k >> 4, (k >> 2) & 3, k & 3
    keep = lanes[:, 4 * (t >> 1) + g, 4 * (t & 1) + r] >= np.uint64(rng_ref.drop_threshold(p) >> 16)
    return torch.from_numpy(keep.reshape(b1 - b0, H, Lq, Lk))


# ------------------------------------------------------------------------------------------------ section B cases
# (B, H, Lq, Lk, dk) -> (forward kind, backward kind): 0 direct, 1 LDS 8 tiles, 2 LDS 13 tiles (gct_attn_route)
CASES_B = {
    (2, 3, 40, 37, 16): (0, 0), (2, 2, 96, 96, 32): (0, 0), (2, 2, 81, 90, 64): (0, 0),
    (2, 2, 100, 100, 16): (1, 1), (2, 2, 33, 128, 32): (1, 1), (2, 2, 120, 97, 64): (1, 1),
    (2, 2, 130, 129, 16): (2, 2), (1, 2, 208, 208, 32): (2, 2), (2, 2, 60, 203, 64): (2, 2),
    (2, 2, 150, 100, 64): (1, 2), (1, 2, 208, 97, 16): (1, 2),
}
FAMILIES = ("left", "band", "blocks")
DROP_P, DROP_SEED, DROP_SITE = 0.2, 4242, 6


def left_masked(B, Lk):
    """Leading masked keys per sample of the `left` family: 21 (key tile 0 invisible, tile 1 begins masked), every key,
    5, 37, and again."""
    return [min(Lk, (21, Lk, 5, 37)[b % 4]) for b in range(B)]


def make_mask(family, B, Lq, Lk):
    """uint8 mask of a family: `left` [B, Lk] (key padding), `band` and `blocks` [B, Lq, Lk]."""
    k = torch.arange(Lk)
    if family == "left":
        n = torch.tensor(left_masked(B, Lk))
        return (k[None, :] >= n[:, None]).to(torch.uint8)
    nkt = (Lk + 15) // 16
    q = torch.arange(Lq)
    m = torch.zeros(B, Lq, Lk, dtype=torch.uint8)
    for b in range(B):
        if family == "band":           # |k - centre(q)| <= Lk / 16 + 3b (at least 2): leading and trailing key tiles are
            centre = (q * Lk) // Lq    # skipped; two rows of different query tiles see nothing (tiles 1 and last / 0 and 1)
            m[b] = ((k[None, :] - centre[:, None]).abs() <= max(2, Lk // 16) + 3 * b).to(torch.uint8)
            r1, r2 = ((3 + 5 * b) % 16, 16 + (5 + b) % 16) if b % 2 else (16 + (3 + 5 * b) % 16, Lq - 1)
            assert r1 // 16 != r2 // 16 and r2 < Lq
            m[b, r1] = 0
            m[b, r2] = 0
        elif family == "blocks":       # query tile u sees only key tile (5u + 3 + b) mod nkt: sample 0 is the plain rule,
            t = (5 * (q // 16) + 3 + b) % nkt          # the shift tells one sample's mask from the next one's
            m[b] = ((k[None, :] // 16) == t[:, None]).to(torch.uint8)
        else:
            raise ValueError(family)
    return m


def make_inputs(B, H, Lq, Lk, dk, seed=1):
    """Independent N(0, 1) fp32 q [B*Lq, d], k, v [B*Lk, d], do [B*Lq, d] (heads merged, as the kernels read them)."""
    g = torch.Generator().manual_seed(seed * 1000003 + 17 * Lq + Lk + dk)
    d = H * dk
    return tuple(torch.randn(r, d, generator=g) for r in (B * Lq, B * Lk, B * Lk, B * Lq))


def heads(x, B, L, H, dk):
    """[B*L, H*dk] -> fp64 [B, H, L, dk]"""
    return x.double().reshape(B, L, H, dk).transpose(1, 2)


def unheads(x):
    """[B, H, L, dk] -> [B*L, H*dk]"""
    B, H, L, dk = x.shape
    return x.transpose(1, 2).reshape(B * L, H * dk)


def causal_ragged_mask(B, Lq, Lk):
    """Section C: uint8 [B, Lq, Lk]; query q sees key k iff k <= q + (Lk - Lq) and k < len_b, a different len per sample."""
    lens = torch.tensor([Lk - (b * 7) % (Lk // 2) for b in range(B)])
    k, q = torch.arange(Lk), torch.arange(Lq)
    causal = k[None, :] <= q[:, None] + (Lk - Lq)
    return (causal[None] & (k[None, None, :] < lens[:, None, None])).to(torch.uint8)


def ratio(got, ref, tol):
    """worst |got - ref| / (atol + rtol |ref|); NaN / inf in `got` count as infinitely wrong"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not got.numel():
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (tol[0] + tol[1] * ref.abs())).max())


def lse_ratio(got, ref):
    """worst |got - ref| / (TOL_LSE (1 + |ref|))"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (TOL_LSE * (1 + ref.abs()))).max())


# ------------------------------------------------------------------------------------------------ section C cases
# (Lq, Lk, dk, p) on the LDS kernels, H = 8, B from the planner: more than two rounds of pairs per workgroup
CASES_C = [(100, 100, 16, 0.1), (20, 100, 64, 0.0), (20, 100, 32, 0.0), (130, 130, 16, 0.0), (130, 130, 64, 0.1)]
H_C = 8


def batch_c(fwd_grid, bwd_grid):
    """The smallest B with B * H_C > 2 * max(forward grid, backward grid), the grids being those of npairs -> infinity."""
    return 2 * max(fwd_grid, bwd_grid) // H_C + 1
