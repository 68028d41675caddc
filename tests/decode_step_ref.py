"""Host references of the decode-step kernels (gct_attn_decode, gct_decode_embed, gct_select_token), written from the
statements in include/gctplus_hip.h, in fp64, plus the inputs of the exact-draw tests: tests/test_decode_step_ref_host.py
holds the references and those inputs to themselves without a GPU, tests/test_decode_step_kernels_gpu.py holds the
kernels to them.  The random stream of the draw is in tests/rng_ref.py (select_uniform, draw)."""
import functools
import itertools

import numpy as np
import torch

from tests import rng_ref as R


# ------------------------------------------------------------------------------------------------ cached attention
def cached_attention(q, keys, values, valid, scale):
    """One query row per sample against its cached keys: q [n, H, dk], keys / values [n, L, H, dk], valid [n, L] (0 =>
    masked, or None) -> [n, H, dk], all fp64: softmax(masked_fill(q . k * scale, valid == 0, -1e9)) v, per head.  A row
    whose keys are all masked comes out with uniform weights, like the module this restates."""
    q, keys, values = q.double(), keys.double(), values.double()
    s = torch.einsum("nhd,njhd->nhj", q, keys) * float(scale)
    if valid is not None:
        s = s.masked_fill(valid[:, None, :] == 0, -1e9)
    return torch.einsum("nhj,njhd->nhd", torch.softmax(s, -1), values)


# ------------------------------------------------------------------------------------------------ embedding of a step
def decode_embed(ys, p, table, pe, pe_off, scale):
    """ys int64 [n, W], p int64 [n] (the position of each row), table [vocab, d], pe [rows, d] -> (x, bound), fp64
    [n, d]: x = table[clamp(ys[b, p_b], 0, vocab - 1)] * scale + pe[pe_off + p_b], and the rounding bound of an fp32
    evaluation of it -- one multiply and one add (2 roundings, each half an ulp of a value no larger than
    |e * scale| + |pe|) or one fma (1 rounding): |err| <= 2^-23 (|e * scale| + |pe|)."""
    n = ys.shape[0]
    tok = ys[torch.arange(n), p].clamp(0, table.shape[0] - 1)
    e, q = table.double()[tok] * float(scale), pe.double()[pe_off + p]
    return e + q, 2.0 ** -23 * (e.abs() + q.abs())


# ------------------------------------------------------------------------------------------------ greedy choice
def greedy(logits):
    """logits [n, V] -> (first index of the maximum [n], fp64 softmax [n, V])."""
    x = logits.double()
    first = np.argmax((x == x.max(-1, keepdim=True).values).numpy(), axis=-1)   # numpy: the first True
    return torch.from_numpy(first), torch.softmax(x, -1)


# ------------------------------------------------------------------------------------------------ exact draws
DRAW_ROWS = 4096
SEEDS = (123, (0xABCDEF01 << 32) | 5)               # the second has a high word: a 32-bit truncation would show
POSITIONS = (1, 7)
UNDECIDABLE_CAP = 0.02                              # share of the rows of a case whose gap is within delta(V)


def combos(V):
    """The (seed, position) pairs a draw case runs at: the whole cross up to V = 257; above, where the fp64 reference of
    4096 rows takes most of a second per launch, each seed and each position once."""
    return list(itertools.product(SEEDS, POSITIONS)) if V <= 257 else list(zip(SEEDS, POSITIONS))


def delta(V):
    """How far the device's fp32 cumulative sum may sit from the fp64 one: a few ulp (of 1) per probability and its
    normalisation, a six-level wave scan, and one carry per chunk of 64 tokens: (16 + V / 64) * 2^-23."""
    return (16 + V / 64) * 2.0 ** -23


# (name, V, logit scale, filter (k, p, T) or None)
PLAIN_CASES = [(f"plain-{V}", V, 2.0, None) for V in (1, 30, 64, 65, 257, 1024)] + [("plain-4099", 4099, 6.0, None)]
FILTER_CASES = [("filt-30", 30, 2.0, (8, 0.9, 0.8)), ("filt-65", 65, 2.0, (12, 0.95, 0.9)),
                ("filt-1024-k50", 1024, 2.0, (50, 0.9, 1.2)), ("filt-1024-p", 1024, 2.0, (None, 0.7, 1.0)),
                ("filt-200-k3", 200, 2.0, (3, None, 1.0))]
# plain draws from rows where 60% of the logits are -inf (tokens a grammar mask forbids): weight-0 tokens in front of,
# behind and between the tokens a draw can hit
NINF_CASES = [("ninf-65", 65, 2.0, None), ("ninf-257", 257, 2.0, None)]
DRAW_CASES = PLAIN_CASES + FILTER_CASES + NINF_CASES
CASE = {c[0]: c for c in DRAW_CASES}


@functools.lru_cache(maxsize=None)
def draw_inputs(name):
    """(logits fp32 [DRAW_ROWS, V], weights fp64 [DRAW_ROWS, V]) of a draw case; computed once, shared, never written.
    Plain: weights = the fp64 softmax of the logits.  Filtered: rows away from the nucleus boundary (the device sums
    the masses in another order), weights = decode.sample_filter_reference (which works on fp32 logits) as fp64."""
    _, V, scale, filt = CASE[name]
    if filt is None:
        g = torch.Generator().manual_seed(1000 + V)
        x = (torch.randn(DRAW_ROWS, V, generator=g) * scale).contiguous()
        if name.startswith("ninf"):
            hide = torch.rand(DRAW_ROWS, V, generator=g) < 0.6
            hide[torch.arange(DRAW_ROWS), torch.arange(DRAW_ROWS) % V] = False      # every row keeps a token
            x[hide] = -float("inf")
        return x, torch.softmax(x.double(), -1).numpy()
    from gct_plus_amd.decode import sample_filter_reference
    from tests.test_sample_filter_gpu import rows_away_from_the_boundary
    k, p, T = filt
    x = rows_away_from_the_boundary(V, k, T, 1.0 if p is None else p, DRAW_ROWS, seed=2000 + V)
    return x, sample_filter_reference(x, top_k=k, top_p=p, temperature=T).double().numpy()


def reference_draws(weights, seed, keys, pos, word=0):
    """(pick, gap, lo, hi) of rng_ref.draw for rows keyed (keys[r], pos[r]) under seed."""
    return R.draw(weights, R.select_uniform(seed, keys, pos, word).astype(np.float64))


def check_draws(got, weights, seed, keys, pos, V):
    """got int64 [n]: the device's picks.  Decidable rows (gap > delta(V)) equal the reference pick; the others hold one
    of the two nonzero-weight tokens at the nearest boundary.  Returns the number of undecidable rows."""
    pick, gap, lo, hi = reference_draws(weights, seed, keys, pos)
    got = np.asarray(got)
    assert (got >= 0).all() and (got < V).all(), "a pick outside the vocabulary"
    assert (weights[np.arange(len(got)), got] > 0).all(), "a token of weight 0 was picked"
    sure = gap > delta(V)
    bad = np.nonzero(sure & (got != pick))[0]
    assert bad.size == 0, (f"{bad.size} decidable rows differ; first: row {bad[0]} got {got[bad[0]]} want "
                           f"{pick[bad[0]]} gap {gap[bad[0]]:.3e} delta {delta(V):.3e}")
    edge = ~sure
    assert ((got[edge] == lo[edge]) | (got[edge] == hi[edge])).all(), "an undecidable row picked a third token"
    assert int(edge.sum()) <= UNDECIDABLE_CAP * len(got), (int(edge.sum()), len(got))
    return int(edge.sum())


def seed_tensor(seed):
    """int64 [1] holding the 64 bits of an unsigned seed (for seed_dev)."""
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64)
