"""Host reference of the per-step sampling statistics (gct_step_stats): plain numpy, written from the comment of
include/gctplus_hip.h and decode.step_stats_reference's docstring, not from csrc/decode.hip.

  pi   softmax of the raw logits row x, log pi_c = (x_c - m) - log sum exp(x - m), m the row maximum
  q    the behaviour distribution: the probs row as given; pi when probs is None; the one-hot at tok under greedy
  model_entropy = -sum pi log pi                  behaviour_logp = log q(tok)
  behaviour_entropy = -sum_{q>0} q log q           behaviour_kl = sum_{q>0} q (log q - log pi)
  tok == pad (or outside the vocabulary): four zeros.

`step_stats_ref` is that in fp64; `step_stats_f32` restates the kernel in fp32 (lane l adds tokens l, l + 64, ... in
ascending order, the 64 partial sums meet in a xor butterfly), with the one-mistake mutants the host test needs.

The bounds (`step_stats_bounds`), per row, u = 2^-24 (half an ulp), the device's expf / logf documented to 1 ulp = 2 u
relative.  k = ceil(V / 64) + 6 roundings lie on any path through a V-term wave sum.  With y_c = x_c - m:
  y_c              one rounding: u |y_c|
  e_c = expf(y_c)  relative 2 u + u |y_c|;  se = sum e_c: relative (2 + k) u + u sum pi_c |y_c| <= (2 + k + Y) u,
                   Y = max |y_c|
  lse = logf(se)   absolute L u,  L = 2 + k + Y + 2 |lse|
  lpi_c            = y_c - lse, one more rounding: D_c u,  D_c = |y_c| + L + |lpi_c|        (behaviour_logp's bound at
                   c = tok when q = pi, and behaviour_kl's under greedy, where KL = -lpi_tok)
  pi_c = expf(lpi_c)  relative (2 + D_c) u
  model_entropy    term pi_c lpi_c with one product rounding: pi_c u (|lpi_c| (3 + D_c) + D_c); the sum of V terms of
                   one sign: k u H.  Bound: u (sum pi_c (|lpi_c| (3 + D_c) + D_c) + k H)
  lq_c = logf(q_c) absolute 2 u |lq_c|  (q is an input: the reference reads the same fp32 values)
  behaviour_logp   2 u |lq_tok|
  behaviour_entropy  term q_c lq_c: 3 u q_c |lq_c|; the sum: k u sum q |lq|.  Bound: (3 + k) u sum q_c |lq_c|
  behaviour_kl     d_c = lq_c - lpi_c: (2 |lq_c| + D_c + |d_c|) u; times q_c with one rounding, summed with mixed signs:
                   u sum q_c (2 |lq_c| + D_c + (2 + k) |d_c|)
All first order; C_STATS = 2 covers the second-order products (each below 2^-20 of a first-order term here) and the
reference's own fp64 rounding.  q = pi: behaviour_entropy has model_entropy's bound and behaviour_kl is exactly 0 (bound
0); greedy: behaviour_logp and behaviour_entropy are exactly 0.  A pad row is exactly 0 everywhere.
"""
import numpy as np

U = 2.0 ** -24
C_STATS = 2.0
NAMES = ("model_entropy", "behaviour_logp", "behaviour_entropy", "behaviour_kl")
MUTANTS = ("entropy_of_pi", "logp_of_pi", "unnormalised_q", "pad_not_zeroed", "log2")


def _live(tok, pad_id, V):
    tok = np.asarray(tok, dtype=np.int64).reshape(-1)
    return tok, (tok != pad_id) & (tok >= 0) & (tok < V)


def _log_pi(x):
    y = x - x.max(-1, keepdims=True)
    return y, y - np.log(np.exp(y).sum(-1, keepdims=True))


def _xlogy_sum(q, l):
    with np.errstate(invalid="ignore"):
        return np.where(q > 0, q * l, 0.0).sum(-1)


def step_stats_ref(logits, probs, tok, pad_id, greedy=False):
    """fp64 [4, n] in NAMES' order: logits [n, V], probs [n, V] or None (taken as given), tok [n]."""
    x = np.asarray(logits, dtype=np.float64)
    n, V = x.shape
    tok, live = _live(tok, pad_id, V)
    at = np.clip(tok, 0, V - 1)
    _, lpi = _log_pi(x)
    pi = np.exp(lpi)
    if greedy:
        q = np.zeros_like(pi)
        q[np.arange(n), at] = 1.0
        lq = np.zeros_like(pi)
    elif probs is None:
        q, lq = pi, lpi
    else:
        q = np.asarray(probs, dtype=np.float64)
        lq = np.log(np.where(q > 0, q, 1.0))
    qt = q[np.arange(n), at]
    out = np.stack([-_xlogy_sum(pi, lpi), np.where(qt > 0, lq[np.arange(n), at], -np.inf), -_xlogy_sum(q, lq),
                    _xlogy_sum(q, lq - lpi)])
    return np.where(live[None, :], out, 0.0)


def _wave_sum_f32(terms):
    """fp32 sum of terms [V] in the kernel's order: lane l adds tokens l, l + 64, ... ascending, then a xor butterfly."""
    lanes = np.zeros(64, dtype=np.float32)
    for c in range(terms.shape[0]):
        lanes[c & 63] = np.float32(lanes[c & 63] + terms[c])
    o = 32
    while o:
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
        o >>= 1
    return lanes[0]


def step_stats_f32(logits, probs, tok, pad_id, greedy=False, mutant=None):
    """The kernel restated in fp32, [4, n] float32.  mutant (one of MUTANTS) makes one mistake:
      entropy_of_pi   H(pi) where H(q) is asked          logp_of_pi     log pi(tok) for log q(tok)
      unnormalised_q  probs used as weights that were not divided by their own sum: the caller passes those weights
                      (the restatement itself takes probs as given -- the mistake is the caller's, in what it passes)
      pad_not_zeroed  a pad row computed like any other   log2          log2 for ln"""
    assert mutant is None or mutant in MUTANTS
    f32 = np.float32
    log = np.log2 if mutant == "log2" else np.log
    x = np.asarray(logits, dtype=f32)
    n, V = x.shape
    tok, live = _live(tok, pad_id, V)
    out = np.zeros((4, n), dtype=f32)
    for r in range(n):
        t = int(tok[r])
        if not live[r]:
            if mutant != "pad_not_zeroed" or not 0 <= t < V:
                continue
        y = (x[r] - x[r].max()).astype(f32)
        lse = f32(log(_wave_sum_f32(np.exp(y).astype(f32))))
        lp = f32(y[t] - lse)
        lpi = (y - lse).astype(f32)
        pi = np.exp(lpi).astype(f32)
        me = f32(0) - _wave_sum_f32(np.where(pi != 0, pi * np.where(pi != 0, lpi, 0), 0).astype(f32))
        if greedy:
            bl, be, kl = f32(0), f32(0), f32(0) - lp
        elif probs is None:
            bl, be, kl = lp, me, f32(0)
        else:
            q = np.asarray(probs, dtype=f32)[r]
            pos = q > 0
            lq = log(np.where(pos, q, f32(1))).astype(f32)
            bl = lp if mutant == "logp_of_pi" else (lq[t] if q[t] > 0 else f32(-np.inf))
            be = me if mutant == "entropy_of_pi" else f32(0) - _wave_sum_f32(np.where(pos, q * lq, 0).astype(f32))
            kl = _wave_sum_f32(np.where(pos, q * (lq - np.where(pos, lpi, 0)).astype(f32), 0).astype(f32))
        out[:, r] = me, bl, be, kl
    return out


def step_stats_bounds(logits, probs, tok, pad_id, greedy=False):
    """fp64 [4, n]: the bound of each output of each row (the module docstring derives them)."""
    x = np.asarray(logits, dtype=np.float64)
    n, V = x.shape
    tok, live = _live(tok, pad_id, V)
    at, rows = np.clip(tok, 0, V - 1), np.arange(n)
    k = -(-V // 64) + 6
    y, lpi = _log_pi(x)
    pi = np.exp(lpi)
    ay, alpi = np.abs(y), np.abs(lpi)
    lse = -lpi[:, :1] + y[:, :1]                                   # lpi = y - lse
    L = 2 + k + ay.max(-1, keepdims=True) + 2 * np.abs(lse)
    D = ay + L + alpi
    b_lp = D[rows, at]
    b_me = (pi * (alpi * (3 + D) + D)).sum(-1) + k * (pi * alpi).sum(-1)
    zero = np.zeros(n)
    if greedy:
        b = [b_me, zero, zero, b_lp]
    elif probs is None:
        b = [b_me, b_lp, b_me, zero]
    else:
        q = np.asarray(probs, dtype=np.float64)
        alq = np.abs(np.log(np.where(q > 0, q, 1.0)))
        d = np.abs(np.where(q > 0, np.log(np.where(q > 0, q, 1.0)) - lpi, 0.0))
        b = [b_me, 2 * alq[rows, at], (3 + k) * (q * alq).sum(-1), (q * (2 * alq + D + (2 + k) * d)).sum(-1)]
    return np.where(live[None, :], C_STATS * U * np.stack(b), 0.0)


def make_case(n, V, seed, pad_id=0, mode="probs"):
    """Seeded inputs of n rows over V tokens: logits fp32 with |x| <= 12; tok [n] drawn among the tokens q allows (never
    pad_id, which lies outside the vocabulary when V == 1); mode "probs": q = normalised weights of a softmax at temperature 0.7 in which about a third of the tokens
    are exact zeros and about a sixth carry the 1e-6 floor (what a nucleus and a top-k filter leave), with the raw
    weights next to them; "none" / "greedy": probs None.  Returns (logits, probs, weights, tok)."""
    g = np.random.default_rng(seed)
    x = np.clip(g.standard_normal((n, V)) * 3.0, -12, 12).astype(np.float32)
    if mode != "probs":
        tok = g.integers(0, V, n)
        tok = np.where(tok == pad_id, (tok + 1) % V, tok)
        assert (tok != pad_id).all()
        return x, None, None, tok
    w = np.exp((x.astype(np.float64) - x.max(-1, keepdims=True)) / 0.7)
    kind = g.random((n, V))
    w = np.where(kind < 1 / 3, 0.0, np.where(kind < 0.5, 1e-6, w))
    xs = x.copy()
    if 0 <= pad_id < V:                                            # pad is never drawn: weight 0 (V == 1: pad_id outside)
        assert V > 1
        xs[:, pad_id] = -np.inf
        w[:, pad_id] = 0.0
    w[np.arange(n), xs.argmax(-1)] = 1.0                           # the top token always stays in
    w = (w * g.uniform(0.3, 0.9, (n, 1))).astype(np.float32)       # raw weights: they do not sum to 1
    q = (w.astype(np.float64) / w.astype(np.float64).sum(-1, keepdims=True)).astype(np.float32)
    tok = np.array([g.choice(np.flatnonzero(q[r] > 0)) for r in range(n)])
    return x, q, w, tok
