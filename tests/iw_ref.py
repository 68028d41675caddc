"""Host reference of the importance-weighted marginal likelihoods (gct_latent_iw / gct_iw_combine): plain numpy fp64,
written from the comments of include/gctplus_hip.h, not from csrc/latent.hip.  It builds on tests/rng_ref.py (Philox,
key, u01), with the Box-Muller of tests/latent_ref.py.

  normals      element d of latent row t of draw k of an item: element d & 3 of the Philox call with the counter
               (item, k, 256 t + (d >> 2), 0D95748F) under the key of (seed, site 1A7E48); radius sqrt(-2 ln u01(first)),
               angle float32(2 pi) u01(second), outputs (r cos, r sin) on the word pairs (x, y) and (z, w)
  latent       on the molecule's own rows t < rows[i]: z = mu + eps exp(log_var / 2); zeros beyond
  term         0.5 ((eps - z)(eps + z) + log_var) = log N(z; 0, 1) - log N(z; mu, exp(log_var)); logw = their sum
  combine      a = logp + logw, m = max a: iwae = m + log sum exp(a - m) - log K, elbo = mean a, recon = mean logp,
               ess = (sum exp(a - m))^2 / sum exp(a - m)^2

The tolerance of logw (logw_tolerance).  The device forms, per element, in fp32 with u = 2^-24 (half an ulp):
  s = expf(0.5f * log_var)      0.5f * log_var is exact; the device expf is documented to 1 ulp: s = sigma (1 + d1),
                                |d1| <= 2 u
  z = fmaf(eps, s, mu)          one rounding: z = (eps s + mu)(1 + d2), |d2| <= u.  With z* the exact latent,
                                |eps sigma| = |z* - mu| <= |z*| + |mu|, so |z - z*| <= u (2 (|z| + |mu|) + |z|)
                                = u (3 |z| + 2 |mu|) to first order
  a = eps - z, b = eps + z      one rounding each: relative u
  f = fmaf(a, b, log_var)       one rounding: relative u on |a b| + |log_var| (bounded by the magnitudes, so that a
                                cancellation between a b and log_var is covered)
  term = 0.5f * f               exact
Against the fp64 term evaluated from the SAME eps (the kernel's eps_out), with S = (|eps| + |z| + |mu|)^2:
  from z:      0.5 |z^2 - z*^2| ~ |z| |z - z*| <= u |z| (3 |z| + 2 |mu|) <= 3 u S
  from a, b:   0.5 * 2 u |eps^2 - z^2| <= u (|eps| + |z|)^2 <= u S
  from f:      0.5 u (|eps^2 - z^2| + |log_var|) <= 0.5 u (S + |log_var|)
  the sum's one rounding to fp32 (the fp64 accumulation itself is 2^-29 times smaller and ignored):
               u |logw| <= u sum |term| <= 0.5 u sum (S + |log_var|)
which is 5 u S + u |log_var| per element to first order.  C_LOGW = 6 covers it with the second-order products
(each below 2^-22 of a first-order term): tolerance = 6 * 2^-24 * sum_j (S_j + |log_var_j|) over the molecule's own
elements.
"""
import numpy as np

from tests.rng_ref import _u01, philox4x32_10, rng_key

IW_SITE = 0x1A7E48
IW_C3 = 0x0D95748F
C_LOGW = 6.0
STAT_SEED = 2024                                     # test_marginal_host.py asserts the anchor under this seed


def iw_normals(seed, item, ks, n_rows, D):
    """float64 [len(ks), n_rows, D]: the standard normals of latent rows 0 .. n_rows - 1 of the draws ks of an item."""
    nq = (D + 3) // 4
    k = np.asarray(ks, dtype=np.int64).reshape(-1, 1, 1)
    t = np.arange(n_rows, dtype=np.int64)[None, :, None]
    j = np.arange(nq, dtype=np.int64)[None, None, :]
    shape = (k.shape[0], n_rows, nq)
    x, y, z, w = philox4x32_10((np.broadcast_to(int(item), shape), np.broadcast_to(k, shape),
                                np.broadcast_to(256 * t + j, shape), IW_C3), rng_key(seed, IW_SITE))
    two_pi = float(np.float32(6.283185307179586))
    out = np.empty(shape + (4,), dtype=np.float64)
    for h, (a, b) in enumerate(((x, y), (z, w))):
        rad, ang = np.sqrt(-2.0 * np.log(_u01(a))), two_pi * _u01(b)
        out[..., 2 * h], out[..., 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(k.shape[0], n_rows, nq * 4)[:, :, :D]


def iw_draws(seed, items, k0, Kc, Le, D):
    """float64 [n, Kc, Le, D]: the draws k0 .. k0 + Kc - 1 of every item, all Le rows (the kernel zeroes rows >= rows[i])."""
    out = np.empty((len(items), Kc, Le, D))
    for i, it in enumerate(items):
        out[i] = iw_normals(seed, int(it), np.arange(k0, k0 + Kc), Le, D)
    return out


def own_rows(rows, Le):
    """bool [n, 1, Le, 1]: latent row t is molecule i's own."""
    return (np.arange(Le)[None, :] < np.asarray(rows, dtype=np.int64)[:, None])[:, None, :, None]


def latent_iw_ref(mu, log_var, rows, eps):
    """mu, log_var [n, Le, D], rows [n], eps [n, K, Le, D] -> (z [n, K, Le, D], logw [n, K]) in float64."""
    mu, lv = np.asarray(mu, dtype=np.float64)[:, None], np.asarray(log_var, dtype=np.float64)[:, None]
    eps = np.asarray(eps, dtype=np.float64)
    own = own_rows(rows, mu.shape[2])
    z = mu + eps * np.exp(0.5 * lv)
    term = 0.5 * ((eps - z) * (eps + z) + lv)
    return np.where(own, z, 0.0), np.where(own, term, 0.0).sum((2, 3))


def logw_tolerance(mu, log_var, rows, eps, z):
    """float64 [n, K]: C_LOGW 2^-24 sum ((|eps| + |z| + |mu|)^2 + |log_var|) over each molecule's own elements."""
    mu, lv = np.abs(np.asarray(mu, dtype=np.float64))[:, None], np.abs(np.asarray(log_var, dtype=np.float64))[:, None]
    s = (np.abs(np.asarray(eps, dtype=np.float64)) + np.abs(np.asarray(z, dtype=np.float64)) + mu) ** 2 + lv
    return C_LOGW * 2.0 ** -24 * np.where(own_rows(rows, mu.shape[2]), s, 0.0).sum((2, 3))


def combine_ref(logp, logw):
    """logp, logw [n, K] -> (iwae, elbo, recon, ess) float64 [n]."""
    logp, logw = np.asarray(logp, dtype=np.float64), np.asarray(logw, dtype=np.float64)
    K = logp.shape[1]
    a = logp + logw
    m = a.max(1, keepdims=True)
    e = np.exp(a - m)
    s1, s2 = e.sum(1), (e * e).sum(1)
    return m[:, 0] + np.log(s1) - np.log(K), a.sum(1) / K, logp.sum(1) / K, s1 * s1 / s2


def combine_tolerance(value):
    """fp64 arithmetic with one rounding to fp32: 2^-23 max(1, |value|)."""
    return 2.0 ** -23 * np.maximum(1.0, np.abs(np.asarray(value, dtype=np.float64)))


# ----------------------------------------------------------------------------------------- the statistical anchor
# D = 4, two latent rows, mu = 0.3, log_var = -0.2 everywhere: s^2 = exp(log_var) > 1/2, so the weight p / q has a
# finite variance.  E_q[p / q] = 1 exactly and, per element, E_q[(p / q)^2] = s^2 / sqrt(2 s^2 - 1) exp(m^2 / (2 s^2 - 1)).
STAT = dict(D=4, rows=2, mu=0.3, log_var=-0.2, K=65536, item=3)


def stat_second_moment():
    s2 = np.exp(STAT["log_var"])
    per = s2 / np.sqrt(2 * s2 - 1) * np.exp(STAT["mu"] ** 2 / (2 * s2 - 1))
    return float(per ** (STAT["D"] * STAT["rows"]))


def stat_check(logw):
    """(mean of exp(logw), its distance from 1 in standard errors) over the K draws of the anchor."""
    w = np.exp(np.asarray(logw, dtype=np.float64).reshape(-1))
    assert w.size == STAT["K"]
    se = np.sqrt((stat_second_moment() - 1.0) / w.size)
    return float(w.mean()), float(abs(w.mean() - 1.0) / se)
