"""Host reference of the interpolation latents (gct_latent_stats / gct_latent_interp): plain numpy, written from the
comments of include/gctplus_hip.h, not from csrc/latent.hip.  It builds on tests/rng_ref.py (Philox, key, u01).

  statistics   per molecule and dimension over its first rows[i] latent rows: mean, then the unbiased standard
               deviation from the squared deviations; one row gives 0
  normals      element d of vector s of token t of an item: element d & 3 of the Philox call with the counter
               (item, 8 t + s, d >> 2, 082EFA98) under the key of (seed, site 1A7E47); Box-Muller as reparam_eps
  latent       u = mean_mu[a] + std_mu[a] n_0, v = mean_mu[b] + std_mu[b] n_1, p / q from log_var with n_2 / n_3;
               m = slerp(u, v, alpha), l = slerp(p, q, alpha); z = m + noise_std n_4 exp(l / 2), exactly m at noise 0
  slerp        c = u.v / (|u| |v|), w = acos c, (sin((1 - alpha) w) u + sin(alpha w) v) / sin w; the lerp
               u + alpha (v - u) when |u| == 0, |v| == 0 or not |c| <= 1 - 2^-20
"""
import numpy as np

from tests.rng_ref import _u01, philox4x32_10, rng_key

LATENT_SITE = 0x1A7E47
LATENT_C3 = 0x082EFA98
SLERP_MAX_COS = 1.0 - 2.0 ** -20


def stats_ref(mu, log_var, rows):
    """float64 [n, 4, D]: mean / std of mu, mean / std of log_var over each molecule's first rows[i] rows."""
    mu, log_var = np.asarray(mu, dtype=np.float64), np.asarray(log_var, dtype=np.float64)
    n, _, D = mu.shape
    out = np.zeros((n, 4, D))
    for i, r in enumerate(int(x) for x in rows):
        for k, src in ((0, mu), (2, log_var)):
            x = src[i, :r]
            mean = x.sum(0) / r
            out[i, k] = mean
            out[i, k + 1] = np.sqrt(((x - mean) ** 2).sum(0) / (r - 1)) if r > 1 else 0.0
    return out


def token_normals(seed, item, n_tokens, D):
    """float64 [n_tokens, 5, D]: the five normal vectors of tokens 0 .. n_tokens - 1 of an item."""
    nq = (D + 3) // 4
    t = np.arange(n_tokens, dtype=np.int64)[:, None, None]
    s = np.arange(5, dtype=np.int64)[None, :, None]
    j = np.arange(nq, dtype=np.int64)[None, None, :]
    shape = (n_tokens, 5, nq)
    x, y, z, w = philox4x32_10((np.broadcast_to(int(item), shape), np.broadcast_to(8 * t + s, shape),
                                np.broadcast_to(j, shape), LATENT_C3), rng_key(seed, LATENT_SITE))
    two_pi = float(np.float32(6.283185307179586))
    out = np.empty(shape + (4,), dtype=np.float64)
    for h, (a, b) in enumerate(((x, y), (z, w))):
        rad, ang = np.sqrt(-2.0 * np.log(_u01(a))), two_pi * _u01(b)
        out[..., 2 * h], out[..., 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(n_tokens, 5, nq * 4)[:, :, :D]


def interp_normals(seed, item, t, s, D):
    """float64 [D]: normal vector s (0..4) of token t of an item."""
    return token_normals(seed, item, t + 1, D)[t, s]


def _slerp(u, v, alpha, dt):
    """u, v [tokens, D] of dtype dt -> (result, c [tokens] (NaN where an endpoint is zero), slerp branch taken [tokens])."""
    uu, vv, uv = (u * u).sum(-1), (v * v).sum(-1), (u * v).sum(-1)
    den = np.sqrt(uu) * np.sqrt(vv)
    nz = (uu != 0) & (vv != 0)
    c = np.where(nz, uv / np.where(nz, den, dt(1)), dt(np.nan)).astype(dt)
    ok = nz & (np.abs(c) <= dt(SLERP_MAX_COS))
    w = np.arccos(np.where(ok, c, dt(0)))[:, None]
    one = dt(1)
    sl = (np.sin((one - alpha) * w) * u + np.sin(alpha * w) * v) / np.sin(w)
    return np.where(ok[:, None], sl, u + alpha * (v - u)).astype(dt), c, ok


def interp_ref(stats, a, b, alpha, noise_std, lens, items, T, seed, dtype=np.float64):
    """(z [R, T, D], c [R, T, 2], slerped [R, T, 2]) evaluated in `dtype` (np.float64, or np.float32 for every
    elementwise operation) from the SAME normals (float64 Box-Muller, rounded to dtype).  c / slerped: the cosine and
    the branch of the mu slerp (index 0) and of the log_var slerp (index 1; evaluated only where noise_std != 0) of
    every token < lens[r]; c is NaN and slerped False where nothing was evaluated.  alpha and noise_std enter as the
    float32 values the device receives."""
    dt = dtype
    stats = np.asarray(stats).astype(dt)
    R, D = len(a), stats.shape[2]
    z = np.zeros((R, T, D), dtype=dt)
    c = np.full((R, T, 2), np.nan)
    sl = np.zeros((R, T, 2), dtype=bool)
    for r in range(R):
        L = int(lens[r])
        if L == 0:
            continue
        nrm = token_normals(seed, int(items[r]), L, D).astype(dt)
        al, ns = dt(np.float32(alpha[r])), dt(np.float32(noise_std[r]))
        fa, fb = stats[int(a[r])], stats[int(b[r])]
        u, v = fa[0] + fa[1] * nrm[:, 0], fb[0] + fb[1] * nrm[:, 1]
        m, c[r, :L, 0], sl[r, :L, 0] = _slerp(u, v, al, dt)
        if ns == 0:
            z[r, :L] = m
            continue
        p, q = fa[2] + fa[3] * nrm[:, 2], fb[2] + fb[3] * nrm[:, 3]
        l, c[r, :L, 1], sl[r, :L, 1] = _slerp(p, q, al, dt)
        z[r, :L] = m + ns * nrm[:, 4] * np.exp(dt(0.5) * l)
    return z, c, sl


def interp_tolerance(stats, a, b, alpha, noise_std, lens, items, T, seed):
    """(z64, tol [R, T, D], c, slerped): the float64 latents and the tolerance a float32 device evaluation is held to --
    4 x the largest difference between this reference's float32 and float64 evaluations of these inputs (the factor
    covers the device's other libm and its reduction order over D), and not less than 1e-5 max(1, |z64|)."""
    z64, c, sl = interp_ref(stats, a, b, alpha, noise_std, lens, items, T, seed)
    z32 = interp_ref(stats, a, b, alpha, noise_std, lens, items, T, seed, dtype=np.float32)[0]
    spread = float(np.abs(z32.astype(np.float64) - z64).max()) if z64.size else 0.0
    return z64, np.maximum(4 * spread, 1e-5 * np.maximum(1.0, np.abs(z64))), c, sl


def well_conditioned(c, slerped):
    """Every evaluated slerp either took the guard or has |c| <= 0.95."""
    c = np.asarray(c)
    return bool(np.all(~slerped | (np.abs(np.where(slerped, c, 0.0)) <= 0.95)))
