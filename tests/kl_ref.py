"""The per-dimension KL rule with free bits, a row mask and running moments, restated in numpy from its definition
(include/gctplus_hip.h, gct_kld_dims_fwd) -- independent of gct_plus_amd.engine, whose references are tested against it.

t(r, j) = 1.0f + l - m*m - expf(l) is formed in fp32, one rounding per operation, left to right; everything after it
is fp64.  A kernel may fuse m*m into the subtraction and has its own expf: T_EPS bounds all of that."""
import numpy as np

T_EPS = 8 * 2.0 ** -24          # the five fp32 operations of t (1 + l, m * m, the difference, expf at 2 ulp, the difference)


def rows2d(mu, log_var, live=None):
    m = np.asarray(mu, dtype=np.float32)
    l = np.asarray(log_var, dtype=np.float32)
    assert m.shape == l.shape
    D = m.shape[-1]
    m, l = m.reshape(-1, D), l.reshape(-1, D)
    keep = np.ones(m.shape[0], dtype=bool) if live is None else np.asarray(live).reshape(-1) != 0
    assert keep.shape[0] == m.shape[0]
    return m, l, keep


def t32(m, l):
    one = np.float32(1.0)
    return ((one + l) - m * m) - np.exp(l).astype(np.float32)


def kl_dims(mu, log_var, live=None, free_bits=0.0, n_mol=1):
    m, l, keep = rows2d(mu, log_var, live)
    K = -0.5 * t32(m, l)[keep].astype(np.float64).sum(axis=0)
    floor = float(np.float32(free_bits)) * int(n_mol)
    gate = K > floor
    return {"kl_dim": K, "floor": floor, "gate": gate, "objective": float(np.where(gate, K, floor).sum()),
            "raw": float(K.sum()), "n_floor": int((~gate).sum()), "live_rows": int(keep.sum())}


def kl_dims_grad(mu, log_var, live=None, free_bits=0.0, n_mol=1):
    m, l, keep = rows2d(mu, log_var, live)
    w = (keep[:, None] & kl_dims(mu, log_var, live, free_bits, n_mol)["gate"][None, :]).astype(np.float64)
    return w * m.astype(np.float64), w * 0.5 * (np.exp(l.astype(np.float64)) - 1.0)


def kl_dim_bound(mu, log_var, live=None):
    """|kl_dim_j - fp64| <= 0.5 * N_live * T_EPS * max over the live rows of (1 + |l| + m^2 + e^l), per dimension."""
    m, l, keep = rows2d(mu, log_var, live)
    if not keep.any():
        return np.zeros(m.shape[1])
    m, l = m[keep].astype(np.float64), l[keep].astype(np.float64)
    return 0.5 * keep.sum() * T_EPS * (1.0 + np.abs(l) + m * m + np.exp(l)).max(axis=0)


def moments(batches):
    """The fp64 [6, D] state after the (mu, log_var, live) batches: sum mu, sum mu^2, sum exp(lv), sum lv,
    sum -0.5 t, live rows."""
    acc = None
    for mu, log_var, live in batches:
        m, l, keep = rows2d(mu, log_var, live)
        if acc is None:
            acc = np.zeros((6, m.shape[1]))
        t = t32(m, l)[keep].astype(np.float64)
        m, l = m[keep].astype(np.float64), l[keep].astype(np.float64)
        acc += np.stack([m.sum(0), (m * m).sum(0), np.exp(l).sum(0), l.sum(0), -0.5 * t.sum(0),
                         np.full(m.shape[1], float(keep.sum()))])
    return acc


def latent_inputs(B, Le, D, seed):
    """The test inputs: mu[:, j] = s_j N(0, 1), lv[:, j] = log v_j + 0.1 N(0, 1), (s_j, v_j) = (0.02, 0.98) for even
    j and (1.0, 0.3) for odd j -- one collapsed and one informative family of dimensions."""
    rng = np.random.default_rng(seed)
    even = (np.arange(D) % 2) == 0
    s = np.where(even, 0.02, 1.0)
    v = np.where(even, 0.98, 0.3)
    mu = (s * rng.standard_normal((B, Le, D))).astype(np.float32)
    lv = (np.log(v) + 0.1 * rng.standard_normal((B, Le, D))).astype(np.float32)
    return mu, lv


def live_masks(B, Le, seed):
    """name -> live [B, Le] (None: no mask): random 70 % live, one molecule fully dead, all dead."""
    rng = np.random.default_rng(seed + 1000)
    one_dead = np.ones((B, Le), dtype=bool)
    one_dead[B // 2] = False
    return {"none": None, "random": rng.random((B, Le)) < 0.7, "one_dead": one_dead,
            "all_dead": np.zeros((B, Le), dtype=bool)}
