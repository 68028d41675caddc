"""fp64 reference, derived error bounds, input families, an fp32 restatement and its mutants for gct_norm_fwd /
gct_norm_bwd (tests/test_norm_ref_host.py runs them on the CPU, tests/test_norm_gpu.py holds the kernels to them).

Reference, per row of width d (the reference's Norm: unbiased std, eps added to the STD), all in fp64:

    m = mean(x)   c = x - m   sigma = sqrt(sum c^2 / (d - 1))   r = 1 / (sigma + eps)   y = alpha * (c * r) + bias
    (dx, dalpha, dbias) = autograd of sum(y * dy);  dx += dres when a residual gradient is given.

eps is the fp32 value the kernel receives (1e-6 is not a binary fraction; the reference uses its fp32 rounding).

Inputs (FAMILIES, seeded functions of (rows, d)): unit randn; offset (1000 + randn: mean = 1000 sigma); sigma = 1e-6
(the default eps); sigma = 1e-7 (below eps); 0.5 + 1e-5 randn (sigma of a few hundred ulps of the values); randn * 1e12;
randn * 1e-12; a mixed batch whose row i is drawn like family i % 7.  The squares and sums of every family stay in
fp32's normal range (1e-12^2 = 1e-24, 2048 * (5e12)^2 < 1e29; a centred value that happens to lie within 1e-7 sigma of
zero has a square 1e-14 of its row's sum, which no fp32 sum notices): nothing here pins behaviour on denormals, which
the kernels may flush.

Bounds (bounds() below: functions of the data, evaluated in fp64, elementwise).  u = 2^-24, X = max |x| of the row,
K_* = the constants of the table further down.  A row sum is a tree of depth <= 2 + 8 + 6 (four elements of a chunk,
<= 8 chunks of a lane, 64 lanes), so its relative error is a small multiple of u times the sum of absolute values.

  mean    E_m = K_mean u X.  The sum's error is (depth) u sum|x| / d <= (depth) u X; measured it is a few u X.
  rstd    The centred values are c_i' = (x_i - m')(1 + u): a common shift by dm = m' - m and one rounding each.  The
          roundings of c', of the squares, of their sum, of the division, the square root, the sum with eps and the
          reciprocal are relative: K_rstd u r in all.  The shift is NOT first order in u: sum (c_i - dm)^2 =
          sum c_i^2 + d dm^2 (sum c_i = 0), so sigma' = sqrt(sigma^2 + dm^2 d / (d - 1)); with shift =
          sqrt(sigma^2 + E_m^2 d / (d - 1)) - sigma and dr = -r r' dsigma:
              E_r = K_rstd u r + r^2 shift.
          (For the 0.5 + 1e-5 randn rows dm is half an ulp of 0.5 = 3e-8, and (3e-8)^2 / (2 sigma^2) = 75 u: the
          largest term there.)
  y       y = alpha (c r) + bias: three roundings on top of those of c and r, and the first-order effect of dm and dr:
              E_y = K_y u (|alpha| |c| r + |bias|) + |alpha| r E_m + |alpha| |c| E_r.
          The middle term is K_mean u |alpha| X / (sigma + eps): what governs the error of y is max |x| / (sigma + eps),
          not |y|.
  dx      dx = r (g - gbar) - c k2 [+ dres], g = dy alpha, gbar = sum g / d, s2 = sum g c,
          k2 = s2 r^2 / (sig (d - 1)), sig = 1 / r - eps.  t1 = r (g - gbar), t2 = c k2, T2 = |c| (sum |g| |c|) r^2 /
          (sigma (d - 1)) (the absolute-value version of t2):
              roundings     K_dx u (r (|g| + sum |g| / d) + T2 + |dres|)
              dr in t1      E_r |g - gbar|
              dm, dr in t2  E2 = E_m (|s2| + |c| sum |g|) r^2 / (sigma (d - 1)) + 2 (E_r / r) |t2|
                            (c_i' = c_i - dm moves the factor c_i and every term of s2; r enters squared)
              1/r - eps     sig' = fl(fl(1 / r') - eps): the error of 1 / r', and one rounding each of the division and
                            of the difference (none where the two are within a factor 2): E_sig = E_r / r^2 + 2 u / r.  t2 is
                            proportional to 1 / sig, so t2' = t2 sigma / sig': |t2' - t2| = |t2| |sig' - sigma| / sig'.
                            sig' is a multiple of the ulp of the smaller of 1 / r' and eps, so sig' > 0 implies
                            sig' >= u eps; sig' <= 0 makes the kernel's guard drop t2 altogether (error |t2|).  Hence
                                amp = E_sig / max(sigma - E_sig, u eps),   error <= amp (|t2| + E2),
                            which also covers the guard: sigma - E_sig <= u eps gives amp >= 4.
              E_dx = the sum of the four.
          Where sigma = 0 (a constant row) d sigma / dx does not exist; the kernel's dx is r (g - gbar) [+ dres]
          (c = 0 wipes t2 whatever the guard does; torch.std's backward puts 0 there, so autograd says the same), and
          E_dx keeps the first two lines only.
  dalpha  dalpha_j = sum_rows dy c r, each output summed in n = rows per wave + 4 waves + norm_blocks(rows) steps
          (a wave's rows one after the other, the block's 4 waves, one slab per block):
              E_da = K_da n u sum_rows |dy| |c| r + sum_rows |dy| (r E_m + |c| E_r).
  dbias   E_db = K_db n u sum_rows |dy|.

How the constants were set.  Measured on the CPU against kernel32() below -- an fp32 plain-torch restatement of the
kernels' formulas: two-pass statistics, r = 1 / (sqrt(var) + eps), sigma = 1 / r - eps, the k2 guard -- over every family,
every width of WIDTHS, eps = 1e-6 and 1e-2, with and without dres, rows = 37.  K_mean and K_rstd first (they enter the
other bounds), then the rest; each is the smallest convenient number that leaves the worst error / bound at or below
0.5, i.e. a margin of 2 x: the kernels sum in another order than torch, and 2 x covers a different tree of the same
depth.  tests/test_norm_ref_host.py asserts the 0.5.

    constant   value   worst error / bound of kernel32 (family, d, eps)
    K_mean      6      0.440  (offset, d = 12, eps = 1e-6)
    K_rstd      8      0.400  (offset, d = 1540, eps = 1e-6)
    K_y         3      0.440  (offset, d = 12, eps = 1e-6; with K_y = 2: 0.499 on sigma-eps, d = 1540, eps = 1e-2,
                              where y is all but bias and one rounding of the result is 0.5 of 2 u |bias|)
    K_dx        4      0.399  (0.5 + 1e-5 randn, d = 768, eps = 1e-6, with dres)
    K_dalpha    1      0.265  (mixed, d = 768, eps = 1e-6)    one rounding per addend: the derivation's own constant,
    K_dbias     1      0.086  (unit, d = 2048, eps = 1e-6)    not lowered to what the measurement would allow

The mutants (MUTANTS: kernel32 with one mistake each) exceed a bound by (rows = 37; quantity, family, d, eps where):
    fwd-rsqrt-var-plus-eps   2.1e6  (rstd, scale-1e-12, 4, 1e-6)     bwd-sigma-is-1-over-r    1.3e5  (dx, sigma-eps, 4, 1e-6)
    fwd-biased-variance      3.2e5  (rstd, scale-1e12, 4, 1e-2)      bwd-k2-over-d            8.0e4  (dx, unit, 4, 1e-6)
    fwd-one-pass-variance    5.7e11 (rstd, offset, 4, 1e-6)          bwd-s1-of-dy             4.2e6  (dx, scale-1e-12, 4, 1e-2)
    bwd-dres-dropped         4.2e6  (dx, scale-1e12, 2048, 1e-6)     bwd-dalpha-without-r     2.5e17 (dalpha, scale-1e12, 2048, 1e-2)
On unit randn rows at eps = 1e-6 and d >= 12 the two eps mutants stay inside the bounds of y, dx, dalpha and dbias (at most
0.90 x); rstd itself shows the forward one at 1.3 x, and d = 4, where a row's sigma can be 0.1, at 8 x (y)."""
import functools
from collections import namedtuple

import torch

from tests.wgrad_ref import ratio                              # worst |got - want| / bound, inf where not finite

U = 2.0 ** -24
WIDTHS = (4, 12, 252, 256, 260, 508, 512, 516, 768, 1024, 1028, 1280, 1540, 2044, 2048)
EPSES = (1e-6, 1e-2)
ROWS = 37
K = dict(mean=6.0, rstd=8.0, y=3.0, dx=4.0, dalpha=1.0, dbias=1.0)
QUANTITIES = ("y", "mean", "rstd", "dx", "dalpha", "dbias")
Out = namedtuple("Out", QUANTITIES)                            # a result, a reference or a set of bounds


def eps32(eps):
    """the value the kernel receives: eps rounded to fp32"""
    return float(torch.tensor(eps, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ input families
def _randn(rows, d, seed):
    return torch.randn(rows, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


_PLAIN = (
    ("unit", lambda z: z),
    ("offset", lambda z: z + 1000.0),
    ("sigma-eps", lambda z: z * 1e-6),
    ("sigma-below-eps", lambda z: z * 1e-7),
    ("half-1e-5", lambda z: z * 1e-5 + 0.5),
    ("scale-1e12", lambda z: z * 1e12),
    ("scale-1e-12", lambda z: z * 1e-12),
)


def _mixed(z):
    out = torch.empty_like(z)
    for i, (_, f) in enumerate(_PLAIN):
        out[i::len(_PLAIN)] = f(z[i::len(_PLAIN)])
    return out


FAMILIES = dict(_PLAIN + (("mixed", _mixed),))


def family_x(name, rows, d):
    """x [rows][d] fp32 of a family (the same draw for every family: only the map differs)"""
    return FAMILIES[name](_randn(rows, d, 100 + d))


Problem = namedtuple("Problem", "x alpha bias dy dres eps")


def problem(name, rows, d, eps, with_dres=True):
    """the operands of one forward + backward call, fp32 on the CPU"""
    return Problem(family_x(name, rows, d), _randn(1, d, 2)[0] + 1.0, _randn(1, d, 3)[0], _randn(rows, d, 4),
                   _randn(rows, d, 5) if with_dres else None, eps32(eps))


# ------------------------------------------------------------------------------------------------ reference
def reference(p):
    """Out of the reference's Norm and of autograd through it, fp64"""
    x, a, b = (t.double().requires_grad_() for t in (p.x, p.alpha, p.bias))
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / (x.std(-1, keepdim=True) + p.eps)             # torch.std: unbiased
    y = a * (x - mean) * rstd + b
    y.backward(p.dy.double())
    dx = x.grad if p.dres is None else x.grad + p.dres.double()
    return Out(y.detach(), mean.detach()[:, 0], rstd.detach()[:, 0], dx, a.grad, b.grad)


def norm_blocks(rows):
    return min(max((rows + 3) // 4, 1), 1024)


def addends(rows):
    """steps in which one dalpha / dbias output is summed: the rows of a wave, 4 waves, one slab per block"""
    quads = (rows + 3) // 4
    nblk = norm_blocks(rows)
    return 4 * ((quads + 4 * nblk - 1) // (4 * nblk)) + 4 + nblk


def bounds(p, n=None, rows=None):
    """Out of the elementwise bounds of the module docstring.  n: addends of dalpha / dbias (default: of p's rows);
    rows (bool [rows]): the rows that dalpha / dbias sum over (default: all)"""
    x, a, b, dy = p.x.double(), p.alpha.double(), p.bias.double(), p.dy.double()
    d, eps = x.shape[1], p.eps
    n = addends(x.shape[0]) if n is None else n
    col = lambda t: t[:, None]                                 # noqa: E731
    m = x.mean(-1)
    c = x - col(m)
    sigma = (c * c).sum(-1).div(d - 1).sqrt()
    r = 1.0 / (sigma + eps)
    X = x.abs().amax(-1)
    f = d / (d - 1.0)

    E_m = K["mean"] * U * X
    root = (sigma * sigma + E_m * E_m * f).sqrt()
    shift = torch.where(root > 0, E_m * E_m * f / (root + sigma).clamp_min(1e-300), 0.0)
    E_r = K["rstd"] * U * r + r * r * shift
    E_y = K["y"] * U * (a.abs() * c.abs() * col(r) + b.abs()) + a.abs() * col(r * E_m) + a.abs() * c.abs() * col(E_r)

    g = dy * a
    gbar = g.mean(-1)
    s2 = (g * c).sum(-1)
    live = sigma > 0
    scale = torch.where(live, r * r / (sigma.clamp_min(1e-300) * (d - 1)), 0.0)     # sigma = 0: t2 = 0, no t2 terms
    t2 = c.abs() * col(s2.abs() * scale)
    T2 = c.abs() * col((g.abs() * c.abs()).sum(-1) * scale)
    rounding = K["dx"] * U * (col(r) * (g.abs() + col(g.abs().mean(-1))) + T2 + (0 if p.dres is None else p.dres.double().abs()))
    E2 = col(E_m * scale) * (col(s2.abs()) + c.abs() * col(g.abs().sum(-1))) + 2 * col(E_r / r) * t2
    E_sig = E_r / (r * r) + 2 * U / r
    amp = E_sig / (sigma - E_sig).clamp_min(U * eps)
    E_dx = rounding + col(E_r) * (g - col(gbar)).abs() + E2 + col(torch.where(live, amp, 0.0)) * (t2 + E2)

    w = dy.abs() if rows is None else dy.abs() * col(rows.double())
    E_da = K["dalpha"] * n * U * (w * c.abs() * col(r)).sum(0) + (w * (col(r * E_m) + c.abs() * col(E_r))).sum(0)
    E_db = K["dbias"] * n * U * w.sum(0)
    return Out(E_y, E_m, E_r, E_dx, E_da, E_db)


def ratios(got, ref, bnd):
    """quantity -> worst error / bound"""
    return {q: ratio(getattr(got, q), getattr(ref, q), getattr(bnd, q)) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def case(name, rows, d, eps, with_dres):
    """(problem, reference, bounds) of one case, computed once"""
    p = problem(name, rows, d, eps, with_dres)
    return p, reference(p), bounds(p)


# ------------------------------------------------------------------------------------------------ fp32 restatement
FWD_MUTANTS = ("fwd-rsqrt-var-plus-eps", "fwd-biased-variance", "fwd-one-pass-variance")
BWD_MUTANTS = ("bwd-sigma-is-1-over-r", "bwd-k2-over-d", "bwd-s1-of-dy", "bwd-dres-dropped", "bwd-dalpha-without-r")
MUTANTS = FWD_MUTANTS + BWD_MUTANTS
EPS_MUTANTS = ("fwd-rsqrt-var-plus-eps", "bwd-sigma-is-1-over-r")


def kernel32(p, mutant=None):
    """Out of the kernels' formulas in fp32 plain torch (mutant: with that one mistake).  The backward reads the
    mean and rstd the forward produced, as the kernels' callers do."""
    assert mutant is None or mutant in MUTANTS, mutant
    x, a, b, dy, eps = p.x, p.alpha, p.bias, p.dy, torch.tensor(p.eps, dtype=torch.float32)
    d = x.shape[1]
    mean = x.sum(-1, keepdim=True) / d
    c = x - mean
    if mutant == "fwd-one-pass-variance":
        var = (((x * x).sum(-1, keepdim=True) / d - mean * mean) * (d / (d - 1.0))).clamp_min(0.0)
    else:
        var = (c * c).sum(-1, keepdim=True) / (d if mutant == "fwd-biased-variance" else d - 1)
    r = torch.rsqrt(var + eps) if mutant == "fwd-rsqrt-var-plus-eps" else 1.0 / (var.sqrt() + eps)
    y = a * (c * r) + b

    g = dy * a
    s1 = (dy if mutant == "bwd-s1-of-dy" else g).sum(-1, keepdim=True) / d
    s2 = (g * c).sum(-1, keepdim=True)
    sigma = 1.0 / r if mutant == "bwd-sigma-is-1-over-r" else 1.0 / r - eps
    k2 = torch.where(sigma > 0, s2 * r * r / (sigma * (d if mutant == "bwd-k2-over-d" else d - 1)), torch.zeros(()))
    dx = r * (g - s1) - c * k2
    if p.dres is not None and mutant != "bwd-dres-dropped":
        dx = dx + p.dres
    dalpha = (dy * c if mutant == "bwd-dalpha-without-r" else dy * c * r).sum(0)
    return Out(y, mean[:, 0], r[:, 0], dx, dalpha, dy.sum(0))
