"""The loss, latent, embedding, optimizer and utility kernels (ce.hip, vae.hip, embed.hip, adam.hip, small.hip and
add / copy_rows / nonzero_row_tiles of reduce.hip) at the sizes where their code takes another path: grid wrap-around,
vector tails, second trips of column loops, the largest LDS table, clamped ids, absent optional operands.

References are fp64 on the CPU.  Tolerances are those of tests/test_kernels_gpu.py for the same kernel; the absolute
part of a sum grows with sqrt(terms / terms of that test), as test_norm does with sqrt(rows).  Outputs are allocated
here and filled with NaN (integers: -1) before the call, so an element that the kernel never wrote fails."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd._lib import check
from tests.test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def ratio(got, ref, atol, rtol, what):
    """max |got - ref| / (atol + rtol |ref|); asserts <= 1 and that everything was written."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} elements not finite (never written?)"
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = float((err / (atol + rtol * ref.abs())).max())
    assert r <= 1.0, f"{what}: error {r:.3f} x tolerance (max err {float(err.max()):.3e}, ref scale {float(ref.abs().max()):.3e})"
    return r


# ------------------------------------------------------------------------------------------ raw entry points
def ce_fwd(ops, logits, tgt, pad):
    out = nans()
    ws = ops.workspace(4096, logits.device)
    check(ops._L().gct_ce_fwd(logits.data_ptr(), tgt.data_ptr(), out.data_ptr(), ws.data_ptr(), logits.shape[0],
                              logits.shape[1], pad, ops._st()), "gct_ce_fwd")
    return out


def ce_bwd(ops, logits, tgt, gout, pad):
    dl = nans(*logits.shape)
    check(ops._L().gct_ce_bwd(logits.data_ptr(), tgt.data_ptr(), gout.data_ptr(), dl.data_ptr(), logits.shape[0],
                              logits.shape[1], pad, ops._st()), "gct_ce_bwd")
    return dl


def kld_fwd(ops, mu, lv):
    out = nans()
    ws = ops.workspace(4096, mu.device)
    check(ops._L().gct_kld_fwd(mu.data_ptr(), lv.data_ptr(), out.data_ptr(), ws.data_ptr(), mu.numel(), ops._st()),
          "gct_kld_fwd")
    return out


def kld_bwd(ops, mu, lv, gout):
    dmu, dlv = nans(*mu.shape), nans(*mu.shape)
    check(ops._L().gct_kld_bwd(mu.data_ptr(), lv.data_ptr(), gout.data_ptr(), dmu.data_ptr(), dlv.data_ptr(), mu.numel(),
                               ops._st()), "gct_kld_bwd")
    return dmu, dlv


def reparam_fwd(ops, mu, lv, eps, seed, site):
    z, eo = nans(*mu.shape), nans(*mu.shape)
    check(ops._L().gct_reparam_fwd(mu.data_ptr(), lv.data_ptr(), None if eps is None else eps.data_ptr(), eo.data_ptr(),
                                   z.data_ptr(), mu.numel(), seed, site, ops._st()), "gct_reparam_fwd")
    return z, eo


def embed_fwd(ops, tok, table, cond, pe, n_c, scale, p, seed, site, d, vocab):
    B, S = tok.shape
    out = nans(B * (S + n_c), d)
    check(ops._L().gct_embed_pe_fwd(ops._p(tok), ops._p(table), ops._p(cond), pe.data_ptr(), out.data_ptr(), B, S, n_c, d,
                                    vocab, scale, p, seed, site, ops._st()), "gct_embed_pe_fwd")
    return out


# ------------------------------------------------------------------------------------------------------ CE
PAD = 1
CE_TERMS_EXISTING = 266          # non-pad rows of test_reparam_kld_ce's 333


def _ce_reference(lg64, tgt, g):
    """fp64 sum-reduced cross-entropy over the rows whose target is not PAD, and (autograd) g * d/dlogits."""
    V = lg64.shape[1]
    lg = lg64.clone().requires_grad_()
    valid = tgt != PAD
    assert bool(((tgt >= 0) & (tgt < V))[valid].all())
    lse = torch.logsumexp(lg, 1)
    picked = lg.gather(1, tgt.clamp(0, V - 1)[:, None])[:, 0]
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    (g * loss).backward()
    return loss.detach(), lg.grad


def _targets(rows, V, share, seed):
    g = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([t for t in range(V) if t != PAD], dtype=torch.int64)
    tgt = allowed[torch.randint(0, len(allowed), (rows,), generator=g)]
    if share == "all":
        tgt[:] = PAD
    elif share:
        tgt[torch.rand(rows, generator=g) < share] = PAD
        tgt[rows // 2] = PAD
    return tgt


@pytest.mark.parametrize("V", [1, 2, 31, 64, 65, 130])
def test_ce_sizes_pad_shares_and_scales(ops, V):
    """rows 4101 wraps ce_fwd's grid (1024 workgroups x 4 rows), 16390 wraps ce_bwd's (4096 x 4); V > 64 takes a second
    trip of the column loops; logits of scale 80 overflow expf without the max subtraction."""
    g = 1.7
    gout = torch.tensor(g, device=DEV)
    worst = {"ce": 0.0, "dlogits": 0.0}
    for rows in (1, 3, 4101, 16390):
        for share in (0.0, 0.2, "all"):
            for scale in (2.0, 80.0):
                what = f"V={V} rows={rows} pad={share} scale={scale}"
                logits = rnd(rows, V, seed=rows + V, scale=scale)
                tgt = _targets(rows, V, share, seed=rows)
                ref, dref = _ce_reference(logits.double(), tgt, g)
                lgd, tgd = logits.to(DEV), tgt.to(DEV)
                got, dl = ce_fwd(ops, lgd, tgd, PAD), ce_bwd(ops, lgd, tgd, gout, PAD)
                terms = int((tgt != PAD).sum())
                atol = 1e-3 * max(1.0, math.sqrt(terms / CE_TERMS_EXISTING))
                worst["ce"] = max(worst["ce"], ratio(got, ref, atol, 1e-6, f"ce {what}"))
                worst["dlogits"] = max(worst["dlogits"], ratio(dl, dref, 1e-6, 1e-5, f"ce_bwd {what}"))
                if share == "all":
                    assert got.item() == 0.0 and not dl.any(), what
                else:
                    assert not dl.cpu()[tgt == PAD].any(), f"pad rows of dlogits: {what}"
    print(f"ce V={V}: worst error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("V", [2, 31, 65, 130])
def test_ce_with_minus_infinity_logits(ops, V):
    """-inf at about 10 % of the non-target positions of every row (a masked vocabulary): the loss is finite and the
    gradient is exactly 0 there."""
    rows, g = 517, 0.5
    logits = rnd(rows, V, seed=V, scale=2.0)
    tgt = _targets(rows, V, 0.2, seed=3)
    hole = torch.rand(rows, V, generator=torch.Generator().manual_seed(V)) < 0.1
    hole[:, 0] |= V > 2                              # every row has one (V = 2: only where the draw says so)
    hole[torch.arange(rows), tgt.clamp(0, V - 1)] = False
    logits[hole] = -math.inf
    ref, dref = _ce_reference(logits.double(), tgt, g)
    assert torch.isfinite(ref) and torch.isfinite(dref).all()
    lgd, tgd = logits.to(DEV), tgt.to(DEV)
    got, dl = ce_fwd(ops, lgd, tgd, PAD), ce_bwd(ops, lgd, tgd, torch.tensor(g, device=DEV), PAD)
    terms = int((tgt != PAD).sum())
    r0 = ratio(got, ref, 1e-3 * max(1.0, math.sqrt(terms / CE_TERMS_EXISTING)), 1e-6, f"ce with -inf V={V}")
    r1 = ratio(dl, dref, 1e-6, 1e-5, f"ce_bwd with -inf V={V}")
    assert hole.any() and not dl.cpu()[hole].any(), "gradient at a -inf logit"
    print(f"ce -inf V={V}: worst error / tolerance ce {r0:.3f}, dlogits {r1:.3f}")


@pytest.mark.parametrize("V", [1, 31, 65])
def test_ce_target_outside_the_vocabulary(ops, V):
    """What include/gctplus_hip.h states: a target that is neither pad nor in [0, V) adds nothing to the loss, and its
    gradient row is g * softmax (no one-hot term)."""
    rows, g = 41, 1.7
    logits = rnd(rows, V, seed=5, scale=2.0)
    tgt = _targets(rows, V, 0.2, seed=6)
    out_of_range = {3: V + 3, 10: -7, 40: V + (V == PAD), 17: 1 << 40}       # V itself, unless that is the pad id
    for r, t in out_of_range.items():
        tgt[r] = t
    oor = torch.zeros(rows, dtype=torch.bool)
    oor[list(out_of_range)] = True
    inside = tgt.clone()
    inside[oor] = PAD                                 # the reference skips them ...
    ref, dref = _ce_reference(logits.double(), inside, g)
    dref[oor] = g * torch.softmax(logits.double()[oor], 1)       # ... and the kernel's documented gradient row
    lgd, tgd = logits.to(DEV), tgt.to(DEV)
    ratio(ce_fwd(ops, lgd, tgd, PAD), ref, 1e-3, 1e-6, f"ce with out-of-range targets V={V}")
    ratio(ce_bwd(ops, lgd, tgd, torch.tensor(g, device=DEV), PAD), dref, 1e-6, 1e-5, f"ce_bwd with out-of-range targets V={V}")


# ----------------------------------------------------------------------------------------------------- KLD
@pytest.mark.parametrize("n", [1, 255, 257, 262144 + 5, 3_000_000])
def test_kld_sizes(ops, n):
    """262144 elements fill kld_fwd's grid (1024 x 256) once: above, threads loop.  log_var in [-8, 4]."""
    g = torch.Generator().manual_seed(n)
    mu = torch.randn(n, generator=g)
    lv = torch.rand(n, generator=g) * 12 - 8
    md, ld = mu.double().requires_grad_(), lv.double().requires_grad_()
    ref = -0.5 * torch.sum(1 + ld - md.pow(2) - ld.exp())
    (0.04 * ref).backward()
    mug, lvg = mu.to(DEV), lv.to(DEV)
    got = kld_fwd(ops, mug, lvg)
    gm, gl = kld_bwd(ops, mug, lvg, torch.tensor(0.04, device=DEV))
    r0 = ratio(got, ref.detach(), 1e-3 * max(1.0, math.sqrt(n / 2576)), 1e-6, f"kld n={n}")       # 2576: test_reparam_kld_ce
    r1 = ratio(gm, md.grad, 1e-7, 1e-5, f"kld dmu n={n}")
    r2 = ratio(gl, ld.grad, 1e-7, 1e-5, f"kld dlv n={n}")
    print(f"kld n={n}: worst error / tolerance kld {r0:.3f}, dmu {r1:.3f}, dlv {r2:.3f}")


# ------------------------------------------------------------------------------------------------- reparam
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099])
def test_reparam_with_given_noise(ops, n):
    """n % 4 != 0 takes the tail of the 4-element threads; dmu_ext / dlv_ext each absent and present."""
    mu, lv, eps, dz = rnd(n, seed=1), rnd(n, seed=2, scale=0.5), rnd(n, seed=3), rnd(n, seed=4)
    e1, e2 = rnd(n, seed=5), rnd(n, seed=6)
    mug, lvg, epg, dzg = (t.to(DEV) for t in (mu, lv, eps, dz))
    z, eo = reparam_fwd(ops, mug, lvg, epg, 0, 0)
    worst = ratio(z, eps.double() * torch.exp(0.5 * lv.double()) + mu.double(), 1e-6, 1e-6, f"z n={n}")
    assert torch.equal(eo.cpu(), eps)
    for x1 in (None, e1):
        for x2 in (None, e2):
            dmu, dlv = nans(n), nans(n)
            ops.reparam_bwd(dzg, lvg, epg, None if x1 is None else x1.to(DEV), None if x2 is None else x2.to(DEV), dmu, dlv)
            what = f"n={n} dmu_ext={x1 is not None} dlv_ext={x2 is not None}"
            worst = max(worst, ratio(dmu, dz.double() + (0 if x1 is None else x1.double()), 1e-6, 1e-6, f"dmu {what}"))
            worst = max(worst, ratio(dlv, 0.5 * dz.double() * eps.double() * torch.exp(0.5 * lv.double())
                                     + (0 if x2 is None else x2.double()), 1e-6, 1e-5, f"dlv {what}"))
    print(f"reparam n={n}: worst error / tolerance {worst:.3f}")


# ----------------------------------------------------------------------------------------------- embedding
EMBED_TERMS_EXISTING = 100       # token rows of test_embed_pe (B = 5, S = 20)


def _embed_case(ops, B, S, d, V, n_c, tok=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    if tok is None:
        tok = torch.randint(0, V, (B, S), generator=g)
    table, pe = rnd(V, d, seed=1), rnd(S + n_c + 3, d, seed=2)
    cond = rnd(B, n_c, d, seed=3) if n_c else None
    scale = math.sqrt(d)
    tc = tok.clamp(0, V - 1)                             # what the kernels do with an id outside [0, V)
    x = table.double()[tc]
    if n_c:
        x = torch.cat([cond.double(), x], 1)
    ref = x * float(np.float32(scale)) + pe.double()[: S + n_c]
    to = lambda t: None if t is None else t.to(DEV)                                                 # noqa: E731
    out = embed_fwd(ops, tok.to(DEV), to(table), to(cond), pe.to(DEV), n_c, scale, 0.0, 0, 0, d, V)
    what = f"B={B} S={S} d={d} V={V} n_c={n_c}"
    r_f = ratio(out.view(B, S + n_c, d), ref, 1e-6, 1e-6, f"embed fwd {what}")
    dout = rnd(B * (S + n_c), d, seed=4)
    dd = dout.double().view(B, S + n_c, d) * float(np.float32(scale))
    exp = torch.zeros(V, d, dtype=torch.double)
    exp.index_add_(0, tc.reshape(-1), dd[:, n_c:].reshape(-1, d))
    dtable = nans(V, d)
    dcond = nans(B, n_c, d) if n_c else None
    ops.embed_pe_bwd(dout.to(DEV), tok.to(DEV), dtable, dcond, n_c, scale, 0.0, 0, 0)
    r_t = ratio(dtable, exp, 1e-4 * max(1.0, math.sqrt(B * S / EMBED_TERMS_EXISTING)), 1e-5, f"embed dtable {what}")
    r_c = ratio(dcond, dd[:, :n_c], 1e-5, 1e-5, f"embed dcond {what}") if n_c else 0.0
    return r_f, r_t, r_c


@pytest.mark.parametrize("V", [1, 31, 64])
@pytest.mark.parametrize("d", [4, 260, 512])
def test_embed_vocab_width_and_cond_rows(ops, V, d):
    """V = 64 is the largest LDS table (64 KB of dynamic LDS); d = 260 has a second column block of 4 live columns;
    n_c = 9 is more than the 8 rows gct_embed_ws_bytes allows for; B * L % 4 != 0 leaves a ragged last quad."""
    worst = [0.0, 0.0, 0.0]
    for n_c in (0, 3, 9):
        for B, S in ((3, 7), (5, 20)):
            worst = [max(a, b) for a, b in zip(worst, _embed_case(ops, B, S, d, V, n_c))]
    print(f"embed V={V} d={d}: worst error / tolerance fwd {worst[0]:.3f}, dtable {worst[1]:.3f}, dcond {worst[2]:.3f}")


def test_embed_ids_outside_the_table_are_clamped(ops):
    V, B, S = 31, 4, 9
    tok = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(2))
    tok[0, 0], tok[1, 3], tok[3, 8], tok[2, 2] = -1, V + 5, V, -(1 << 40)
    _embed_case(ops, B, S, 64, V, 3, tok=tok)
    _embed_case(ops, B, S, 260, V, 0, tok=tok)


def test_embed_many_row_groups_per_chunk(ops):
    """B * (S + 8) / 64 > 512 chunks: the chunk count is capped, every chunk walks 18 row groups."""
    B, S, n_c = 700, 50, 3
    assert ((B * (S + 8)) // 4 + 15) // 16 > 512 and -(-((B * (S + n_c) + 3) // 4) // 512) > 16
    r = _embed_case(ops, B, S, 64, 31, n_c)
    print(f"embed B={B} S={S}: worst error / tolerance fwd {r[0]:.3f}, dtable {r[1]:.3f}, dcond {r[2]:.3f}")
    r = _embed_case(ops, 40, 50, 8, 5, 0)          # several chunks below the cap: 37 of 14 row groups
    print(f"embed B=40 S=50: worst error / tolerance fwd {r[0]:.3f}, dtable {r[1]:.3f}")


@pytest.mark.parametrize("d", [4, 260])
def test_embed_positional_encoding_alone(ops, d):
    """S = 0: x * scale + pe over the cond rows, no table, no token ids (the standalone PositionalEncoding)."""
    B, n_c, scale = 7, 3, 1.5
    cond, pe = rnd(B, n_c, d, seed=3), rnd(n_c, d, seed=2)
    tok = torch.empty(B, 0, dtype=torch.int64, device=DEV)
    out = embed_fwd(ops, tok, None, cond.to(DEV), pe.to(DEV), n_c, scale, 0.0, 0, 0, d, 1)
    ratio(out.view(B, n_c, d), cond.double() * scale + pe.double(), 1e-6, 1e-6, f"PE alone fwd d={d}")
    dout = rnd(B * n_c, d, seed=4)
    dcond = nans(B, n_c, d)
    ops.embed_pe_bwd(dout.to(DEV), tok, None, dcond, n_c, scale, 0.0, 0, 0, d=d)
    ratio(dcond, dout.double().view(B, n_c, d) * scale, 1e-5, 1e-5, f"PE alone bwd d={d}")


# ---------------------------------------------------------------------------------------------------- Adam
def _adam_reference(p, g, m, v, lr, b1, b2, eps, step, gscale):
    """The rule of include/gctplus_hip.h in fp64, on the float32 values of the scalars the kernel is given."""
    lr, b1, b2, eps, gscale = (float(np.float32(x)) for x in (lr, b1, b2, eps, gscale))
    p, g, m, v = p.double(), g.double() * gscale, m.double(), v.double()
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** step) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v


LR, B1, B2, EPS = 1e-4, 0.9, 0.98, 1e-9


def _adam_run(ops, p, g, m, v, steps, gscale, what):
    pg, mg, vg, gg = p.to(DEV).clone(), m.to(DEV).clone(), v.to(DEV).clone(), g.to(DEV)
    worst = 0.0
    for step in steps:
        # the reference restarts from the device's state: one step's error, not the accumulated drift
        ref = _adam_reference(pg.cpu(), g, mg.cpu(), vg.cpu(), LR, B1, B2, EPS, step, gscale)
        ops.adam_step(pg, gg, mg, vg, LR, B1, B2, EPS, step, gscale=gscale, guard=False)
        worst = max(worst, ratio(pg, ref[0], 1e-7, 1e-6, f"adam p {what} step={step}"),
                    ratio(mg, ref[1], 1e-7, 1e-5, f"adam m {what} step={step}"),
                    ratio(vg, ref[2], 1e-9, 1e-5, f"adam v {what} step={step}"))
    return worst, pg, mg, vg


@pytest.mark.parametrize("n", [1, 3, 4, 5, 10007])
def test_adam_sizes_and_gradient_scale(ops, n):
    """n % 4 != 0: the scalar tail; gscale = 0.25; from a zero state (steps 1..3) and from a running one (step 20000,
    where both bias corrections are 1)."""
    p, g = rnd(n, seed=1), rnd(n, seed=2)
    z = torch.zeros(n)
    w1, *_ = _adam_run(ops, p, g, z, z, (1, 2, 3), 0.25, f"n={n} cold")
    w2, *_ = _adam_run(ops, p, g, rnd(n, seed=3, scale=0.1), rnd(n, seed=4).square() * 0.01, (20000,), 0.25, f"n={n} warm")
    # gradients of 1e-10: sqrt(v) << eps = 1e-9, the update is lr * m / eps
    w3, *_ = _adam_run(ops, p, g * 1e-10, z, z, (1, 20000), 0.25, f"n={n} tiny gradients")
    print(f"adam n={n}: worst error / tolerance {max(w1, w2, w3):.3f}")


@pytest.mark.parametrize("step", [1, 20000])
def test_adam_zero_gradient_leaves_the_parameters(ops, step):
    n = 1031
    p, z = rnd(n, seed=1), torch.zeros(n)
    _, pg, mg, vg = _adam_run(ops, p, z, z, z, (step,), 0.25, "zero gradient")
    assert torch.equal(pg.cpu(), p) and not mg.any() and not vg.any()       # 0 / (0 + eps): no NaN, no step


def test_adam_grid_wraps(ops):
    """8192 workgroups x 256 threads x 4 elements = 8192 * 1024: seven more elements send threads round again."""
    n = 8192 * 1024 + 7
    g_ = torch.Generator().manual_seed(9)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m, v = torch.randn(n, generator=g_) * 0.1, torch.rand(n, generator=g_) * 0.01
    w, *_ = _adam_run(ops, p, g, m, v, (7,), 0.25, f"n={n}")
    print(f"adam n={n}: worst error / tolerance {w:.3f}")


# -------------------------------------------------------------------------------------------- small linear
@pytest.mark.parametrize("rows,K,N", [(1, 1, 1), (37, 8, 192), (2100, 3, 512)])
def test_small_linear_shapes(ops, rows, K, N):
    """2100 x 512 outputs wrap the forward grid (4096 x 256); bias and bias gradient each absent and present."""
    x, w, b, dy = rnd(rows, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(rows, N, seed=4)
    xg, wg, bg, dyg = (t.to(DEV) for t in (x, w, b, dy))
    worst = 0.0
    for bias in (bg, None):
        y = nans(rows, N)
        check(ops._L().gct_small_linear_fwd(xg.data_ptr(), wg.data_ptr(), ops._p(bias), y.data_ptr(), rows, K, N, ops._st()),
              "gct_small_linear_fwd")
        ref = x.double() @ w.double().t() + (b.double() if bias is not None else 0.0)
        worst = max(worst, ratio(y, ref, 1e-5, 1e-5, f"small fwd bias={bias is not None}"))
    scale = max(1.0, math.sqrt(rows / 37))                              # 37 rows in test_small_linear_and_copy_rows
    for with_db in (True, False):
        dw, db = nans(N, K), nans(N)
        ops.small_linear_bwd(dyg, xg, dw, db if with_db else None)
        worst = max(worst, ratio(dw, dy.double().t() @ x.double(), 1e-5 * scale, 1e-5, "small dw"))
        if with_db:
            worst = max(worst, ratio(db, dy.double().sum(0), 1e-5 * scale, 1e-5, "small db"))
        else:
            assert torch.isnan(db).all()
    print(f"small linear rows={rows} K={K} N={N}: worst error / tolerance {worst:.3f}")


def test_small_linear_backward_of_no_rows_is_zero(ops):
    K, N = 3, 192
    x, dy = torch.ones(4, K, device=DEV), torch.ones(4, N, device=DEV)      # an empty tensor has no address to pass
    dw, db = nans(N, K), nans(N)
    check(ops._L().gct_small_linear_bwd(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), 0, K, N, ops._st()),
          "gct_small_linear_bwd")
    assert not dw.any() and not db.any() and torch.isfinite(dw).all() and torch.isfinite(db).all()


# ------------------------------------------------------------------------------------------ copy_rows / add
def test_copy_rows_offsets_and_accumulate(ops):
    """Rows [src_off, src_off + rpb) of every src batch land at [dst_off, ...) of the dst batch; accumulate adds."""
    B, src_rpb, src_off, dst_rpb, dst_off, rpb, cols = 37, 9, 2, 11, 4, 5, 12
    src, base = rnd(B, src_rpb, cols, seed=1), rnd(B, dst_rpb, cols, seed=2)
    for accumulate in (False, True):
        dst = base.to(DEV).clone()
        ops.copy_rows(src.to(DEV), src_rpb, src_off, dst, dst_rpb, dst_off, B * rpb, rpb, cols, accumulate=accumulate)
        want = base.clone()
        part = src[:, src_off:src_off + rpb]
        want[:, dst_off:dst_off + rpb] = want[:, dst_off:dst_off + rpb] + part if accumulate else part
        assert torch.equal(dst.cpu(), want), f"accumulate={accumulate}"      # one fp32 add per element: exact
    # a last batch that is cut short: rows is not a multiple of rpb
    dst = nans(B, dst_rpb, cols)
    ops.copy_rows(src.to(DEV), src_rpb, src_off, dst, dst_rpb, dst_off, 2 * rpb + 3, rpb, cols)
    d = dst.cpu()
    assert torch.equal(d[:2, dst_off:dst_off + rpb], src[:2, src_off:src_off + rpb])
    assert torch.equal(d[2, dst_off:dst_off + 3], src[2, src_off:src_off + 3])
    d[:2, dst_off:dst_off + rpb] = NAN
    d[2, dst_off:dst_off + 3] = NAN
    assert torch.isnan(d).all(), "rows outside the copy were written"


@pytest.mark.parametrize("n", [1, 3, 5, (1 << 22) + 3])
def test_add_sizes(ops, n):
    """n % 4 != 0: the scalar tail; 2^22 + 3 elements wrap the grid (4096 x 256 x 4)."""
    a, b = rnd(n, seed=1), rnd(n, seed=2)
    buf = nans(n + 4)
    ops.add(a.to(DEV), b.to(DEV), out=buf[:n])
    assert torch.equal(buf[:n].cpu(), a + b) and torch.isnan(buf[n:]).all()


# --------------------------------------------------------------------------------------- nonzero_row_tiles
def _row_tiles(ops, x2d):
    rows, cols = x2d.shape
    nt = (rows + 31) // 32
    lst = torch.full((nt + 8,), -1, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    flags = torch.full((nt + 8,), 7, dtype=torch.uint8, device=DEV)
    check(ops._L().gct_nonzero_row_tiles(x2d.data_ptr(), x2d.stride(0), rows, cols, lst.data_ptr(), cnt.data_ptr(),
                                         flags.data_ptr(), ops._st()), "gct_nonzero_row_tiles")
    return lst.cpu().tolist(), int(cnt.item())


@pytest.mark.parametrize("rows", [31, 33, 32 * 1024 + 5])
def test_nonzero_row_tiles_patterns(ops, rows):
    """ld > cols (the columns behind `cols` are non-zero and must not count); more than 1024 tiles take a second trip of
    the compaction loop.  The list is ascending and exact, and so is the count; nothing is written behind it."""
    cols, ld = 4, 12
    nt = (rows + 31) // 32
    g = torch.Generator().manual_seed(rows)
    patterns = {"all zero": torch.zeros(rows, dtype=torch.bool), "all non-zero": torch.ones(rows, dtype=torch.bool),
                "last row": torch.arange(rows) == rows - 1, "random rows": torch.rand(rows, generator=g) < 0.01,
                "every 1000th tile": (torch.arange(rows) // 32) % 1000 == 999}
    for name, live in patterns.items():
        buf = torch.ones(rows, ld)
        buf[:, :cols] = 0.0
        col = torch.randint(0, cols, (rows,), generator=g)
        buf[torch.arange(rows)[live], col[live]] = -0.5
        lst, cnt = _row_tiles(ops, buf.to(DEV)[:, :cols])
        want = sorted(set((torch.arange(rows)[live] // 32).tolist()))
        assert cnt == len(want), f"{name}: count {cnt}, expected {len(want)}"
        assert lst[:cnt] == want, f"{name}: list"
        assert all(v == -1 for v in lst[cnt:]), f"{name}: wrote behind the count"
        assert len(want) <= nt
