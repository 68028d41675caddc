"""The distribution terms of a policy on the device: gct_seq_dist / gct_seq_dist_bwd against the rules
(decode.dist_reference / dist_grad_reference) in fp64 on the same fp32 logits; engine.SeqDistFn under autograd;
decode.sequence_policy against sequence_logp (bit for bit), a frozen prior (KL exactly 0) and the CPU oracle (values and
gradients); Train/finetune.reinforce_step with an entropy bonus and a KL penalty against the same steps on the oracle,
and with its defaults against the step made by hand; and Sampling.policy_terms.

Tolerances.
Forward kernel: tests/test_score_gpu.py's kernel tolerance, atol 1e-4 per token and tokens * 1e-4 per sequence -- the
arithmetic is that kernel's (x - m, expf, a V-term sum, logf) plus one p-weighted V-term sum of values <= 40.
Backward kernel: kernel_ratio of tests/test_seq_logp_grad_gpu.py, 1e-6 max|g| + 1e-5 |ref|, imported.  Its absolute part
was set for softmax - onehot; the rows here multiply p by log p + H, so the fp32 RULE (dist_grad_reference on the fp32
logits, CPU) was first measured against the fp64 rule at exactly these cases: its worst error is 2.69e-6 max|g| (2.03
times kernel_ratio's tolerance), so the absolute coefficient here is twice that, rounded up: 6e-6 (BWD_ABS below).
Device path against the oracle: the project's logits tolerance (atol 1e-4, rtol 1e-4) pushed through each
term: 1e-4 + sum_v |d term / d x_v| (1e-4 + 1e-4 |x_v|), plus the same sum over the prior's logits for the KL.  Model
gradients: tests/test_model_gpu.py's (rtol 1e-3 + 1e-5 max|g| per tensor + grad_floor).  Per update step: the loss-curve
tolerance, 1e-3 relative (mean_kl, which starts at exactly 0: plus 1e-6 absolute)."""
import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd._lib import GctError, check
from gct_plus_amd.decode import dist_grad_reference, dist_reference, sequence_logp, sequence_policy
from tests.test_mixed_scaffold_decode_gpu import PAD, TINY, build
from tests.test_model_gpu import assert_close, grad_floor
from tests.test_policy_terms_host import ENTROPY_COEF, KL_COEF, oracle_regularised_run, pick, scored_columns
from tests.test_score_gpu import close_sums, close_tokens, cu, kernel_case, target_rows
from tests.test_seq_logp_grad_gpu import kernel_ratio, policy_sampler, weights
from tests.test_seq_logp_grad_host import UPDATE_LR, UPDATE_STEPS
from tests.test_stream_decode_gpu import make_sampler

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 7.25


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


# ------------------------------------------------------------------------------ 1. gct_seq_dist / gct_seq_dist_bwd
SHAPES = [(1, 2, 2), (3, 8, 30), (3, 4, 65), (5, 200, 31), (2, 256, 5), (2, 9, 1024), (67, 5, 30), (300, 60, 30)]
VARIANTS = ["plain", "no_lens", "ld", "shift", "no_prior"]
WHICH = ["entropy", "token_entropy", "kl", "token_kl", "all"]

# The absolute coefficient of the backward tolerance, in units of max|g| (kernel_ratio's own is 1e-6).  Measured on the
# RULE, never on the kernel: dist_grad_reference evaluated in fp32 on the CPU against itself in fp64, on the fp32 logits
# and weights of every case below (SHAPES x VARIANTS x WHICH).  Under kernel_ratio's own tolerance the fp32 rule's worst
# ratio is 2.03 -- (300, 60, 30) no_lens kl -- which exceeds 0.5; its worst error / max|g| is 2.69e-6 -- (5, 200, 31)
# no_lens kl --, so the coefficient is twice that, rounded up to one digit.
BWD_ABS = 6e-6


def dist_kernel_case(n, W, V, variant):
    """kernel_case's rows and agent logits (ties, a -1e4 logit), an independent draw for the prior, a -inf at index 1 of
    row 0's first logits row (scored) in both, and the weight tables: (g_entropy, g_token_entropy, g_kl, g_token_kl),
    each pair with zeros and one that cancels exactly at (0, 2) -- in both pairs, so that with all four tables that
    scored column has a = b = 0."""
    ys, lens, x = kernel_case(n, W, V, seed=n * 1000 + W)
    q = (torch.randn(n, W - 1, V, generator=torch.Generator().manual_seed(n * 1000 + W + 7)) * 4).clamp(-15, 15)
    if V > 2:
        x[0, 0, 1] = q[0, 0, 1] = -float("inf")
    if variant == "no_lens":
        lens = None
    return ys, lens, x, q, weights(n, W, seed=W) + weights(n, W, seed=W + 1)


def geometry(n, W, V, variant):
    shift = 3 if variant == "shift" else 0
    return shift, (V + 3 if variant == "ld" else V), (V + 5 if variant == "ld" else V), W - 1 + shift


def on_device(rows, live, n, R, shift, ld, V):
    """rows [n, W - 1, V] as the kernels take them: NaN in the rows that are not live, in the shift rows in front of a
    sequence and behind V; the [n * R, V] view of the [n * R, ld] buffer."""
    big = torch.full((n, R, ld), NAN)
    rows = rows.clone()
    rows[~live] = NAN
    big[:, shift:, :V] = rows
    return big.cuda().view(n * R, ld)[:, :V]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_dist_against_the_rule(ops, n, W, V, variant):
    ys, lens, x, q, _ = dist_kernel_case(n, W, V, variant)
    prior = variant != "no_prior"
    scored = scored_columns(ys, lens)
    ref = dist_reference(x.double(), ys, lens, PAD, prior_logits=q.double() if prior else None)
    shift, ld, ldq, R = geometry(n, W, V, variant)
    xd = on_device(x, scored, n, R, shift, ld, V)
    qd = on_device(q, scored, n, R, shift, ldq, V) if prior else None
    args = (xd, ys.cuda(), None if lens is None else lens.int().cuda(), PAD)
    runs = []
    for _ in range(2):
        out = (torch.full((n, W), NAN, device="cuda"), torch.full((n,), NAN, device="cuda"))
        out += (torch.full((n, W), NAN, device="cuda"), torch.full((n,), NAN, device="cuda")) if prior else (None, None)
        got = ops.seq_dist(*args, row_shift=shift, rows_per_seq=R, prior_logits2d=qd, out=out)
        assert all(g is o for g, o in zip(got, out))
        runs.append(out)
    torch.cuda.synchronize()
    tokens = scored.sum(1).double()
    worst = 0.0
    for i, name in enumerate(("token_entropy", "entropy", "token_kl", "kl")):
        if not prior and i >= 2:
            assert runs[0][i] is None
            continue
        assert torch.equal(runs[0][i], runs[1][i]), name                          # two runs: the same bits
        got = runs[0][i].cpu().double()
        assert bool(torch.isfinite(got).all()), f"{name}: not finite (never written, or a poisoned row read)"
        if got.dim() == 2:
            assert not got[:, 0].any() and not got[:, 1:][~scored].any(), name    # exact zeros
            tol = torch.full_like(got, 1e-4)
        else:
            tol = tokens * 1e-4 + 1e-12
        ratio = float(((got - ref[i]).abs() / tol).max())
        print(f"seq_dist {n, W, V} {variant} {name}: worst error / tolerance {ratio:.4f}")
        assert ratio <= 1.0, name
        worst = max(worst, ratio)
    if n > 2:
        assert float(runs[0][1][2]) == 0                                          # the all-pad row
    print(f"seq_dist {n, W, V} {variant}: worst error / tolerance {worst:.4f}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_dist_bwd_against_the_rule(ops, n, W, V, variant):
    ys, lens, x, q, gs = dist_kernel_case(n, W, V, variant)
    prior = variant != "no_prior"
    scored = scored_columns(ys, lens)
    shift, ld, ldq, R = geometry(n, W, V, variant)
    worst = 0.0
    for which in WHICH:
        g_e, g_te, g_k, g_tk = pick(gs, which) if prior else pick(gs[:2] + (None, None), which)
        if all(g is None for g in (g_e, g_te, g_k, g_tk)):
            continue                                                              # a kl table without a prior
        zero = torch.zeros(n, W - 1)
        a = zero + (0 if g_e is None else g_e[:, None]) + (0 if g_te is None else g_te[:, 1:])
        b = zero + (0 if g_k is None else g_k[:, None]) + (0 if g_tk is None else g_tk[:, 1:])
        live = scored & ((a != 0) | (b != 0))
        dbl = [None if g is None else g.double() for g in (g_e, g_te, g_k, g_tk)]
        ref = dist_grad_reference(x.double(), ys, lens, PAD, prior_logits=q.double() if prior else None,
                                  g_entropy=dbl[0], g_token_entropy=dbl[1], g_kl=dbl[2], g_token_kl=dbl[3])
        # NaN wherever the kernel has no business reading: behind V, the shift rows, and BOTH models' logits rows that
        # are not scored or whose two weights are 0; the prior's also where its own weight is 0.  dlogits starts as NaN
        xd = on_device(x, live, n, R, shift, ld, V)
        qd = on_device(q, live & (b != 0), n, R, shift, ldq, V) if prior else None
        args = (xd, ys.cuda(), None if lens is None else lens.int().cuda(), PAD)
        outs = []
        for _ in range(2):
            buf = torch.full((n * R, ld), NAN, device="cuda")
            ops.seq_dist_bwd(*args, row_shift=shift, rows_per_seq=R, prior_logits2d=qd, g_entropy=cu(g_e),
                             g_token_entropy=cu(g_te), g_kl=cu(g_k), g_token_kl=cu(g_tk), out=buf[:, :V])
            outs.append(buf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:, :V], outs[1][:, :V])                        # two runs: the same bits
        assert bool(torch.isnan(outs[0][:, V:]).all())                            # nothing written behind V
        got = outs[0][:, :V].cpu().view(n, R, V)
        assert bool(torch.isfinite(got).all()), f"{which}: dlogits not finite (never written, or a poisoned row read)"
        assert not got[:, :shift].any() and not got[:, shift:][~live].any()       # exact zeros
        gmax = max(float(a.abs().max()), float(b.abs().max()))
        worst = max(worst, kernel_ratio(got[:, shift:], ref, gmax * (BWD_ABS / 1e-6),
                                        f"seq_dist_bwd {n, W, V} {variant} {which}"))
        if which == "all" and W > 2 and lens is None:
            assert bool(scored[0, 1]) and not bool(live[0, 1])                    # the cancelling pairs were in play
        if V > 2 and bool(live[0, 0]):
            assert float(got[0, shift, 1]) == 0.0 and float(ref[0, 0, 1]) == 0.0  # the -inf logit
        if W > 3 and bool(live[0, 2]):
            assert float(got[0, shift + 2, (int(ys[0, 3]) + 1) % V]) == 0.0       # the -1e4 logit: p == 0 in fp32
    print(f"seq_dist_bwd {n, W, V} {variant}: worst error / tolerance {worst:.4f}")


@pytest.mark.parametrize("n,W,V", [(3, 8, 30), (2, 9, 1024)])
def test_kl_from_itself_is_exactly_zero(ops, n, W, V):
    """The prior's pointer IS the agent's buffer: every token_kl, kl and the kl gradient are exactly 0."""
    ys, lens, x, _, gs = dist_kernel_case(n, W, V, "plain")
    xd = x.cuda().view(n * (W - 1), V)
    args = (xd, ys.cuda(), lens.int().cuda(), PAD)
    te, en, tk, kl = ops.seq_dist(*args, prior_logits2d=xd)
    assert bool((te[:, 1:].cpu()[scored_columns(ys, lens)] > 0).all()) and not tk.any() and not kl.any()
    dl = ops.seq_dist_bwd(*args, prior_logits2d=xd, g_kl=cu(gs[2]), g_token_kl=cu(gs[3]))
    assert dl.shape == xd.shape and not dl.any()


# ------------------------------------------------------------------------------------------------------ 2. refusals
def raw_case():
    n, W, V = 2, 9, 30
    t = dict(x=torch.zeros(n * (W - 1), V), q=torch.zeros(n * (W - 1), V), ys=torch.zeros(n, W, dtype=torch.long),
             g=torch.ones(n), gt=torch.ones(n, W))
    return n, W, V, {k: v.cuda() for k, v in t.items()}


def raw_fwd(ops, outs, **over):
    n, W, V, t = raw_case()
    a = dict(logits=t["x"].data_ptr(), ld=V, V=V, rows_per_seq=W - 1, row_shift=0, prior=t["q"].data_ptr(), ld_prior=V,
             ys=t["ys"].data_ptr(), ld_ys=W, prefix_lens=None, pad_id=PAD, n=n, W=W, token_entropy=outs[0].data_ptr(),
             ld_out=W, entropy=outs[1].data_ptr(), token_kl=outs[2].data_ptr(), kl=outs[3].data_ptr())
    a.update(over)
    rc = ops._L().gct_seq_dist(*a.values(), ops._st())
    torch.cuda.synchronize()
    return rc


def raw_bwd(ops, out, **over):
    n, W, V, t = raw_case()
    a = dict(logits=t["x"].data_ptr(), ld=V, V=V, rows_per_seq=W - 1, row_shift=0, prior=t["q"].data_ptr(), ld_prior=V,
             ys=t["ys"].data_ptr(), ld_ys=W, prefix_lens=None, pad_id=PAD, n=n, W=W, g_entropy=t["g"].data_ptr(),
             g_token_entropy=t["gt"].data_ptr(), ld_ge=W, g_kl=t["g"].data_ptr(), g_token_kl=t["gt"].data_ptr(), ld_gk=W,
             dlogits=out.data_ptr(), ld_d=V)
    a.update(over)
    rc = ops._L().gct_seq_dist_bwd(*a.values(), ops._st())
    torch.cuda.synchronize()
    return rc


FWD_REFUSALS = [dict(logits=None), dict(ys=None), dict(token_entropy=None), dict(entropy=None), dict(ld=29),
                dict(ld_prior=29), dict(W=257, rows_per_seq=256, ld_ys=257, ld_out=257), dict(W=0), dict(ld_ys=8),
                dict(ld_out=8), dict(rows_per_seq=7), dict(row_shift=1), dict(row_shift=-1), dict(V=0),
                dict(prior=None),                                                 # kl outputs without a prior
                dict(token_kl=None), dict(kl=None)]                               # a prior without them
BWD_REFUSALS = [dict(logits=None), dict(ys=None), dict(dlogits=None), dict(ld=29), dict(ld_prior=29), dict(ld_d=29),
                dict(W=257, rows_per_seq=256, ld_ys=257, ld_ge=257, ld_gk=257), dict(W=0), dict(ld_ys=8),
                dict(ld_ge=8), dict(ld_gk=8), dict(rows_per_seq=7), dict(row_shift=1), dict(V=0),
                dict(prior=None),                                                 # kl weights without a prior
                dict(prior=None, g_kl=None),                                      # (one of them is enough)
                dict(g_entropy=None, g_token_entropy=None, g_kl=None, g_token_kl=None)]


def test_seq_dist_refuses_before_a_launch(ops):
    n, W, V, _ = raw_case()
    outs = [torch.full(s, SENT, device="cuda") for s in ((n, W), (n,), (n, W), (n,))]
    assert raw_fwd(ops, outs) == 0                                                # the case itself is fine
    assert not any(bool((o == SENT).any()) for o in outs)
    for over in FWD_REFUSALS:
        outs = [torch.full(s, SENT, device="cuda") for s in ((n, W), (n,), (n, W), (n,))]
        with pytest.raises(GctError, match="seq_dist"):
            check(raw_fwd(ops, outs, **over), "gct_seq_dist")
        assert all(bool((o == SENT).all()) for o in outs), over
    assert raw_fwd(ops, outs, n=0) == 0                                           # no sequence: nothing is written
    assert all(bool((o == SENT).all()) for o in outs)
    # the binding: the same refusals reach the caller, and no sequences means no call at all
    x, ys = torch.zeros(16, 30, device="cuda"), torch.zeros(2, 9, dtype=torch.long, device="cuda")
    with pytest.raises(GctError, match="null"):
        ops.seq_dist(None, ys, None, PAD, V=30)
    with pytest.raises(GctError, match="without prior"):
        ops.seq_dist(x, ys, None, PAD, out=tuple(outs))
    with pytest.raises(GctError, match="257"):
        ops.seq_dist(torch.zeros(256, 30, device="cuda"), torch.zeros(1, 257, dtype=torch.long, device="cuda"), None,
                     PAD)
    assert ops.seq_dist(x, ys[:0], None, PAD)[0].shape == (0, 9)


def test_seq_dist_bwd_refuses_before_a_launch(ops):
    n, W, V, _ = raw_case()
    out = torch.full((n * (W - 1), V), SENT, device="cuda")
    assert raw_bwd(ops, out) == 0 and not bool((out == SENT).any())               # the case itself is fine
    for over in BWD_REFUSALS:
        out = torch.full((n * (W - 1), V), SENT, device="cuda")
        with pytest.raises(GctError, match="seq_dist_bwd"):
            check(raw_bwd(ops, out, **over), "gct_seq_dist_bwd")
        assert bool((out == SENT).all()), over
    assert raw_bwd(ops, out, n=0) == 0 and bool((out == SENT).all())              # no sequence: nothing is written
    x, ys = torch.zeros(16, 30, device="cuda"), torch.zeros(2, 9, dtype=torch.long, device="cuda")
    one = torch.ones(2, device="cuda")
    with pytest.raises(GctError, match="all four"):
        ops.seq_dist_bwd(x, ys, None, PAD)
    with pytest.raises(GctError, match="without prior"):
        ops.seq_dist_bwd(x, ys, None, PAD, g_kl=one)
    with pytest.raises(GctError, match="do not hold"):
        ops.seq_dist_bwd(x, ys, None, PAD, rows_per_seq=7, g_entropy=one)
    assert ops.seq_dist_bwd(x, ys[:0], None, PAD, g_entropy=one[:0]).shape == (16, 30)   # the binding: no call at all
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------- 3. SeqDistFn
class _NoGradient(torch.autograd.Function):
    """Identity whose backward hands None on: what a consumer that needs no gradient looks like to SeqDistFn."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("use", ["entropy", "kl", "token", "nothing"])
def test_seq_dist_fn_under_autograd(use):
    from gct_plus_amd import engine
    n, W, V = 5, 11, 31
    ys, lens, x, q, gs = dist_kernel_case(n, W, V, "plain")
    xd, qd = x.cuda().requires_grad_(), q.cuda().requires_grad_()
    entropy, token_entropy, kl, token_kl = engine.SeqDistFn.apply(xd, qd, ys.cuda(), lens.int().cuda(), PAD, 0)
    assert all(t.requires_grad for t in (entropy, token_entropy, kl, token_kl))
    ref = dist_reference(x.double(), ys, lens, PAD, prior_logits=q.double())
    for got, want in zip((token_entropy, entropy, token_kl, kl), ref):
        assert got.shape == want.shape and float((got.detach().cpu().double() - want).abs().max()) <= W * 1e-4
    tables = dict(entropy=(gs[0], None, None, None), kl=(None, None, gs[2], None), token=(None, gs[1], None, None),
                  nothing=(None,) * 4)[use]
    if use == "nothing":
        _NoGradient.apply(entropy).sum().backward()                               # every incoming gradient is None
        assert xd.grad.shape == xd.shape and not xd.grad.any() and qd.grad is None
        return
    obj = sum((g.cuda() * out).sum() for g, out in zip(tables, (entropy, token_entropy, kl, token_kl)) if g is not None)
    obj.backward()
    assert xd.grad.shape == xd.shape and qd.grad is None                          # the prior gets no gradient
    dbl = [None if g is None else g.double() for g in tables]
    want = dist_grad_reference(x.double(), ys, lens, PAD, prior_logits=q.double(), g_entropy=dbl[0],
                               g_token_entropy=dbl[1], g_kl=dbl[2], g_token_kl=dbl[3])
    gmax = max(float(g.abs().max()) for g in tables if g is not None)
    kernel_ratio(xd.grad, want, gmax * (BWD_ABS / 1e-6), f"SeqDistFn {use}")
    # without a prior: no kl outputs
    e2, te2, none_kl, none_tkl = engine.SeqDistFn.apply(xd, None, ys.cuda(), lens.int().cuda(), PAD, 0)
    assert none_kl is None and none_tkl is None and torch.equal(e2, entropy) and torch.equal(te2, token_entropy)


# ----------------------------------------------------------------------------------------------- 4. sequence_policy
def perturb_out_bias(model, seed=11):
    """Move the agent away from its frozen copy: an in-place write of out.bias (model.weights_token follows it)."""
    with torch.no_grad():
        b = model.out.bias
        b.add_((torch.randn(b.shape, generator=torch.Generator().manual_seed(seed)) * 0.5).to(b.device))


def oracle_logits(state, mtype, c2d, extra, t, z=None):
    """The CPU oracle's teacher-forced logits [n, W - 1, V] of the rows t under a state dict (leaves or tensors)."""
    from oracle import gct_oracle as O
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, **dict(dict(use_cond2lat=True), **extra), **TINY)
    trg = t["ys"][:, :-1]
    return O.decode(state, cfg, trg, t["z"] if z is None else z, t["src_mask"],
                    O.get_trg_mask(trg, PAD, c2d, t["dconds"] if nc else None), t["dconds"])[:, nc if c2d else 0:]


def pushed_through(x, q, scored):
    """The logits tolerance pushed through each term, per scored column [n, W - 1], from fp64 logits x (agent) and q
    (prior): 1e-4 + sum_v |dH/dx_v| (1e-4 + 1e-4 |x_v|) for the entropy; for the KL the same with dKL/dx_v, plus the sum
    over the prior's logits with dKL/dy_v = q_v - p_v."""
    lp, lq = torch.log_softmax(x, -1), torch.log_softmax(q, -1)
    p, pq = lp.exp(), lq.exp()
    H = -(p * lp).sum(-1, keepdim=True)
    KL = (p * (lp - lq)).sum(-1, keepdim=True)
    ex, eq = 1e-4 + 1e-4 * x.abs(), 1e-4 + 1e-4 * q.abs()
    tol_h = 1e-4 + ((p * (lp + H)).abs() * ex).sum(-1)
    tol_k = 1e-4 + ((p * ((lp - lq) - KL)).abs() * ex).sum(-1) + ((pq - p).abs() * eq).sum(-1)
    return torch.where(scored, tol_h, torch.ones(())), torch.where(scored, tol_k, torch.ones(()))


@pytest.mark.parametrize("mtype,c2d", [("vaetf", False), ("pscavaetf", False), ("pvaetf", True)])
def test_sequence_policy_values_and_gradients_vs_oracle(ops, mtype, c2d):
    from oracle import gct_oracle as O
    from gct_plus_amd.Train.finetune import frozen_prior
    extra = dict(use_cond2dec=True, use_cond2lat=False) if c2d else {}
    model = build(mtype, seed=31, **extra)                                        # eval mode
    t = target_rows(mtype, 7)
    args = (cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda())
    kw = dict(prefix_lens=t["lens"], pad_id=PAD)
    prior = frozen_prior(model)
    z = t["z"].cuda().requires_grad_()
    # the prior is the model: KL exactly 0, its log-likelihood the model's; logp & co. are sequence_logp's bits
    same = sequence_policy(model, z, *args, prior=prior, **kw)
    want = sequence_logp(model, z, *args, **kw)
    for name, w in zip(("logp", "tokens", "hits", "token_logp"), want):
        assert torch.equal(getattr(same, name).detach(), w.detach()), name
    assert not same.kl.any() and not same.token_kl.any() and torch.equal(same.prior_logp, same.logp.detach())
    assert same.kl.requires_grad and same.entropy.requires_grad and not same.prior_logp.requires_grad
    assert bool((same.entropy > 0).all())
    # the agent moves away
    perturb_out_bias(model)
    terms = sequence_policy(model, z, *args, prior=prior, **kw)
    want = sequence_logp(model, z, *args, **kw)
    for name, w in zip(("logp", "tokens", "hits", "token_logp"), want):
        assert torch.equal(getattr(terms, name).detach(), w.detach()), name
    assert torch.equal(terms.prior_logp, same.prior_logp)                         # the prior did not move
    alone = sequence_policy(model, z, *args, **kw)                                # without a prior
    assert alone.kl is None and alone.token_kl is None and alone.prior_logp is None
    assert torch.equal(alone.token_entropy, terms.token_entropy) and torch.equal(alone.entropy, terms.entropy)
    bare = sequence_policy(model, z, *args, entropy=False, **kw)
    assert bare.entropy is None and bare.token_entropy is None and torch.equal(bare.logp, terms.logp)
    # values against the oracle
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    Q = {k: v.detach().cpu() for k, v in prior.state_dict().items()}
    zo = t["z"].clone().requires_grad_()
    x = oracle_logits(P, mtype, c2d, extra, t, z=zo)
    with torch.no_grad():
        q = oracle_logits(Q, mtype, c2d, extra, t)
    scored = scored_columns(t["ys"], t["lens"])
    ref = dist_reference(x.detach().double(), t["ys"], t["lens"], PAD, prior_logits=q.double())
    tol_h, tol_k = pushed_through(x.detach().double(), q.double(), scored)
    for name, got, want_tab, tol in (("token_entropy", terms.token_entropy, ref[0], tol_h),
                                     ("token_kl", terms.token_kl, ref[2], tol_k)):
        got = got.detach().cpu().double()
        assert not got[:, 0].any() and not got[:, 1:][~scored].any(), name
        ratio = ((got - want_tab)[:, 1:].abs() / tol)
        print(f"{mtype} c2d={c2d} {name} vs oracle: worst error / tolerance {float(ratio.max()):.4f}")
        assert bool((ratio <= 1).all()), name
    assert float(ref[3].min()) > 1e-3                                             # the KL is not a rounding residue
    # gradients of entropy.sum() - 0.5 kl.sum() against the oracle's autograd through dist_reference
    model.zero_grad(set_to_none=True)
    (terms.entropy.sum() - 0.5 * terms.kl.sum()).backward()
    ops.assert_no_skipped_row_gradients()
    _, en, _, kl = dist_reference(x, t["ys"], t["lens"], PAD, prior_logits=q)
    (en.sum() - 0.5 * kl.sum()).backward()
    floor = grad_floor([v.grad for v in P.values()] + [zo.grad])
    seen = 0
    for name, p in model.named_parameters():
        e = P[name].grad
        if not name.startswith(("decoder.", "out.")):
            assert e is None or not e.any(), name
            assert p.grad is None or not p.grad.any(), f"{name}: the encoder side got a gradient"
            continue
        if e is None:
            assert p.grad is None or not p.grad.any(), name
            continue
        assert p.grad is not None, name
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad {name}")
        seen += 1
    assert seen > 20
    assert_close(z.grad, zo.grad, 1e-5 * float(zo.grad.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad z")
    assert all(p.grad is None for p in prior.parameters())


def test_sequence_policy_does_not_depend_on_the_row_plan(ops, monkeypatch):
    """tests/test_seq_logp_grad_gpu.py's row-plan test with the distribution terms: 24 rows, the planner takes the live
    rows; values and gradients are the same with every live-row shortcut switched off."""
    from gct_plus_amd import engine
    from gct_plus_amd.Train.finetune import frozen_prior
    model = build("pscavaetf", seed=32)
    prior = frozen_prior(model)
    perturb_out_bias(model)
    t = target_rows("pscavaetf", 8, lengths=(5, 20, 8, 12, 6, 16) + (6, 7, 9, 5, 8, 10) * 3)
    took = []
    finish = engine.RowPlan.finish

    def spy(self):
        plan = finish(self)
        took.append(plan.live is not None)
        return plan
    monkeypatch.setattr(engine.RowPlan, "finish", spy)
    grads, values, sums = {}, {}, {}
    for mode in (True, False):
        for name in ("COMPACT_FWD", "COMPACT_BWD", "COMPACT_KV", "COMPACT_ENC_KV"):
            monkeypatch.setattr(engine, name, mode)
        took.clear()
        z = t["z"].cuda().requires_grad_()
        model.zero_grad(set_to_none=True)
        terms = sequence_policy(model, z, cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda(), prefix_lens=t["lens"],
                                pad_id=PAD, prior=prior)
        (terms.entropy.sum() - 0.5 * terms.kl.sum() + 0.1 * terms.logp.sum()).backward()
        ops.assert_no_skipped_row_gradients()
        assert any(took) == mode and len(took) >= 2                               # the agent's forward and the prior's
        grads[mode] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        grads[mode]["__z__"] = z.grad.clone()
        values[mode] = dict(token_entropy=terms.token_entropy.detach(), token_kl=terms.token_kl.detach(),
                            token_logp=terms.token_logp.detach())
        sums[mode] = (terms.entropy.detach(), terms.kl.detach(), terms.prior_logp, terms.tokens)
    floor = grad_floor(list(grads[False].values()))
    for n, e in grads[False].items():
        assert_close(grads[True][n], e, 2e-6 * float(e.abs().max()) + floor, 2e-5, f"live rows vs every row: {n}")
    for n, e in values[False].items():                                            # test_score_gpu.py's tolerance there
        close_tokens(values[True][n], e, f"live rows vs every row: {n}")
    assert torch.equal(sums[True][3], sums[False][3]) and int(sums[True][3].min()) >= 1
    assert float((sums[True][1] - sums[False][1]).abs().max()) <= 2e-4 * int(sums[True][3].max())


def test_sequence_policy_refuses_before_device_work():
    from gct_plus_amd.Train.finetune import frozen_prior
    model = build("vaetf", seed=33)
    z, m = torch.randn(2, 8, TINY["latent_dim"]).cuda(), torch.ones(2, 1, 8, dtype=torch.bool).cuda()
    ys = torch.full((2, 9), 5)
    with pytest.raises(ValueError, match="no column"):
        sequence_policy(model, z, m, None, torch.full((2, 9), PAD), pad_id=PAD)
    with pytest.raises(ValueError, match="positional table"):
        sequence_policy(model, z, m, None, torch.full((2, 202), 5), pad_id=PAD)
    with pytest.raises(ValueError, match="nconds"):
        sequence_policy(model, z, m, None, ys, pad_id=PAD, prior=build("pvaetf", seed=33))
    with pytest.raises(ValueError, match="vocabulary"):
        sequence_policy(model, z, m, None, ys, pad_id=PAD, prior=build("scavaetf", seed=33))
    with pytest.raises(ValueError, match="use_cond2dec"):
        sequence_policy(build("pvaetf", seed=33), z, m, torch.zeros(2, 3).cuda(), ys, pad_id=PAD,
                        prior=build("pvaetf", seed=33, use_cond2dec=True, use_cond2lat=False))
    prior = frozen_prior(model)
    assert not prior.training and all(not p.requires_grad for p in prior.parameters())
    mine = {p.data_ptr() for p in model.parameters()} | {model.flat_params().data_ptr()}
    assert prior.flat_params().data_ptr() not in mine and all(p.data_ptr() not in mine for p in prior.parameters())
    lo, hi = prior.flat_params().data_ptr(), prior.flat_params().data_ptr() + 4 * prior.flat_params().numel()
    assert all(lo <= p.data_ptr() < hi for p in prior.parameters())               # the copy lives in ITS flat buffer
    sd, sp_ = model.state_dict(), prior.state_dict()
    assert list(sd) == list(sp_) and all(torch.equal(sd[k], sp_[k]) for k in sd)


# --------------------------------------------------------------------------------------------------- 5. update steps
@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_regularised_steps_follow_the_oracle(ops, mtype):
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import frozen_prior, reinforce_step
    sp, t, reward = policy_sampler(mtype)
    model = sp.model
    prior = frozen_prior(model)
    prior_state = {k: v.detach().clone() for k, v in prior.state_dict().items()}
    rows = DecodedRows(t["z"], t["ys"], t["src_mask"], t["dconds"], t["lens"])
    frozen = {k: p.detach().clone() for k, p in model.named_parameters() if not k.startswith(("decoder.", "out."))}
    start = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt = FusedAdam(model.parameters(), lr=UPDATE_LR, betas=(0.9, 0.98), eps=1e-9, model=model)
    got, first = dict(loss=[], mean_entropy=[], mean_kl=[]), None
    for _ in range(UPDATE_STEPS):
        stats = reinforce_step(sp, opt, rows, reward, entropy_coef=ENTROPY_COEF, kl_coef=KL_COEF, prior=prior)
        assert not model.training and not prior.training
        assert set(stats) == {"loss", "mean_reward", "mean_logp", "tokens", "mean_entropy", "mean_kl", "mean_prior_logp"}
        for k in got:
            got[k].append(stats[k])
        first = first or stats
    ops.assert_no_skipped_row_gradients()
    want = oracle_regularised_run(mtype)
    for k in got:
        print(f"{mtype} {k}: device {[round(v, 7) for v in got[k]]}\n{' ' * (len(mtype) + len(k))}  oracle "
              f"{[round(v, 7) for v in want[k]]}")
        extra = 1e-6 if k == "mean_kl" else 0.0
        assert all(abs(a - b) <= 1e-3 * abs(b) + extra for a, b in zip(got[k], want[k])), (k, got[k], want[k])
    assert got["mean_kl"][0] == 0.0 and all(v > 0 for v in got["mean_kl"][1:])
    assert first["mean_prior_logp"] == first["mean_logp"] == stats["mean_prior_logp"]   # the prior is the initial model
    for k, v in prior.state_dict().items():
        assert torch.equal(v, prior_state[k]), f"{k}: the prior moved"
    for k, p in model.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach(), frozen[k]), f"{k}: the encoder side moved"
    assert any(not torch.equal(p.detach(), start[k]) for k, p in model.named_parameters() if k.startswith("decoder."))


def test_reinforce_step_with_its_defaults_is_the_step_made_by_hand():
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import reinforce_loss, reinforce_step
    losses = []
    for by_hand in (False, True):
        sp, t, reward = policy_sampler("vaetf")
        model = sp.model
        rows = DecodedRows(t["z"], t["ys"], t["src_mask"], t["dconds"], t["lens"])
        opt = FusedAdam(model.parameters(), lr=UPDATE_LR, betas=(0.9, 0.98), eps=1e-9, model=model)
        run = []
        for _ in range(UPDATE_STEPS):
            if by_hand:
                model.train()
                scores = sp.logp(*rows)
                opt.zero_grad(set_to_none=True)
                loss = reinforce_loss(scores.logp, reward)
                loss.backward()
                opt.step()
                model.eval()
                run.append(float(loss.detach()))
            else:
                stats = reinforce_step(sp, opt, rows, reward)
                assert set(stats) == {"loss", "mean_reward", "mean_logp", "tokens"}
                run.append(stats["loss"])
        losses.append(run)
    assert losses[0] == losses[1], losses                                         # bit-equal floats: the old path
    assert len(set(losses[0])) == UPDATE_STEPS


# ------------------------------------------------------------------------------------------------------ 6. front end
@pytest.mark.parametrize("cls,mtype", [("VaetfSampling", "vaetf"), ("PscavaetfSampling", "pscavaetf")])
def test_policy_terms_of_decoded_rows(cls, mtype):
    from gct_plus_amd.decode import PolicyTerms
    from gct_plus_amd.Train.finetune import frozen_prior
    n = 6
    g = torch.Generator().manual_seed(6)
    z = torch.randn(n, 30, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    sp = make_sampler(cls, mtype, "multinomial", None, with_logp=True)
    if mtype == "vaetf":
        out = sp.sample_smiles(n, zs=z, return_rows=True)
    else:
        out = sp.sample_smiles(dconds, "c1ccccc1", zs=z, transform=False, return_rows=True)
    logp, rows = out[3], out[4]
    prior = frozen_prior(sp.model)
    terms = sp.policy_terms(*rows, prior=prior)
    L = rows.ys.shape[1]
    assert isinstance(terms, PolicyTerms) and all(t.is_cuda for t in terms)
    assert terms.logp.shape == terms.entropy.shape == terms.kl.shape == terms.prior_logp.shape == (n,)
    assert terms.token_logp.shape == terms.token_entropy.shape == terms.token_kl.shape == (n, L)
    assert bool((terms.tokens >= 1).all()) and bool((terms.entropy > 0).all())
    assert terms.logp.requires_grad and terms.entropy.requires_grad and terms.kl.requires_grad
    assert not terms.prior_logp.requires_grad
    close_sums(logp, terms.token_logp, f"{cls}: policy_terms(*rows) vs the decode's own log-probabilities")
    assert not terms.kl.any() and torch.equal(terms.prior_logp, terms.logp.detach())   # the prior is the model
    perturb_out_bias(sp.model)
    moved = sp.policy_terms(*rows, prior=prior)
    assert bool((moved.kl > 0).all()) and torch.equal(moved.prior_logp, terms.prior_logp)
    assert sp.policy_terms(*rows).kl is None
