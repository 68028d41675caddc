"""PPO's clipped surrogate on the device: gct_seq_ppo / gct_seq_ppo_bwd against the rules (decode.ppo_reference /
ppo_grad_reference) in fp64 on the same fp32 inputs, and bit for bit against gct_seq_logp / gct_seq_logp_bwd;
engine.SeqPpoFn under autograd; decode.sequence_ppo against sequence_logp / sequence_policy (bits) and the CPU oracle with
the rule under torch autograd (gradients); Train/finetune.ppo_update against reinforce_step (bits), against the same
epochs on the oracle, with target_kl and minibatches; and Sampling.ppo_terms.

Inputs.  tests/test_ppo_host.ppo_inputs: old = lp_fp64 + delta, delta from {0, +-0.05, +-0.5}, so every ratio stays at
least 0.148 away from the boundaries of clip 0.2 and the fp32 kernel takes the clip decisions of the fp64 rule.

Tolerances.
Forward kernel: token_logp, logp, tokens and hits are gct_seq_logp's bits.  tests/test_score_gpu.py's kernel tolerance of
a log-probability is 1e-4 per token; pushed through the surrogate (d (A rho) / d lp = A rho) that is 1e-4 |A| rho per
token, and through the k3 term (d / d lp = rho - 1) 1e-4 |rho - 1|, plus what fp32 adds behind lp: expf (2 ulp of rho)
and two subtractions, 2^-21 (1 + rho); a sequence sum gets the sum of its tokens' tolerances plus 2^-23 sum |term| per
addition.
Backward kernel: kernel_ratio of tests/test_seq_logp_grad_gpu.py (1e-6 max|w| + 1e-5 |ref|, w = g A rho the weight of the
live rows), imported and unchanged.  The weight carries rho = exp(lp - old) with an fp32 lp, so the fp32 RULE
(ppo_grad_reference on the fp32 inputs, CPU) was measured against the fp64 rule on exactly these cases (SHAPES x
VARIANTS x WHICH) before the kernel ran: its worst ratio under kernel_ratio's tolerance is 0.163 -- (300, 60, 30) plain
surrogate --, so the tolerance is not too tight for fp32 and stays as it is.
Model gradients: tests/test_model_gpu.py's (rtol 1e-3 + 1e-5 max|g| per tensor + grad_floor).  Per epoch: the loss-curve
tolerance, 1e-3 relative."""
import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd._lib import GctError, check
from gct_plus_amd.decode import (PpoTerms, ppo_grad_reference, ppo_reference, score_reference, sequence_logp,
                                 sequence_policy, sequence_ppo)
from tests.test_mixed_scaffold_decode_gpu import PAD, TINY, build
from tests.test_model_gpu import assert_close, grad_floor
from tests.test_policy_terms_gpu import oracle_logits, perturb_out_bias
from tests.test_policy_terms_host import scored_columns
from tests.test_ppo_host import (CLIP, DELTAS, NEAR_CAP, PPO_EPOCHS, PPO_LR, PPO_MTYPE, near_a_boundary,
                                 oracle_ppo_run, ppo_inputs, ppo_update_case)
from tests.test_score_gpu import cu, kernel_case, target_rows
from tests.test_seq_logp_grad_gpu import greedy_matches_uncached, kernel_ratio
from tests.test_seq_logp_grad_host import update_vocabs
from tests.test_stream_decode_gpu import make_sampler

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 7.25


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


# ------------------------------------------------------------------------------- 1. gct_seq_ppo / gct_seq_ppo_bwd
SHAPES = [(1, 2, 2), (3, 4, 65), (2, 256, 5), (2, 9, 1024), (67, 5, 30), (300, 60, 30)]   # the last: 17 700 rows, past
VARIANTS = ["plain", "no_lens", "ld", "shift"]                                           # the 4096 x 4 of one grid
WHICH = ["surrogate", "token", "both"]


def ppo_kernel_case(n, W, V, variant):
    """kernel_case's rows and logits (ties, a -1e4 logit) with ppo_inputs' tables rounded to fp32: (ys, lens, x, old
    [n, W], adv [n], g_surrogate [n], g_token_surrogate [n, W])."""
    ys, lens, x = kernel_case(n, W, V, seed=n * 1000 + W)
    if variant == "no_lens":
        lens = None
    old, adv, g_s, g_ts = ppo_inputs(ys, lens, x, seed=W)
    return ys, lens, x, old.float(), adv.float(), g_s.float(), g_ts.float()


def geometry(n, W, V, variant):
    """(row_shift, ld of the logits and dlogits, ld of old, ld of the gradient table, ld of the token outputs, R)."""
    strided = variant == "ld"
    return (3 if variant == "shift" else 0, V + 3 if strided else V, W + 2 if strided else W, W + 5 if strided else W,
            W + 1 if strided else W, W - 1 + (3 if variant == "shift" else 0))


def strided(t, ld, fill=NAN):
    """t [n, W] as the [n, W] view of a [n, ld] device buffer filled with `fill`."""
    buf = torch.full((t.shape[0], ld), fill, device="cuda")
    buf[:, :t.shape[1]] = t.cuda()
    return buf[:, :t.shape[1]]


def logits_on_device(x, live, n, R, shift, ld, V):
    """x [n, W - 1, V] as the kernels take it: NaN in the rows that are not live, in the shift rows in front of a
    sequence and behind V; the [n * R, V] view of the [n * R, ld] buffer."""
    big = torch.full((n, R, ld), NAN)
    rows = x.clone()
    rows[~live] = NAN
    big[:, shift:, :V] = rows
    return big.cuda().view(n * R, ld)[:, :V]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_ppo_against_the_rule(ops, n, W, V, variant):
    ys, lens, x, old, adv, _, _ = ppo_kernel_case(n, W, V, variant)
    scored = scored_columns(ys, lens)
    ref = ppo_reference(x.double(), ys, lens, PAD, old.double(), adv.double(), CLIP, CLIP)
    shift, ld, ld_old, _, ld_out, R = geometry(n, W, V, variant)
    xd = logits_on_device(x, scored, n, R, shift, ld, V)
    oldp = old.clone()
    oldp[:, 1:][~scored] = NAN                                                    # old is not read where nothing is scored
    oldp[:, 0] = NAN
    args = (xd, ys.cuda(), strided(oldp, ld_old), adv.cuda(), CLIP, CLIP, None if lens is None else lens.int().cuda(), PAD)
    runs = []
    for _ in range(2):
        out = (strided(torch.full((n, W), NAN), ld_out), strided(torch.full((n, W), NAN), ld_out)) + tuple(
            torch.full((n,), NAN, device="cuda") for _ in range(3)) + tuple(
            torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        got = ops.seq_ppo(*args, row_shift=shift, rows_per_seq=R, out=out)
        assert all(g is o for g, o in zip(got, out))
        runs.append(out)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                                  # two runs: the same bits
    tl, ts, lp, su, kl, nt, nh, nc = (t.cpu() for t in runs[0])
    assert torch.equal(nt, ref[5]) and torch.equal(nh, ref[6]) and torch.equal(nc, ref[7])   # counts: exactly
    want = ops.seq_logp(xd, ys.cuda(), None if lens is None else lens.int().cuda(), PAD, row_shift=shift, rows_per_seq=R)
    assert torch.equal(tl, want[0].cpu()) and torch.equal(lp, want[1].cpu())       # gct_seq_logp's bits
    assert torch.equal(nt, want[2].cpu()) and torch.equal(nh, want[3].cpu())
    for t in (tl, ts, lp, su, kl):
        assert bool(torch.isfinite(t).all()), "not finite: never written, or a poisoned row / old entry read"
    assert not ts[:, 0].any() and not ts[:, 1:][~scored].any()                    # exact zeros
    # tolerances of the module docstring, from the fp64 rule's own rho
    rho = torch.where(scored, torch.exp(ref[0] - old.double())[:, 1:], torch.ones((), dtype=torch.float64))
    A = adv.double().abs().view(-1, 1)
    behind = 2.0 ** -21 * (1 + rho)
    tol_s = torch.where(scored, 1e-4 * A * rho + A * behind, torch.zeros((), dtype=torch.float64))
    tol_k = torch.where(scored, 1e-4 * (rho - 1).abs() + behind, torch.zeros((), dtype=torch.float64))
    k3 = torch.where(scored, (rho - 1) - (ref[0] - old.double())[:, 1:], torch.zeros((), dtype=torch.float64))
    worst = 0.0
    for name, got, want_t, tol in (("token_surrogate", ts[:, 1:], ref[1][:, 1:], tol_s + 1e-30),
                                   ("surrogate", su, ref[3], tol_s.sum(1) + 2.0 ** -23 * W * ref[1].abs().sum(1) + 1e-30),
                                   ("approx_kl", kl, ref[4], tol_k.sum(1) + 2.0 ** -23 * W * k3.abs().sum(1) + 1e-30)):
        err = (got.double() - want_t).abs()
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())
        print(f"seq_ppo {n, W, V} {variant} {name}: worst error / tolerance {ratio:.4f}")
        assert ratio <= 1.0, name
        worst = max(worst, ratio)
    if n > 1:
        assert not ts[1].any() and float(su[1]) == 0.0 and int(nc[1]) == 0        # A == 0, whatever the row scores
    if n > 2:
        assert float(su[2]) == 0 and float(kl[2]) == 0 and int(nt[2]) == 0 and int(nc[2]) == 0  # the all-pad row
    if n >= 67:
        hi_side = scored & (adv.view(-1, 1) > 0) & (rho > 1 + CLIP)
        lo_side = scored & (adv.view(-1, 1) < 0) & (rho < 1 - CLIP)
        assert bool(hi_side.any()) and bool(lo_side.any())                        # both sides were clipped
    print(f"seq_ppo {n, W, V} {variant}: worst error / tolerance {worst:.4f}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_ppo_bwd_against_the_rule(ops, n, W, V, variant):
    ys, lens, x, old, adv, g_s, g_ts = ppo_kernel_case(n, W, V, variant)
    scored = scored_columns(ys, lens)
    shift, ld, ld_old, ld_g, _, R = geometry(n, W, V, variant)
    rho = torch.exp(score_reference(x.double(), ys, lens, PAD)[0] - old.double())[:, 1:]
    worst = 0.0
    for which in WHICH:
        gs, gt = (g_s if which != "token" else None), (g_ts if which != "surrogate" else None)
        g = (0 if gs is None else gs[:, None]) + (0 if gt is None else gt[:, 1:]) + torch.zeros(n, W - 1)
        looked = scored & (g != 0) & (adv.view(-1, 1) != 0)
        ref = ppo_grad_reference(x.double(), ys, lens, PAD, old.double(), adv.double(), CLIP, CLIP,
                                 g_surrogate=None if gs is None else gs.double(),
                                 g_token_surrogate=None if gt is None else gt.double())
        # NaN wherever the kernel has no business reading: behind V, the shift rows, the logits rows (and old entries)
        # that are not scored or whose advantage or weight is 0; dlogits starts as NaN everywhere
        xd = logits_on_device(x, looked, n, R, shift, ld, V)
        oldp = old.clone()
        oldp[:, 1:][~looked] = NAN
        oldp[:, 0] = NAN
        args = (xd, ys.cuda(), strided(oldp, ld_old), adv.cuda(), CLIP, CLIP, None if lens is None else lens.int().cuda(),
                PAD)
        outs = []
        for _ in range(2):
            buf = torch.full((n * R, ld), NAN, device="cuda")
            ops.seq_ppo_bwd(*args, row_shift=shift, rows_per_seq=R, g_surrogate=cu(gs),
                            g_token_surrogate=None if gt is None else strided(gt, ld_g), out=buf[:, :V])
            outs.append(buf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:, :V], outs[1][:, :V])                        # two runs: the same bits
        assert bool(torch.isnan(outs[0][:, V:]).all())                            # nothing written behind V
        got = outs[0][:, :V].cpu().view(n, R, V)
        assert bool(torch.isfinite(got).all()), f"{which}: dlogits not finite (a row never written, or a poisoned one read)"
        A = adv.view(-1, 1)
        clipped = looked & (((A > 0) & (rho > 1 + CLIP)) | ((A < 0) & (rho < 1 - CLIP)))
        live = looked & ~clipped
        assert not got[:, :shift].any() and not got[:, shift:][~live].any()       # exact zeros, the clipped rows too
        assert not ref[~live].any()
        w = (g.double() * adv.double().view(-1, 1) * rho)[live]
        gmax = float(w.abs().max()) if w.numel() else 0.0
        worst = max(worst, kernel_ratio(got[:, shift:], ref, gmax, f"seq_ppo_bwd {n, W, V} {variant} {which}"))
        if which == "both" and bool(scored[0].any()):
            c = int(scored[0].nonzero()[0])
            assert not bool(looked[0, c])                                         # the cancelling weights were in play
    print(f"seq_ppo_bwd {n, W, V} {variant}: worst error / tolerance {worst:.4f}")


# ------------------------------------------------------------------------------------------- 2. the bit identities
@pytest.mark.parametrize("clip", [0.0, 0.2])
@pytest.mark.parametrize("n,W,V", [(7, 9, 30), (3, 5, 130), (300, 60, 30)])
def test_a_ratio_of_one_is_seq_logp_bwd_bit_for_bit(ops, n, W, V, clip):
    """old = gct_seq_ppo's own token_logp bits: every ratio is exactly 1, nothing is clipped (also at clip 0), the
    surrogate is A per token, approx_kl exactly 0, and the backward with g_surrogate = g is gct_seq_logp_bwd's with
    g_logp = g * A, the fp32 product formed on the host."""
    ys, lens, x = kernel_case(n, W, V, seed=V)
    gen = torch.Generator().manual_seed(n)
    adv, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    adv[n // 2] = 0
    xd = x.cuda().view(n * (W - 1), V)
    args = (xd, ys.cuda(), lens.int().cuda(), PAD)
    want = ops.seq_logp(*args)
    zero = torch.zeros(n, W, device="cuda")
    tl, ts, lp, su, kl, nt, nh, nc = ops.seq_ppo(xd, ys.cuda(), want[0], adv.cuda(), clip, clip, lens.int().cuda(), PAD)
    assert torch.equal(tl, want[0]) and torch.equal(lp, want[1]) and torch.equal(nt, want[2]) and torch.equal(nh, want[3])
    assert not nc.any() and not kl.any() and int(nt.sum()) > 0
    scored = scored_columns(ys, lens)
    assert torch.equal(ts.cpu()[:, 1:], torch.where(scored, adv.view(-1, 1), torch.zeros(())))
    got = ops.seq_ppo_bwd(xd, ys.cuda(), want[0], adv.cuda(), clip, clip, lens.int().cuda(), PAD, g_surrogate=g.cuda())
    ref = ops.seq_logp_bwd(*args, g_logp=(g * adv).cuda())
    torch.cuda.synchronize()
    assert bool(ref.any()) and torch.equal(got, ref)
    # the token table alone, and an old table that is not the policy's: the ratios move and so do the bits
    got_t = ops.seq_ppo_bwd(xd, ys.cuda(), want[0], adv.cuda(), clip, clip, lens.int().cuda(), PAD,
                            g_token_surrogate=g.cuda().view(-1, 1).expand(n, W).contiguous())
    assert torch.equal(got_t, ref)
    moved = ops.seq_ppo_bwd(xd, ys.cuda(), want[0] + 0.05 * (zero + 1), adv.cuda(), 0.2, 0.2, lens.int().cuda(), PAD,
                            g_surrogate=g.cuda())
    assert not torch.equal(moved, ref)


# ------------------------------------------------------------------------------------------------------ 3. refusals
def raw_case():
    n, W, V = 2, 9, 30
    t = dict(x=torch.zeros(n * (W - 1), V), ys=torch.zeros(n, W, dtype=torch.long), old=torch.zeros(n, W),
             adv=torch.ones(n), g=torch.ones(n), gt=torch.ones(n, W))
    return n, W, V, {k: v.cuda() for k, v in t.items()}


def raw_fwd(ops, outs, **over):
    n, W, V, t = raw_case()
    a = dict(logits=t["x"].data_ptr(), ld=V, V=V, rows_per_seq=W - 1, row_shift=0, ys=t["ys"].data_ptr(), ld_ys=W,
             prefix_lens=None, pad_id=PAD, n=n, W=W, old=t["old"].data_ptr(), ld_old=W, adv=t["adv"].data_ptr(),
             clip_lo=0.2, clip_hi=0.2, token_logp=outs[0].data_ptr(), token_surrogate=outs[1].data_ptr(), ld_out=W,
             logp=outs[2].data_ptr(), surrogate=outs[3].data_ptr(), approx_kl=outs[4].data_ptr(),
             tokens=outs[5].data_ptr(), hits=outs[6].data_ptr(), clipped=outs[7].data_ptr())
    a.update(over)
    rc = ops._L().gct_seq_ppo(*a.values(), ops._st())
    torch.cuda.synchronize()
    return rc


def raw_bwd(ops, out, **over):
    n, W, V, t = raw_case()
    a = dict(logits=t["x"].data_ptr(), ld=V, V=V, rows_per_seq=W - 1, row_shift=0, ys=t["ys"].data_ptr(), ld_ys=W,
             prefix_lens=None, pad_id=PAD, n=n, W=W, old=t["old"].data_ptr(), ld_old=W, adv=t["adv"].data_ptr(),
             clip_lo=0.2, clip_hi=0.2, g_surrogate=t["g"].data_ptr(), g_token=t["gt"].data_ptr(), ld_g=W,
             dlogits=out.data_ptr(), ld_d=V)
    a.update(over)
    rc = ops._L().gct_seq_ppo_bwd(*a.values(), ops._st())
    torch.cuda.synchronize()
    return rc


def fwd_outs(n, W):
    return [torch.full(s, SENT, device="cuda") for s in ((n, W), (n, W), (n,), (n,), (n,))] + [
        torch.full((n,), 77, dtype=torch.int32, device="cuda") for _ in range(3)]


def untouched(outs):
    return all(bool((o == (SENT if o.dtype == torch.float32 else 77)).all()) for o in outs)


CLIP_REFUSALS = [dict(clip_lo=-0.01), dict(clip_lo=1.0), dict(clip_lo=NAN), dict(clip_hi=-0.01), dict(clip_hi=NAN)]
FWD_REFUSALS = [dict(logits=None), dict(ys=None), dict(old=None), dict(adv=None), dict(token_logp=None),
                dict(token_surrogate=None), dict(logp=None), dict(surrogate=None), dict(approx_kl=None),
                dict(tokens=None), dict(hits=None), dict(clipped=None), dict(ld=29),
                dict(W=257, rows_per_seq=256, ld_ys=257, ld_out=257, ld_old=257), dict(W=0), dict(ld_ys=8),
                dict(ld_out=8), dict(ld_old=8), dict(rows_per_seq=7), dict(row_shift=1), dict(row_shift=-1), dict(V=0),
                dict(n=-1)] + CLIP_REFUSALS
BWD_REFUSALS = [dict(logits=None), dict(ys=None), dict(old=None), dict(adv=None), dict(dlogits=None), dict(ld=29),
                dict(ld_d=29), dict(W=257, rows_per_seq=256, ld_ys=257, ld_old=257, ld_g=257), dict(W=0), dict(ld_ys=8),
                dict(ld_old=8), dict(ld_g=8), dict(rows_per_seq=7), dict(row_shift=1), dict(V=0),
                dict(g_surrogate=None, g_token=None)] + CLIP_REFUSALS


def test_seq_ppo_refuses_before_a_launch(ops):
    n, W, V, _ = raw_case()
    outs = fwd_outs(n, W)
    assert raw_fwd(ops, outs) == 0                                                # the case itself is fine
    assert not any(bool((o == (SENT if o.dtype == torch.float32 else 77)).any()) for o in outs)
    assert raw_fwd(ops, fwd_outs(n, W), clip_lo=0.0, clip_hi=0.0) == 0 and raw_fwd(ops, fwd_outs(n, W), clip_hi=9.0) == 0
    for over in FWD_REFUSALS:
        outs = fwd_outs(n, W)
        with pytest.raises(GctError, match="seq_ppo"):
            check(raw_fwd(ops, outs, **over), "gct_seq_ppo")
        assert untouched(outs), over
    assert raw_fwd(ops, outs, n=0) == 0 and untouched(outs)                       # no sequence: nothing is written
    x, ys = torch.zeros(16, 30, device="cuda"), torch.zeros(2, 9, dtype=torch.long, device="cuda")
    old, adv = torch.zeros(2, 9, device="cuda"), torch.ones(2, device="cuda")
    with pytest.raises(GctError, match="null"):
        ops.seq_ppo(None, ys, old, adv, 0.2, 0.2, V=30)
    with pytest.raises(GctError, match="null"):
        ops.seq_ppo(x, ys, None, adv, 0.2, 0.2)
    with pytest.raises(GctError, match="clip"):
        ops.seq_ppo(x, ys, old, adv, 1.0, 0.2)
    with pytest.raises(ValueError, match="old_token_logp"):
        ops.seq_ppo(x, ys, old[:, :8], adv, 0.2, 0.2)
    assert ops.seq_ppo(x, ys[:0], old[:0], adv[:0], 0.2, 0.2)[1].shape == (0, 9)   # the binding: no call at all


def test_seq_ppo_bwd_refuses_before_a_launch(ops):
    n, W, V, _ = raw_case()
    out = torch.full((n * (W - 1), V), SENT, device="cuda")
    assert raw_bwd(ops, out) == 0 and not bool((out == SENT).any())               # the case itself is fine
    assert raw_bwd(ops, out, g_token=None) == 0 and raw_bwd(ops, out, g_surrogate=None) == 0
    for over in BWD_REFUSALS:
        out = torch.full((n * (W - 1), V), SENT, device="cuda")
        with pytest.raises(GctError, match="seq_ppo_bwd"):
            check(raw_bwd(ops, out, **over), "gct_seq_ppo_bwd")
        assert bool((out == SENT).all()), over
    assert raw_bwd(ops, out, n=0) == 0 and bool((out == SENT).all())              # no sequence: nothing is written
    x, ys = torch.zeros(16, 30, device="cuda"), torch.zeros(2, 9, dtype=torch.long, device="cuda")
    old, one = torch.zeros(2, 9, device="cuda"), torch.ones(2, device="cuda")
    with pytest.raises(GctError, match="both gradients"):
        ops.seq_ppo_bwd(x, ys, old, one, 0.2, 0.2)
    with pytest.raises(GctError, match="do not hold"):
        ops.seq_ppo_bwd(x, ys, old, one, 0.2, 0.2, rows_per_seq=7, g_surrogate=one)
    with pytest.raises(GctError, match="clip"):
        ops.seq_ppo_bwd(x, ys, old, one, 0.2, -1.0, g_surrogate=one)
    assert ops.seq_ppo_bwd(x, ys[:0], old[:0], one[:0], 0.2, 0.2, g_surrogate=one[:0]).shape == (16, 30)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ 4. SeqPpoFn
class _NoGradient(torch.autograd.Function):
    """Identity whose backward hands None on: what a consumer that needs no gradient looks like to SeqPpoFn."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("use", ["both", "surrogate", "token", "nothing"])
def test_seq_ppo_fn_under_autograd(use):
    from gct_plus_amd import engine
    n, W, V = 5, 11, 31
    ys, lens, x, old, adv, g_s, g_ts = ppo_kernel_case(n, W, V, "plain")
    xd = x.cuda().requires_grad_()
    oldd, advd = old.cuda().requires_grad_(), adv.cuda().requires_grad_()
    out = engine.SeqPpoFn.apply(xd, ys.cuda(), lens.int().cuda(), PAD, 0, oldd, advd, CLIP, CLIP)
    surrogate, token_surrogate, logp, token_logp, approx_kl, tokens, hits, clipped = out
    assert surrogate.requires_grad and token_surrogate.requires_grad
    assert not any(t.requires_grad for t in (logp, token_logp, approx_kl, tokens, hits, clipped))
    ref = ppo_reference(x.double(), ys, lens, PAD, old.double(), adv.double(), CLIP, CLIP)
    assert torch.equal(tokens.cpu(), ref[5]) and torch.equal(hits.cpu(), ref[6]) and torch.equal(clipped.cpu(), ref[7])
    assert int(ref[7].sum()) > 0
    for got, want in ((token_logp, ref[0]), (token_surrogate, ref[1]), (logp, ref[2]), (surrogate, ref[3]),
                      (approx_kl, ref[4])):
        assert got.shape == want.shape
        assert float((got.detach().cpu().double() - want).abs().max()) <= W * 1e-4 * 2 * float(adv.abs().max() + 1)
    if use == "nothing":
        _NoGradient.apply(surrogate).sum().backward()                             # every incoming gradient is None
        assert xd.grad.shape == xd.shape and not xd.grad.any()
        return
    gs, gt = (None if use == "token" else g_s), (None if use == "surrogate" else g_ts)
    obj = sum((g.cuda() * o).sum() for g, o in ((gs, surrogate), (gt, token_surrogate)) if g is not None)
    obj.backward()
    assert xd.grad.shape == xd.shape and oldd.grad is None and advd.grad is None   # no gradient into old or advantage
    want = ppo_grad_reference(x.double(), ys, lens, PAD, old.double(), adv.double(), CLIP, CLIP,
                              g_surrogate=None if gs is None else gs.double(),
                              g_token_surrogate=None if gt is None else gt.double())
    g = (0 if gs is None else gs[:, None]) + (0 if gt is None else gt[:, 1:]) + torch.zeros(n, W - 1)
    rho = torch.exp(ref[0] - old.double())[:, 1:]
    gmax = float((g.double() * adv.double().view(-1, 1) * rho)[scored_columns(ys, lens)].abs().max())
    kernel_ratio(xd.grad, want, gmax, f"SeqPpoFn {use}")


# -------------------------------------------------------------------------------------------------- 5. sequence_ppo
def delta_table(shape, seed):
    """A table of deltas from tests/test_ppo_host.DELTAS, each with probability 1 / 5."""
    pick = torch.randint(0, len(DELTAS), shape, generator=torch.Generator().manual_seed(seed))
    return torch.tensor(DELTAS)[pick]


def test_sequence_ppo_shares_its_fields_with_sequence_logp_and_sequence_policy(ops):
    from gct_plus_amd.Train.finetune import frozen_prior
    model = build("pscavaetf", seed=31)
    prior = frozen_prior(model)
    perturb_out_bias(model)
    t = target_rows("pscavaetf", 7)
    z = t["z"].cuda().requires_grad_()
    args = (cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda())
    kw = dict(prefix_lens=t["lens"], pad_id=PAD)
    want = sequence_logp(model, z, *args, **kw)
    pol = sequence_policy(model, z, *args, prior=prior, **kw)
    old = want[3].detach()
    adv = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.25, -1.25])
    terms = sequence_ppo(model, z, *args, old, adv, clip=0.2, prior=prior, entropy=True, **kw)
    assert isinstance(terms, PpoTerms) and PpoTerms._fields[:9] == type(pol)._fields
    for name, w in zip(("logp", "tokens", "hits", "token_logp"), want):
        assert torch.equal(getattr(terms, name), w.detach()), name
    for name in ("entropy", "token_entropy", "kl", "token_kl", "prior_logp"):
        assert torch.equal(getattr(terms, name).detach(), getattr(pol, name).detach()), name
    assert terms.surrogate.requires_grad and terms.token_surrogate.requires_grad and terms.kl.requires_grad
    assert not terms.logp.requires_grad and not terms.approx_kl.requires_grad and not terms.clipped.requires_grad
    # the old policy is the policy: ratios of exactly 1
    assert torch.equal(terms.surrogate.detach().cpu(), adv * terms.tokens.cpu()) and not terms.clipped.any()
    assert not terms.approx_kl.any()
    bare = sequence_ppo(model, z, *args, old, adv, clip=(0.1, 0.3), **kw)
    assert bare.entropy is None and bare.kl is None and bare.prior_logp is None
    assert torch.equal(bare.surrogate, terms.surrogate)
    with_h = sequence_ppo(model, z, *args, old, adv, entropy=True, **kw)
    assert torch.equal(with_h.entropy, terms.entropy) and with_h.kl is None
    # refusals, before any device work
    for bad in (dict(old=old[:, :-1]), dict(old=old.long()), dict(adv=adv[:5]), dict(adv=adv * NAN), dict(clip=1.0),
                dict(clip=(0.2, -0.1)), dict(clip="x")):
        a = dict(dict(old=old, adv=adv, clip=0.2), **bad)
        with pytest.raises(ValueError):
            sequence_ppo(model, z, *args, a["old"], a["adv"], clip=a["clip"], **kw)
    with pytest.raises(ValueError, match="no column"):
        sequence_ppo(model, z, *args[:2], torch.full_like(t["ys"], PAD), old, adv, pad_id=PAD)
    with pytest.raises(ValueError, match="nconds"):
        sequence_ppo(model, z, *args, old, adv, prior=build("scavaetf", seed=33), **kw)


def oracle_ppo_grads(model, mtype, c2d, extra, t, old, adv):
    """The CPU oracle's autograd through ppo_reference: gradients of surrogate.sum() for every parameter and z."""
    from oracle import gct_oracle as O
    P = O.make_leaves({k: v.detach().cpu() for k, v in model.state_dict().items()})
    z = t["z"].clone().requires_grad_()
    out = ppo_reference(oracle_logits(P, mtype, c2d, extra, t, z=z), t["ys"], t["lens"], PAD, old, adv, CLIP, CLIP)
    out[3].sum().backward()
    return P, z.grad, out


@pytest.mark.parametrize("shortcuts", [True, False])
@pytest.mark.parametrize("mtype,c2d", [("vaetf", False), ("pscavaetf", False), ("pvaetf", True)])
def test_sequence_ppo_gradients_vs_oracle(ops, monkeypatch, mtype, c2d, shortcuts):
    """24 rows (tests/test_seq_logp_grad_gpu.py's row-plan case: the planner takes the live rows when it may), the
    sampling-time table = the policy's own log-probabilities + a delta table, advantages of both signs and zeros:
    gradients of surrogate.sum() for every decoder-side parameter and z against the oracle's autograd through the rule."""
    from gct_plus_amd import engine
    for name in ("COMPACT_FWD", "COMPACT_BWD", "COMPACT_KV", "COMPACT_ENC_KV"):
        monkeypatch.setattr(engine, name, shortcuts)
    extra = dict(use_cond2dec=True, use_cond2lat=False) if c2d else {}
    model = build(mtype, seed=31, **extra)                                        # eval mode
    t = target_rows(mtype, 8, lengths=(5, 20, 8, 12, 6, 16) + (6, 7, 9, 5, 8, 10) * 3)
    n = t["ys"].shape[0]
    adv = torch.randn(n, generator=torch.Generator().manual_seed(1))
    adv[::5] = 0
    z = t["z"].cuda().requires_grad_()
    args = (cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda())
    kw = dict(prefix_lens=t["lens"], pad_id=PAD)
    with torch.no_grad():
        now = sequence_logp(model, z, *args, **kw)[3].cpu()
    old = now + delta_table(now.shape, seed=2)
    model.zero_grad(set_to_none=True)
    terms = sequence_ppo(model, z, *args, old, adv, clip=CLIP, **kw)
    terms.surrogate.sum().backward()
    ops.assert_no_skipped_row_gradients()
    P, zg, ref = oracle_ppo_grads(model, mtype, c2d, extra, t, old, adv)
    scored = scored_columns(t["ys"], t["lens"])
    rho = torch.exp(ref[0].detach() - old)[:, 1:][scored]
    assert float(torch.minimum((rho - 0.8).abs(), (rho - 1.2).abs()).min()) >= 0.14   # the oracle's ratios: off the ties
    assert torch.equal(terms.clipped.cpu(), ref[7]) and int(ref[7].sum()) > 0 and torch.equal(terms.tokens.cpu(), ref[5])
    assert float((terms.surrogate.detach().cpu() - ref[3].detach()).abs().max()) <= 1e-3 * float(ref[3].detach().abs().max())
    floor = grad_floor([v.grad for v in P.values()] + [zg])
    seen = 0
    for name, p in model.named_parameters():
        e = P[name].grad
        if not name.startswith(("decoder.", "out.")):
            assert e is None or not e.any(), name                                 # the oracle agrees: z is an input
            assert p.grad is None or not p.grad.any(), f"{name}: the encoder side got a gradient"
            continue
        if e is None:
            assert p.grad is None or not p.grad.any(), name
            continue
        assert p.grad is not None, name
        assert_close(p.grad, e, 1e-5 * float(e.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad {name}")
        seen += 1
    assert seen > 20
    assert_close(z.grad, zg, 1e-5 * float(zg.abs().max()) + floor, 1e-3, f"{mtype} c2d={c2d} grad z")
    assert not z.grad.cpu()[adv == 0].any() and bool(z.grad.cpu()[adv != 0].any())   # A == 0 contributes nothing


# ------------------------------------------------------------------------------------------------------- 6. updates
def ppo_sampler():
    """A greedy sampler over the PPO update test's model (dropout 0, the oracle's initial state), its rows as a
    DecodedRows and the rewards."""
    from gct_plus_amd.Inference import sampling_tool
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.Model import model_dict
    cfg, state, t, reward = ppo_update_case()
    vs, vt = synthetic.vocab_sizes(PPO_MTYPE)
    nc = synthetic.n_conds(PPO_MTYPE)
    model = model_dict[PPO_MTYPE](vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).cuda()
    model.load_state_dict(state)
    SRC, TRG = update_vocabs(PPO_MTYPE)
    sp = sampling_tool.sampling_tool_dict[PPO_MTYPE](model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=20,
                                                     cond_dim=nc, decode_algo="greedy")
    return sp, t, DecodedRows(t["z"], t["ys"], t["src_mask"], t["dconds"], t["lens"]), reward


def fused_adam(model, lr=PPO_LR):
    from gct_plus_amd.optim import FusedAdam
    return FusedAdam(model.parameters(), lr=lr, betas=(0.9, 0.98), eps=1e-9, model=model)


def test_one_epoch_in_train_mode_is_reinforce_step_bit_for_bit():
    """n = 8 is a power of two, so (-1 / n) * A, the weight autograd hands gct_seq_logp_bwd in reinforce_step, and
    (g * A) with g = -(1 / n), the one gct_seq_ppo_bwd forms, are the same fp32 number; the ratios are exactly 1."""
    from gct_plus_amd.Train.finetune import ppo_update, reinforce_step
    final = []
    for ppo in (False, True):
        sp, t, rows, reward = ppo_sampler()
        assert len(reward) == 8
        start = {k: p.detach().clone() for k, p in sp.model.named_parameters()}
        opt = fused_adam(sp.model)
        if ppo:
            stats = ppo_update(sp, opt, rows, reward, epochs=1, train_mode=True)
            assert len(stats) == 1 and stats[0]["clip_fraction"] == 0.0 and stats[0]["approx_kl"] == 0.0
        else:
            reinforce_step(sp, opt, rows, reward)
        assert not sp.model.training
        final.append({k: p.detach().clone() for k, p in sp.model.named_parameters()})
    moved = [k for k in final[0] if not torch.equal(final[0][k], start[k])]
    assert moved and all(k.startswith(("decoder.", "out.")) for k in moved)
    for k in final[0]:
        assert torch.equal(final[0][k], final[1][k]), f"{k}: ppo_update(epochs=1) is not reinforce_step"


def device_clipped(terms, adv):
    """The clipped tokens of a PpoTerms as the kernel decided them, bool [n, W - 1]: a clipped token's surrogate is the
    fp32 product A * (1 + clip) or A * (1 - clip) exactly."""
    ts, A = terms.token_surrogate.detach().cpu()[:, 1:], adv.view(-1, 1)
    one, c = torch.ones(()), torch.tensor(CLIP)
    mask = ((A > 0) & (ts == A * (one + c))) | ((A < 0) & (ts == A * (one - c)))
    assert torch.equal(mask.sum(1).to(torch.int32), terms.clipped.cpu())
    return mask


def test_four_epochs_follow_the_oracle(ops):
    from gct_plus_amd.Train.finetune import advantages, ppo_update
    sp, t, rows, reward = ppo_sampler()
    model = sp.model
    n = t["ys"].shape[0]
    ys0 = t["ys"][:1, :1].repeat(n, 1)
    greedy_matches_uncached(sp, t["z"], t["src_mask"], t["dconds"], ys0)          # folds the projections of the old weights
    fold_before = sp.kv._fold_key
    frozen = {k: p.detach().clone() for k, p in model.named_parameters() if not k.startswith(("decoder.", "out."))}
    seen, inner = [], sp.ppo_terms

    def spy(*a, **kw):
        terms = inner(*a, **kw)
        seen.append(terms)
        return terms
    sp.ppo_terms = spy
    got = ppo_update(sp, fused_adam(model), rows, reward, epochs=PPO_EPOCHS, clip=CLIP)
    ops.assert_no_skipped_row_gradients()
    assert not model.training and len(got) == PPO_EPOCHS == len(seen)
    assert all(set(g) == {"loss", "mean_surrogate", "clip_fraction", "approx_kl", "tokens"} for g in got)
    want = oracle_ppo_run()
    scored = want["scored"]
    tokens = int(scored.sum())
    adv = advantages(reward.cuda()).cpu()                                         # the device's bits, as ppo_update's
    for k in ("loss", "approx_kl", "clip_fraction"):
        print(f"{k}: device {[round(g[k], 7) for g in got]}\n{' ' * len(k)}  oracle {[round(v, 7) for v in want[k]]}")
    assert all(g["tokens"] == tokens for g in got)
    assert all(abs(g["loss"] - w) <= 1e-3 * abs(w) for g, w in zip(got, want["loss"])), (got, want["loss"])
    assert all(abs(g["loss"] + g["mean_surrogate"]) <= 1e-6 * abs(g["loss"]) for g in got)
    assert got[0]["approx_kl"] == 0.0 and got[0]["clip_fraction"] == 0.0
    assert all(abs(g["approx_kl"] - w) <= 1e-3 * w for g, w in zip(got[1:], want["approx_kl"][1:]))
    for e in range(PPO_EPOCHS):
        near = near_a_boundary(want["rho"][e], scored)
        assert int(near.sum()) <= NEAR_CAP * tokens
        mine = device_clipped(seen[e], adv)
        assert torch.equal(mine[~near], want["clipped"][e][~near]), f"epoch {e}: the clipped sets differ"
    assert got[-1]["clip_fraction"] > 0 and int(seen[-1].clipped.sum()) > 0       # tokens are in fact clipped in the end
    for k, p in model.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach(), frozen[k]), f"{k}: the encoder side moved"
    del sp.ppo_terms
    greedy_matches_uncached(sp, t["z"], t["src_mask"], t["dconds"], ys0)          # the sampler decodes with the new weights
    assert sp.kv._fold_key != fold_before                                         # (its folded projections were redone)


def test_target_kl_minibatches_and_a_table_of_the_callers(ops):
    from gct_plus_amd.Train.finetune import advantages, frozen_prior, ppo_loss, ppo_update
    want = oracle_ppo_run()
    assert want["approx_kl"][1] > 1e-3
    sp, t, rows, reward = ppo_sampler()
    short = ppo_update(sp, fused_adam(sp.model), rows, reward, epochs=PPO_EPOCHS, clip=CLIP, target_kl=1e-3)
    assert len(short) == 2 and short[1]["approx_kl"] > 1e-3 >= short[0]["approx_kl"]   # epoch 2 was not started
    # the caller's own table (Sampling.score, eval mode, CPU) is the one ppo_update takes itself
    sp2, _, _, _ = ppo_sampler()
    own = ppo_update(sp2, fused_adam(sp2.model), rows, reward, epochs=2, clip=CLIP,
                     old_token_logp=sp2.score(*rows).token_logp)
    assert own == short
    # minibatches of 3, 3 and 2 rows, against the same updates made by hand
    final, stats = [], []
    for by_hand in (False, True):
        sp, t, rows, reward = ppo_sampler()
        prior = frozen_prior(sp.model)
        opt = fused_adam(sp.model)
        if not by_hand:
            stats = ppo_update(sp, opt, rows, reward, epochs=2, clip=(0.1, 0.3), minibatch=3, entropy_coef=0.05,
                               kl_coef=0.5, prior=prior, normalize=True)
            assert len(stats) == 2 and set(stats[0]) == {"loss", "mean_surrogate", "clip_fraction", "approx_kl", "tokens",
                                                          "mean_entropy", "mean_kl", "mean_prior_logp"}
            assert stats[0]["mean_kl"] > 0 and stats[0]["approx_kl"] > 0          # minibatches 2 and 3 see a moved policy
        else:
            adv = advantages(reward.cuda(), normalize=True).cpu()                 # the device's bits, as ppo_update's
            sp.model.eval()
            with torch.no_grad():
                old = sp.logp(*rows).token_logp
            for _ in range(2):
                for lo, hi in ((0, 3), (3, 6), (6, 8)):
                    part = tuple(None if a is None else a[lo:hi] for a in rows)
                    terms = sp.ppo_terms(*part, old_token_logp=old[lo:hi], advantage=adv[lo:hi], clip=(0.1, 0.3),
                                         prior=prior, entropy=True)
                    opt.zero_grad(set_to_none=True)
                    ppo_loss(terms, 0.05, 0.5).backward()
                    opt.step()
        final.append({k: p.detach().clone() for k, p in sp.model.named_parameters()})
    for k in final[0]:
        assert torch.equal(final[0][k], final[1][k]), f"{k}: minibatch=3 is not the three updates made by hand"
    ops.assert_no_skipped_row_gradients()


# ------------------------------------------------------------------------------------------------------ 7. front end
@pytest.mark.parametrize("cls,mtype", [("VaetfSampling", "vaetf"), ("PscavaetfSampling", "pscavaetf")])
def test_ppo_terms_of_decoded_rows(cls, mtype):
    n = 6
    g = torch.Generator().manual_seed(6)
    z = torch.randn(n, 30, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    sp = make_sampler(cls, mtype, "multinomial", None, with_logp=True)
    if mtype == "vaetf":
        out = sp.sample_smiles(n, zs=z, return_rows=True)
    else:
        out = sp.sample_smiles(dconds, "c1ccccc1", zs=z, transform=False, return_rows=True)
    rows = out[4]
    old = sp.score(*rows).token_logp                                              # the sampling-time policy, on the CPU
    adv = torch.tensor([1.0, -0.5, 0.0, 2.0, 0.25, -1.25])
    terms = sp.ppo_terms(*rows, old_token_logp=old, advantage=adv, clip=0.2)
    L = rows.ys.shape[1]
    assert isinstance(terms, PpoTerms) and all(x.is_cuda for x in terms if x is not None)
    assert terms.surrogate.shape == terms.approx_kl.shape == terms.clipped.shape == (n,)
    assert terms.token_surrogate.shape == terms.token_logp.shape == (n, L) and terms.entropy is None
    assert terms.surrogate.requires_grad and bool((terms.tokens >= 1).all())
    assert torch.equal(terms.token_logp.cpu(), old)                               # score's bits: ratios of exactly 1
    assert torch.equal(terms.surrogate.detach().cpu(), adv * terms.tokens.cpu()) and not terms.clipped.any()
    perturb_out_bias(sp.model)
    moved = sp.ppo_terms(*rows, old_token_logp=old, advantage=adv, clip=(0.0, 0.0), entropy=True)
    assert bool((moved.approx_kl > 0).all()) and int(moved.clipped.sum()) > 0 and bool((moved.entropy > 0).all())
    moved.surrogate.sum().backward()
    assert any(p.grad is not None and bool(p.grad.any()) for p in sp.model.parameters())
    with pytest.raises(TypeError):
        sp.ppo_terms(*rows)                                                       # old_token_logp and advantage are required
