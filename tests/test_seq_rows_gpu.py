"""The scored-token kernels with logits rows BEHIND a sequence's last token column.

The ABI allows rows_per_seq > row_shift + W - 1; every other test uses exactly row_shift + W - 1.  Here all six entry
points (gct_seq_logp / _bwd, gct_seq_dist / _bwd, gct_seq_ppo / _bwd) run twice on the same case: on the tight layout, and
on a loose one with three more logits rows per sequence -- NaN in them and in the shift rows in front.  Nothing may move:
every forward output and every backward row the two layouts share is the same bit for bit, the trailing rows of dlogits
are exact zeros, everything is finite.  No tolerance is involved.
"""
import pytest
import torch

from tests.test_mixed_scaffold_decode_gpu import PAD
from tests.test_ppo_host import CLIP, ppo_inputs
from tests.test_score_gpu import kernel_case
from tests.test_seq_logp_grad_gpu import weights

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHIFT, TAIL = 2, 3
SHAPES = [(3, 5, 30), (3, 6, 65)]                         # more columns than waves, more vocabulary than lanes


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def bits(t):
    return t.cpu().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def laid_out(rows, tail):
    """rows [n, W - 1, V] behind SHIFT rows of NaN and in front of `tail` more: ([n * R, V] on the device, R)."""
    n, Wm1, V = rows.shape
    R = SHIFT + Wm1 + tail
    big = torch.full((n, R, V), NAN)
    big[:, SHIFT:SHIFT + Wm1] = rows
    return big.cuda().view(n * R, V), R


def run_all(ops, tail, ys, lens, x, q, old, adv, g_s, g_ts, gs):
    """The six entry points on one layout: (the 16 forward outputs, the three dlogits as [n, R, V], each written into a
    buffer that started as NaN)."""
    n = ys.shape[0]
    xd, R = laid_out(x, tail)
    qd, _ = laid_out(q, tail)
    geom = dict(row_shift=SHIFT, rows_per_seq=R)
    y, t0 = ys.cuda(), lens.int().cuda()
    fwd = ops.seq_logp(xd, y, t0, PAD, **geom) + ops.seq_dist(xd, y, t0, PAD, prior_logits2d=qd, **geom) + ops.seq_ppo(
        xd, y, old.cuda(), adv.cuda(), CLIP, CLIP, t0, PAD, **geom)
    dl = [torch.full_like(xd, NAN) for _ in range(3)]
    ops.seq_logp_bwd(xd, y, t0, PAD, g_logp=gs[0].cuda(), g_token=gs[1].cuda(), out=dl[0], **geom)
    ops.seq_dist_bwd(xd, y, t0, PAD, prior_logits2d=qd, g_entropy=gs[0].cuda(), g_token_entropy=gs[1].cuda(),
                     g_kl=gs[2].cuda(), g_token_kl=gs[3].cuda(), out=dl[1], **geom)
    ops.seq_ppo_bwd(xd, y, old.cuda(), adv.cuda(), CLIP, CLIP, t0, PAD, g_surrogate=g_s.cuda(),
                    g_token_surrogate=g_ts.cuda(), out=dl[2], **geom)
    torch.cuda.synchronize()
    return fwd, [d.cpu().view(n, R, -1) for d in dl]


@pytest.mark.parametrize("n,W,V", SHAPES)
def test_rows_behind_the_last_column_change_nothing(ops, n, W, V):
    ys, lens, x = kernel_case(n, W, V, seed=n * 1000 + W)
    q = (torch.randn(n, W - 1, V, generator=torch.Generator().manual_seed(W)) * 4).clamp(-15, 15)
    old, adv, g_s, g_ts = (t.float() for t in ppo_inputs(ys, lens, x, seed=W))
    case = (ys, lens, x, q, old, adv, g_s, g_ts, weights(n, W, seed=W) + weights(n, W, seed=W + 1))
    tight_fwd, tight_bwd = run_all(ops, 0, *case)
    loose_fwd, loose_bwd = run_all(ops, TAIL, *case)
    assert len(tight_fwd) == 16 and int(tight_fwd[2].sum()) > 0                   # tokens were scored
    for i, (a, b) in enumerate(zip(tight_fwd, loose_fwd)):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"forward output {i} not finite"
        assert torch.equal(bits(a), bits(b)), f"forward output {i} moved with the layout"
    used = SHIFT + W - 1
    for name, a, b in zip(("seq_logp_bwd", "seq_dist_bwd", "seq_ppo_bwd"), tight_bwd, loose_bwd):
        assert a.shape[1] == used and b.shape[1] == used + TAIL
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{name}: a row never written"
        assert bool(a.any()), name                                                # a gradient was there to move
        assert torch.equal(bits(a), bits(b[:, :used])), f"{name}: the shared rows moved with the layout"
        assert not bits(b[:, used:]).any(), f"{name}: a trailing row is not exact zeros"
