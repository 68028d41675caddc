"""The slab reductions of csrc/reduce.hip called directly: every lane class of launch_reduce, the scalar fallback,
`accumulate`, and the deferred form (recorded between gct_reduce_defer_begin / _end, run as one launch per 24 jobs).

Values against the fp64 column sum.  The tolerance is the bound of fp32 summation in ANY order (Higham, Accuracy and
Stability of Numerical Algorithms, eq. 4.4): |err| <= (t - 1) u / (1 - (t - 1) u) * sum |x| over t terms, u = 2^-24 --
stated here as t u sum |x|.  Deferred against direct, and a call against its repetition, are bit for bit.  Every
destination starts as NaN, so an element that no lane wrote fails."""
import math

import pytest
import torch

from tests.test_kernels_gpu import close, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def _reduce(ops, slabs, nslab, stride, dst, n, accumulate=0):
    from gct_plus_amd._lib import check
    check(ops._L().gct_reduce_slabs(slabs.data_ptr(), nslab, stride, dst.data_ptr(), n, accumulate, ops._st()),
          "gct_reduce_slabs")


def _check_sum(got, terms64, what):
    """terms64 [t, n] fp64: every term of every destination element."""
    t = terms64.shape[0]
    ref, tol = terms64.sum(0), t * U * terms64.abs().sum(0) + 1e-45
    err = (got.detach().cpu().double() - ref).abs()
    assert torch.isfinite(got).all(), f"{what}: an element was not written"
    ratio = float((err / tol).max())
    print(f"reduce_slabs {what}: worst error / tolerance {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x the summation bound"
    return ratio


# (nslab, n, lanes): launch_reduce takes 4 lanes when n / 4 >= 16384 or nslab <= 4, else 16 when n / 4 >= 1024 or
# nslab <= 16, else 64
SHAPES = [(3, 1024, 4), (40, 65536, 4), (12, 512, 16), (200, 4096, 16), (1024, 512, 64), (33, 8, 64), (1, 64, 4),
          (1, 8, 4), (17, 4, 64), (5, 16388, 16)]


def test_the_shapes_cover_every_lane_class():
    for nslab, n, lanes in SHAPES:
        n4 = n // 4
        assert n % 4 == 0
        assert lanes == (4 if (n4 >= 16384 or nslab <= 4) else (16 if (n4 >= 1024 or nslab <= 16) else 64))
    assert {s[2] for s in SHAPES} == {4, 16, 64}


@pytest.mark.parametrize("nslab,n,lanes", SHAPES)
@pytest.mark.parametrize("pad", [0, 12])
def test_reduce_slabs_values(ops, nslab, n, lanes, pad):
    """pad: stride = n + pad > n (the floats between two slabs are NaN: a lane that strays into them poisons the sum)."""
    stride = n + pad
    buf = torch.full((nslab, stride), float("nan"))
    x = rnd(nslab, n, seed=nslab + n)
    buf[:, :n] = x
    slabs = buf.to(DEV)
    guard = torch.full((n + 8,), float("nan"), device=DEV)
    dst = guard[:n]
    _reduce(ops, slabs, nslab, stride, dst, n)
    _check_sum(dst, x.double(), f"nslab={nslab} n={n} stride={stride}")
    assert torch.isnan(guard[n:]).all(), "wrote behind the destination"
    again = torch.full((n,), float("nan"), device=DEV)
    _reduce(ops, slabs, nslab, stride, again, n)
    assert torch.equal(again, dst), "the same call twice is not bit-identical"
    # accumulate: dst += sum
    base = rnd(n, seed=7)
    acc = base.to(DEV).clone()
    _reduce(ops, slabs, nslab, stride, acc, n, accumulate=1)
    _check_sum(acc, torch.cat([x.double(), base.double()[None]]), f"accumulate nslab={nslab} n={n} stride={stride}")


@pytest.mark.parametrize("nslab,n,stride,dst_off", [(5, 7, 7, 0), (40, 1026, 1026, 0), (9, 1024, 1027, 0), (9, 1024, 1024, 1),
                                                    (1, 1, 1, 0), (300, 1026, 1030, 1)])
def test_reduce_slabs_scalar_fallback(ops, nslab, n, stride, dst_off):
    """n % 4 != 0, stride % 4 != 0 or a destination that is not 16-byte aligned: the scalar kernel."""
    assert n % 4 or stride % 4 or dst_off % 4
    buf = torch.full((nslab, stride), float("nan"))
    x = rnd(nslab, n, seed=3)
    buf[:, :n] = x
    slabs = buf.to(DEV)
    guard = torch.full((n + 16,), float("nan"), device=DEV)
    dst = guard[dst_off:dst_off + n]
    _reduce(ops, slabs, nslab, stride, dst, n)
    _check_sum(dst, x.double(), f"scalar nslab={nslab} n={n} stride={stride} off={dst_off}")
    assert torch.isnan(guard[:dst_off]).all() and torch.isnan(guard[dst_off + n:]).all()
    again = torch.full((n + 16,), float("nan"), device=DEV)[dst_off:dst_off + n]
    _reduce(ops, slabs, nslab, stride, again, n)
    assert torch.equal(again, dst)
    base = rnd(n, seed=8)
    guard[dst_off:dst_off + n] = base.to(DEV)
    _reduce(ops, slabs, nslab, stride, dst, n, accumulate=1)
    _check_sum(dst, torch.cat([x.double(), base.double()[None]]), "scalar accumulate")


# the job mix of the deferral tests: (nslab, n) of the three lane classes, small enough for 100 of them
JOB_KINDS = [(3, 1024), (12, 512), (33, 8), (20, 4096), (64, 256), (2, 64), (5, 16388)]
TABLE = 96


def _jobs(count):
    jobs = []
    for i in range(count):
        nslab, n = JOB_KINDS[i % len(JOB_KINDS)]
        jobs.append((rnd(nslab, n, seed=100 + i).to(DEV), nslab, n))
    return jobs


@pytest.mark.parametrize("count", [5, 30, 100])
def test_deferred_reductions_equal_direct_ones(ops, count):
    """5 jobs: one launch; 30: two launches (24 jobs each); 100: the table holds 96, the rest run at once."""
    L = ops._L()
    jobs = _jobs(count)
    direct = []
    for slabs, nslab, n in jobs:
        d = torch.full((n,), float("nan"), device=DEV)
        _reduce(ops, slabs, nslab, n, d, n)
        direct.append(d)
    assert L.gct_reduce_defer_pending() == 0
    dsts = [torch.full((n,), float("nan"), device=DEV) for _, _, n in jobs]
    assert L.gct_reduce_defer_begin() == 0
    try:
        for i, ((slabs, nslab, n), d) in enumerate(zip(jobs, dsts)):
            _reduce(ops, slabs, nslab, n, d, n)
            assert L.gct_reduce_defer_pending() == min(i + 1, TABLE)
        torch.cuda.synchronize()
        for i, d in enumerate(dsts):         # recorded, not launched -- and launched at once when the table is full
            assert bool(torch.isnan(d).all()) == (i < TABLE), f"job {i} before the flush"
    finally:
        rc = L.gct_reduce_defer_end(ops._st())
    assert rc == 0 and L.gct_reduce_defer_pending() == 0
    for i, (d, ref) in enumerate(zip(dsts, direct)):
        assert torch.equal(d, ref), f"job {i} of {count} {JOB_KINDS[i % len(JOB_KINDS)]}: deferred != direct"
    # deferral is off again: a call runs at once
    slabs, nslab, n = jobs[0]
    d = torch.full((n,), float("nan"), device=DEV)
    _reduce(ops, slabs, nslab, n, d, n)
    assert L.gct_reduce_defer_pending() == 0 and torch.equal(d, direct[0])


def test_flush_keeps_recording(ops):
    L = ops._L()
    jobs = _jobs(4)
    dsts = [torch.full((n,), float("nan"), device=DEV) for _, _, n in jobs]
    assert L.gct_reduce_defer_begin() == 0
    try:
        for (slabs, nslab, n), d in zip(jobs[:2], dsts[:2]):
            _reduce(ops, slabs, nslab, n, d, n)
        assert L.gct_reduce_defer_flush(ops._st()) == 0 and L.gct_reduce_defer_pending() == 0
        for (slabs, nslab, n), d in zip(jobs[2:], dsts[2:]):
            _reduce(ops, slabs, nslab, n, d, n)
        assert L.gct_reduce_defer_pending() == 2
        torch.cuda.synchronize()
        assert all(torch.isfinite(d).all() for d in dsts[:2]) and all(torch.isnan(d).all() for d in dsts[2:])
    finally:
        rc = L.gct_reduce_defer_end(ops._st())
    assert rc == 0 and L.gct_reduce_defer_pending() == 0
    for (slabs, nslab, n), d in zip(jobs, dsts):
        _check_sum(d, slabs.cpu().double(), f"after flush nslab={nslab} n={n}")


def test_an_accumulation_flushes_what_was_recorded(ops):
    """dst = sum(A) recorded, dst += sum(B) must see it: the accumulating call flushes first and runs at once."""
    L = ops._L()
    n = 512
    a, b, c = rnd(12, n, seed=1).to(DEV), rnd(40, n, seed=2).to(DEV), rnd(3, n, seed=3).to(DEV)

    def sequence(dst, other):
        _reduce(ops, a, 12, n, dst, n)
        pend_a = L.gct_reduce_defer_pending()
        _reduce(ops, b, 40, n, dst, n, accumulate=1)
        pend_b = L.gct_reduce_defer_pending()
        _reduce(ops, c, 3, n, other, n)
        return pend_a, pend_b, L.gct_reduce_defer_pending()

    ref, ref_o = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    assert sequence(ref, ref_o) == (0, 0, 0)
    got, got_o = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    assert L.gct_reduce_defer_begin() == 0
    try:
        pend = sequence(got, got_o)
    finally:
        rc = L.gct_reduce_defer_end(ops._st())
    assert rc == 0 and pend == (1, 0, 1) and L.gct_reduce_defer_pending() == 0
    assert torch.equal(got, ref) and torch.equal(got_o, ref_o)
    _check_sum(got, torch.cat([a.cpu().double(), b.cpu().double()]), "recorded sum + accumulation")


@pytest.mark.parametrize("n_c", [0, 3])
def test_embedding_backward_under_deferred_reductions(ops, n_c):
    """embed_pe_bwd ends in a slab reduction that is recorded inside deferred_reductions(); kld_fwd, the next user of
    the shared workspace, writes 1024 partial sums over its head before the flush.  dtable must not notice: the slabs
    live in the kept workspace.  (With the slabs in the shared workspace, dtable row 0 is the KLD's partial sums.)"""
    if not ops.DEFER_REDUCTIONS or ops.SIDE_ENABLED:
        pytest.skip("deferred_reductions() records nothing with GCT_DEFER_REDUCTIONS=0 or the side stream")
    B, S, d, V = 5, 20, 64, 30
    tok = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(0))
    dout = rnd(B * (S + n_c), d, seed=4)
    exp = torch.zeros(V, d, dtype=torch.double)
    exp.index_add_(0, tok.reshape(-1), dout.double().view(B, S + n_c, d)[:, n_c:].reshape(-1, d) * math.sqrt(d))
    mu, lv = rnd(1 << 18, seed=5).to(DEV), rnd(1 << 18, seed=6, scale=0.5).to(DEV)
    dtable = torch.full((V, d), float("nan"), device=DEV)
    dcond = torch.full((B, n_c, d), float("nan"), device=DEV) if n_c else None
    tokg, doutg = tok.to(DEV), dout.to(DEV)
    try:
        with ops.deferred_reductions() as ctx:
            assert ctx.mine and ops._L().gct_reduce_defer_pending() == 0
            ops.embed_pe_bwd(doutg, tokg, dtable, dcond, n_c, math.sqrt(d), 0.0, 0, 0)
            assert ops._L().gct_reduce_defer_pending() == 1, "the embedding's reduction was not recorded"
            kld = ops.kld_fwd(mu, lv)
    finally:
        ops._L().gct_reduce_defer_end(ops._st())        # a failure above cannot leave recording on
    assert ops._L().gct_reduce_defer_pending() == 0
    # the existing embedding tolerance (test_embed_pe: same B, S, d, V)
    close(dtable, exp, 1e-4, 1e-5, "dtable under deferred reductions")
    close(kld, -0.5 * torch.sum(1 + lv.cpu().double() - mu.cpu().double().pow(2) - lv.cpu().double().exp()),
          1e-3 * math.sqrt((1 << 18) / 2576), 1e-6, "kld next to it")
    direct = torch.full((V, d), float("nan"), device=DEV)
    ops.embed_pe_bwd(doutg, tokg, direct, dcond, n_c, math.sqrt(d), 0.0, 0, 0)
    assert torch.equal(dtable, direct), "deferred dtable != direct dtable"
