"""gct_linear_bwd (ops.linear_bwd): one Linear's weight gradient and input gradient as ONE bf16 tile launch, against the
two separate calls (ops.PAIR_BWD off) on the smallest shapes the planner pairs -- the dgrad needs more than 160 tiles of
128 x 256 to be on the large-tile route, i.e. about 10 400 rows at K = 512 (fewer where N = 128 keeps the small-tile kernel away).

A shape counts only if ops.linear_bwd_route says it is paired (asserted first; the launch counters confirm it: two GEMM
problems, one kernel launch).  Then
  dX   bit-identical to gct_linear_dgrad (same tiles, same epilogue, no tail launch in between);
  dW   bit-identical to gct_linear_wgrad when the pair's split equals gct_wgrad_route's; otherwise within the derived
       bound of tests/wgrad_ref.py with the paired call's own nsplit, against the fp64 reference;
  db   like dW: bit-identical at an equal split; at another split the column sums are grouped differently (one partial
       per slab), so only wgrad_ref.bound_b can hold -- bit-identity is not attainable there.
Rows: M % 128 != 0 everywhere.  M % 32 != 0 keeps the weight gradient off the bf16 tile route (its reduction runs over
whole 32-row tiles), so such an M is the refused shape: the call must then BE the two separate calls, bit for bit."""
import types

import pytest
import torch

from tests import wgrad_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 512


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as o
    keep_pair, keep_mode = o.PAIR_BWD, o.gemm_get_mode()
    yield o
    o.PAIR_BWD = keep_pair
    o.gemm_set_mode(keep_mode)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


_REF = {}


def fp64_ref(key, dys, x, tiles):
    """tests/wgrad_ref.reference of a data set, computed once"""
    if key not in _REF:
        _REF[key] = (W.reference(dys, x, tiles), W.x_abs_colsum(x, tiles))
    return _REF[key]


def counters(ops):
    return ops.gemm_launch_counts()[1], int(ops._L().gct_gemm_x6_kernel_launches()), ops.gemm_x3_launches()


def run_both(ops, M, nseg, nper, *, depi=0, bias=True, tiles=None, mode=W.BF16X6, live=None, pre=None, pre_full=False,
             expect_paired=True, lddy=None, seed=0):
    """-> (route, separate (dw, db, dx), paired (dw, db, dx), dy segments and x on the CPU)"""
    N = nseg * nper
    lddy = lddy or N
    ops.gemm_set_mode(mode)
    route = ops.linear_bwd_route(M, nseg, nper, K, lddy, K, K, K, depi, want_bias=bias, mode=mode)
    assert bool(route[0]) == expect_paired, f"planner: {route}"
    dy = rnd(M, lddy, seed=seed + 1)
    for s in range(nseg):
        dy[:, s * nper:(s + 1) * nper] *= W.SEG_SCALES[s]
    kt = None
    if tiles is not None:                                       # dY is zero outside the listed tiles, as the engine's lists promise
        keep = torch.zeros(M, dtype=torch.bool)
        keep[W.rows_of_tiles(tiles, M)] = True
        dy[~keep] = 0
        kt = (torch.tensor(tiles + [0] * 8, dtype=torch.int32, device=DEV),
              torch.tensor([len(tiles)], dtype=torch.int32, device=DEV))
    x = rnd(M, K, seed=seed + 2)
    wflat = rnd(N * K, seed=seed + 3, scale=0.05).to(DEV)
    ops.register_planes(wflat, ops.split_planes(wflat))
    ws = [wflat[s * nper * K:(s + 1) * nper * K].view(nper, K) for s in range(nseg)]
    dyg, xg = dy.to(DEV), x.to(DEV)
    dys = [dyg[:, s * nper:(s + 1) * nper] for s in range(nseg)]
    base = rnd(M, K, seed=seed + 4).to(DEV)                      # what ACCUM adds to
    out = []
    for pair in (False, True):
        ops.PAIR_BWD = pair
        dws = [torch.full((nper, K), float("nan"), device=DEV) for _ in range(nseg)]
        dbs = [torch.full((nper,), float("nan"), device=DEV) if bias else None for _ in range(nseg)]
        dx = base.clone()
        c0 = counters(ops)
        ops.linear_bwd(dys, lddy, xg, ws, dws, dbs, dx, depi=depi, pre=pre, p=0.1, seed=11, site=3, kt=kt, live=live,
                       pre_full=pre_full)
        torch.cuda.synchronize()
        c1 = counters(ops)
        if pair and expect_paired:                              # two GEMM problems, one kernel launch
            if mode == W.BF16X6:
                assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (2, 1, 0)
            else:
                assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, 0, 1)
        elif mode == W.BF16X6 and expect_paired:
            assert c1[0] - c0[0] == 2 and c1[1] - c0[1] >= 2
        out.append((torch.cat(dws).cpu(), torch.cat(dbs).cpu() if bias else None, dx.cpu()))
    ops.unregister_planes(wflat)
    cpu_dys = [dy[:, s * nper:(s + 1) * nper] for s in range(nseg)]
    return route, out[0], out[1], cpu_dys, x


def check(ops, key, M, nseg, nper, *, tiles=None, mode=W.BF16X6, bias=True, **kw):
    route, sep, pr, dys, x = run_both(ops, M, nseg, nper, tiles=tiles, mode=mode, bias=bias, **kw)
    assert torch.equal(pr[2], sep[2]), "dX differs from gct_linear_dgrad"
    assert torch.isfinite(pr[0]).all()
    wr = ops.wgrad_route(M, nseg, nper, K, kw.get("lddy") or nseg * nper, K, want_bias=bias, mode=mode)
    same_split = (route[1], route[2]) == (wr[1], wr[2])
    if same_split:
        assert torch.equal(pr[0], sep[0]), "dW differs at an equal split"
        if bias:
            assert torch.equal(pr[1], sep[1]), "db differs at an equal split"
    ref, xcol = fp64_ref(key, dys, x, tiles)
    rw = W.ratio(pr[0], ref.dw, W.bound_w(ref, mode, route[1], xcol))
    rb = W.ratio(pr[1], ref.db, W.bound_b(ref, route[1])) if bias else 0.0
    print(f"[bwd pair] {key}: route {route} wgrad_route {wr} same split {same_split} err/bound dW {rw:.4f} db {rb:.4f}")
    assert rw <= 1.0 and rb <= 1.0, (rw, rb)
    return route, same_split, pr


M1 = 13344          # 104 x 128 + 32: the pair takes fewer, longer splits than the weight gradient alone
M_EQ = 16832        # 131 x 128 + 64: the pair's split is gct_wgrad_route's (31 x 544 rows), so dW and db are bit-identical


def test_store_with_bias_equal_split_bit_identical(ops):
    _, same, _ = check(ops, "e", M_EQ, 1, 512, seed=0)
    assert same


def test_narrow_layer_equal_split_bit_identical(ops):
    """N = 128: 130 dgrad tiles (one round) behind 104 weight-gradient workgroups; M = 64 x 128 + 32"""
    _, same, _ = check(ops, "f", 8224, 1, 128, seed=60)
    assert same


def test_accumulate_no_bias_other_split(ops):
    """dW against fp64 only: 14 splits of 960 rows where gct_linear_wgrad makes 30 of 448"""
    _, same, _ = check(ops, "a", M1, 1, 512, depi=1, bias=False, seed=0)
    assert not same


def test_store_with_bias_other_split(ops):
    _, same, _ = check(ops, "a", M1, 1, 512, seed=0)
    assert not same


def test_three_segments_accumulate(ops):
    """dQ | dK | dV cut out of one buffer with a wider leading dimension; M = 81 x 128 + 96"""
    check(ops, "b", 10464, 3, 128, depi=1, lddy=3 * 128 + 8, seed=10)


def test_tile_list_that_omits_tiles(ops):
    nt = M1 // 32
    tiles = sorted(torch.randperm(nt, generator=torch.Generator().manual_seed(4))[:2 * nt // 3].tolist())
    check(ops, "c", M1, 1, 512, tiles=tiles, seed=20)


def test_bf16x3_mode(ops):
    _, same, _ = check(ops, "e", M_EQ, 1, 512, mode=W.BF16X3, seed=0)
    assert same


@pytest.mark.parametrize("pre_full", [True, False])
def test_mul_saved_on_compact_rows_through_the_quad_map(ops, pre_full):
    """the FFN-2 pair of a compacted backward: the rows are live quads of a larger row space, the saved factor is read
    through the quad map (pre_rows) or from a gathered copy; padding quads give zero rows"""
    Mc, Mfull, p = M1, 2 * M1, 0.1
    g = torch.Generator().manual_seed(5)
    quads = torch.randperm(Mfull // 4, generator=g)[:Mc // 4].sort().values.to(torch.int32)
    quads[-5:] = -1
    qpad = torch.cat([quads, torch.full((32,), -1, dtype=torch.int32)])
    live = types.SimpleNamespace(quad_list=qpad.to(DEV), Mc=Mc)
    saved = rnd(Mfull, K, seed=1) * (torch.rand(Mfull, K, generator=g) >= p)
    if not pre_full:
        rows = (quads.long().clamp(min=0)[:, None] * 4 + torch.arange(4)[None, :]).reshape(-1)
        saved = (saved[rows] * (quads.long() >= 0).repeat_interleave(4)[:, None]).contiguous()
    _, _, pr = check(ops, "d", Mc, 1, 256, depi=3, bias=False, live=live, pre=saved.to(DEV), pre_full=pre_full, seed=30)
    assert (pr[2][-20:] == 0).all() and bool((pr[2] != 0).any())


def test_refused_shape_is_the_two_separate_calls(ops):
    """M % 32 != 0: the weight gradient is not on the bf16 tile route, nothing is paired, not a bit changes"""
    route, sep, pr, _, _ = run_both(ops, 10420, 1, 512, expect_paired=False, seed=40)
    for a, b in zip(sep, pr):
        assert torch.equal(a, b)


def test_overlapping_dx_is_not_paired(ops):
    """dX written over X (legal for the separate calls: the weight gradient has read X by then) keeps the two launches"""
    M, nper = M1, 512
    ops.gemm_set_mode(W.BF16X6)
    assert ops.linear_bwd_route(M, 1, nper, K, nper, K, K, K)[0] == 1
    dy, x = rnd(M, nper, seed=51).to(DEV), rnd(M, K, seed=52).to(DEV)
    wflat = rnd(nper * K, seed=53, scale=0.05).to(DEV)
    ops.register_planes(wflat, ops.split_planes(wflat))
    res = []
    for pair in (False, True):
        ops.PAIR_BWD = pair
        xin = x.clone()
        dw, db = torch.empty(nper, K, device=DEV), torch.empty(nper, device=DEV)
        k0 = int(ops._L().gct_gemm_x6_kernel_launches())
        ops.linear_bwd([dy], nper, xin, [wflat.view(nper, K)], [dw], [db], xin)
        torch.cuda.synchronize()
        assert int(ops._L().gct_gemm_x6_kernel_launches()) - k0 >= 2
        res.append((dw.cpu(), db.cpu(), xin.cpu()))
    ops.unregister_planes(wflat)
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_two_plus_two_layer_model_pair_on_and_off(ops, monkeypatch):
    """A 2 + 2-layer vaetf of the full width (d = 512, dff = 2048) at 168 x 80 = 13 440 encoder rows, the smallest batch of
    whole 32-row tiles at which the planner pairs the d x d Linears: one training step with ops.PAIR_BWD off and on.
    The loss and every gradient that is not the direct output of a paired call are bit-identical (dX is, so nothing
    downstream moves); the dW / db of every linear_bwd call differ by no more than the two calls' derived bounds
    (tests/wgrad_ref.py: (drop + (t + ns) u 1.01) S per call, ns = that call's own split) allow."""
    from gct_plus_amd import engine, synthetic
    from tests.test_model_gpu import build, run_fwd_loss
    real = ops.linear_bwd
    calls = []

    def spy(dys, lddy, x2d, ws_, dws, dbs, dx, depi=0, **kw):
        real(dys, lddy, x2d, ws_, dws, dbs, dx, depi=depi, **kw)
        M, (nper, Kx) = kw.get("M") or x2d.shape[0], dws[0].shape
        wb = dbs[0] is not None
        r = ops.linear_bwd_route(M, len(dws), nper, Kx, lddy, x2d.stride(0), ws_[0].stride(0), dx.stride(0), depi, want_bias=wb)
        ns = r[1] if (ops.PAIR_BWD and r[0]) else ops.wgrad_route(M, len(dws), nper, Kx, lddy, x2d.stride(0), want_bias=wb)[1]
        D = torch.cat([d[:M, :nper].double() for d in dys], 1)
        t = int((D != 0).any(1).sum())
        S, Sb = D.abs().t() @ x2d[:M].double().abs(), D.abs().sum(0)
        calls[-1].append(dict(paired=bool(ops.PAIR_BWD and r[0] and M == x2d.shape[0]), dw=torch.cat(list(dws)).clone(),
                              db=torch.cat(list(dbs)).clone() if wb else None,
                              bw=(W.DROP[W.BF16X6] + (t + ns) * W.U * 1.01) * S, bb=(t + ns + 16) * W.U * 1.01 * Sb))

    monkeypatch.setattr(ops, "linear_bwd", spy)
    monkeypatch.setattr(ops, "DEFER_REDUCTIONS", False)         # the spy reads dW / db right after each call
    ops.gemm_set_mode(W.BF16X6)
    ds = synthetic.make_dataset(168, max_len=80, model_type="vaetf", seed=5)
    res = []
    for pair in (False, True):
        ops.PAIR_BWD = pair
        calls.append([])
        model = build("vaetf", dropout=0.1, full=True, N=2).train()
        torch.manual_seed(100)
        engine._SEED["base"] = None                            # the dropout seed counter restarts: both runs draw the same masks
        loss = run_fwd_loss(model, "vaetf", ds, 0.3)[5]
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    off, on = calls
    assert len(off) == len(on) > 0 and not any(c["paired"] for c in off)
    npaired = sum(c["paired"] for c in on)
    assert npaired >= 4, f"{npaired} of {len(on)} calls paired"
    assert torch.equal(res[0][0], res[1][0]), "loss"
    worst = 0.0
    for a, b in zip(off, on):
        if not b["paired"]:
            assert torch.equal(a["dw"], b["dw"]) and (a["db"] is None or torch.equal(a["db"], b["db"]))
            continue
        worst = max(worst, W.ratio(b["dw"].cpu(), a["dw"].cpu().double(), (a["bw"] + b["bw"]).cpu()))
        if a["db"] is not None:
            worst = max(worst, W.ratio(b["db"].cpu(), a["db"].cpu().double(), (a["bb"] + b["bb"]).cpu()))
    print(f"[bwd pair] model: {npaired} of {len(on)} linear_bwd calls paired, worst |on - off| / bound {worst:.4f}")
    assert worst <= 1.0
    outs = [(b["dw"], a["dw"]) for a, b in zip(off, on) if b["paired"]]
    outs += [(b["db"], a["db"]) for a, b in zip(off, on) if b["paired"] and b["db"] is not None]
    assert res[0][1].keys() == res[1][1].keys()
    for k, g_on in res[1][1].items():
        if torch.equal(g_on, res[0][1][k]):
            continue
        # a gradient that moved is the output of a paired call (whole, or one segment of it), already held to its bound
        flat_on, flat_off = g_on.reshape(-1), res[0][1][k].reshape(-1)
        hit = False
        for o_on, o_off in outs:
            o1, o0 = o_on.reshape(-1), o_off.reshape(-1)
            if o1.numel() % flat_on.numel():
                continue
            for sgi in range(o1.numel() // flat_on.numel()):
                sl = slice(sgi * flat_on.numel(), (sgi + 1) * flat_on.numel())
                if torch.equal(o1[sl], flat_on) and torch.equal(o0[sl], flat_off):
                    hit = True
        assert hit, f"{k} changed but is not the output of a paired call"
