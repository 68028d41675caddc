"""gct_kld_dims_fwd / gct_kld_dims_bwd / gct_latent_moments (csrc/vae.hip) against the fp64 restatement of their rule
in tests/kl_ref.py.

Shapes (B, Le, D): one row; a few rows at the smallest D; rows below, at and not a multiple of the rows a workgroup
covers per pass (8 at D = 128); D = 1024 (one row per pass); D = 12 (3 lanes per row: 85 rows per pass, one idle
thread); (6, 37, 128) -- 222 rows = 28 passes -> 7 workgroups by the grid rule, the last pass ragged; and (64, 300,
128) -- 19200 rows = 2400 passes, past the 512-workgroup cap, so workgroups loop.

Bounds.  kl_dim: |err_j| <= 0.5 * N_live * 8 * 2^-24 * max_r (1 + |l| + m^2 + e^l): the five fp32 operations of
t = 1 + l - m*m - expf(l) (expf at 2 ulp) on terms of at most that size; the fp64 sum adds nothing visible.  out[0],
out[1]: the sum of those plus one fp32 rounding of the result.  Gates and counts are exact, which needs every
K_j / floor away from 1: the inputs are asserted to keep it outside [0.95, 1.05]."""
import functools
import math

import numpy as np
import pytest
import torch

from gct_plus_amd._lib import GctError
from tests import kl_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAMBDA = 0.25
U32 = 2.0 ** -24
SHAPES = [(1, 1, 4), (2, 3, 4), (3, 3, 128), (5, 9, 128), (7, 37, 64), (2, 5, 1024), (4, 11, 12), (6, 37, 128),
          (64, 300, 128)]
MASKS = ["none", "random", "one_dead", "all_dead"]


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


@functools.lru_cache(maxsize=None)
def case(shape, mask):
    """(mu, lv, live) numpy, the fp64 reference at LAMBDA and the per-dimension bound: computed once per case."""
    B, Le, D = shape
    mu, lv = kl_ref.latent_inputs(B, Le, D, seed=B * 1000 + Le * 10 + D)
    live = kl_ref.live_masks(B, Le, seed=B + Le + D)[mask]
    ref = kl_ref.kl_dims(mu, lv, live, LAMBDA, B)
    for a in (mu, lv) + ((live,) if live is not None else ()):
        a.setflags(write=False)
    return mu, lv, live, ref, kl_ref.kl_dim_bound(mu, lv, live)


def to_dev(mu, lv, live):
    return (torch.tensor(mu, device=DEV), torch.tensor(lv, device=DEV),
            None if live is None else torch.tensor(live, device=DEV))


def check_forward(out, kl_dim, gate, ref, bound, what):
    out, kl_dim, gate = out.cpu().double().numpy(), kl_dim.cpu().double().numpy(), gate.cpu().numpy()
    err = np.abs(kl_dim - ref["kl_dim"])
    tol = bound + U32 * np.abs(ref["kl_dim"])                   # + the rounding of K_j to fp32
    print(f"{what}: kl_dim worst error / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
    assert (err <= tol).all(), (what, float(err.max()))
    assert np.array_equal(gate, ref["gate"].astype(np.float32)), what
    assert out[2] == ref["n_floor"] and out[3] == ref["live_rows"], (what, out)
    gated = bound[ref["gate"]].sum()                            # a dimension on the floor contributes the exact floor
    for k, key, b in ((0, "objective", gated), (1, "raw", bound.sum())):
        tol_k = b + U32 * abs(ref[key])
        print(f"{what}: {key} {out[k]!r} vs {ref[key]!r}, error / bound {abs(out[k] - ref[key]) / max(tol_k, 1e-300):.3f}")
        assert abs(out[k] - ref[key]) <= tol_k, (what, key, out[k], ref[key])


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_backward(ops, shape, mask):
    mu, lv, live, ref, bound = case(shape, mask)
    B, Le, D = shape
    ratio = ref["kl_dim"] / ref["floor"]
    assert not ((ratio >= 0.95) & (ratio <= 1.05)).any(), f"inputs too close to the floor: {ratio}"
    m, l, lvm = to_dev(mu, lv, live)
    out, kl_dim, gate = ops.kld_dims_fwd(m, l, lvm, LAMBDA, B)
    check_forward(out, kl_dim, gate, ref, bound, f"{shape} {mask}")
    out2, kl2, gate2 = ops.kld_dims_fwd(m, l, lvm, LAMBDA, B)
    assert torch.equal(out, out2) and torch.equal(kl_dim, kl2) and torch.equal(gate, gate2), "two runs differ"
    if mask == "all_dead":
        assert out[0].item() == np.float32(D * ref["floor"]) and out[1].item() == 0 and not gate.any()

    # backward: exact zeros at closed gates and dead rows, kld_bwd's bits everywhere else
    g = torch.tensor(0.37, device=DEV)
    dmu, dlv = ops.kld_dims_bwd(m, l, lvm, gate, g)
    rmu, rlv = ops.kld_bwd(m, l, g)
    keep = torch.ones(B * Le, dtype=torch.bool, device=DEV) if lvm is None else lvm.view(-1)
    open_ = (keep[:, None] & (gate != 0)[None, :]).view(B, Le, D)
    assert (dmu[~open_] == 0).all() and (dlv[~open_] == 0).all()
    assert not torch.signbit(dmu[~open_]).any() and not torch.signbit(dlv[~open_]).any()
    assert torch.equal(dmu[open_], rmu[open_]) and torch.equal(dlv[open_], rlv[open_])
    # ... and the fp64 gradient of the rule (fp32 products: 4 ulp covers expf, the difference and the two products)
    gmu, glv = kl_ref.kl_dims_grad(mu, lv, live, LAMBDA, B)
    gmu, glv = 0.37 * gmu.reshape(shape), 0.37 * glv.reshape(shape)
    assert np.all(np.abs(dmu.cpu().double().numpy() - gmu) <= 4 * U32 * np.abs(gmu) + 1e-30)
    e = np.exp(lv.astype(np.float64))
    assert np.all(np.abs(dlv.cpu().double().numpy() - glv) <= 0.37 * 0.5 * 8 * U32 * (e + 1.0))


@pytest.mark.parametrize("shape", [(3, 3, 128), (4, 11, 12), (6, 37, 128)], ids=lambda s: "x".join(map(str, s)))
def test_lambda_zero_and_huge(ops, shape):
    mu, lv, live, _, bound = case(shape, "none")
    B, Le, D = shape
    m, l, _ = to_dev(mu, lv, None)
    out, kl_dim, gate = ops.kld_dims_fwd(m, l, None, 0.0, B)
    assert (gate == 1).all() and out[2].item() == 0
    assert out[0].item() == out[1].item(), "free_bits 0: objective and raw must be the same bits"
    dmu, dlv = ops.kld_dims_bwd(m, l, None, gate, torch.tensor(1.0, device=DEV))
    rmu, rlv = ops.kld_bwd(m, l, torch.tensor(1.0, device=DEV))
    assert torch.equal(dmu, rmu) and torch.equal(dlv, rlv)

    # the anchor: gct_kld_fwd sums the same fp32 terms in fp32.  A term passes through at most
    # depth = ceil(n / (256 g)) + 8 + ceil(g / 256) + 8 additions (a thread's run, the 256-lane tree, twice: g =
    # min(1024, ceil(n / 256)) workgroups, then one), each with a relative error of 2^-24, so it is within
    # depth * 2^-24 * 0.5 * sum |t| of the exact sum of its own terms; both kernels' terms are within `bound` of fp64.
    n = mu.size
    g_old = min(1024, -(-n // 256))
    depth = -(-n // (256 * g_old)) + 8 + -(-g_old // 256) + 8
    mag = (1.0 + np.abs(lv.astype(np.float64)) + mu.astype(np.float64) ** 2 + np.exp(lv.astype(np.float64))).sum()
    old = ops.kld_fwd(m, l).item()
    tol = 1.01 * depth * U32 * 0.5 * mag + 2 * bound.sum() + 2 * U32 * abs(old)
    print(f"{shape}: kld_fwd {old!r}, raw {out[1].item()!r}, difference / bound {abs(old - out[1].item()) / tol:.4f}")
    assert abs(old - out[1].item()) <= tol

    huge = 1e30
    out, kl_dim, gate = ops.kld_dims_fwd(m, l, None, huge, B)
    assert (gate == 0).all() and out[2].item() == D
    assert out[0].item() == np.float32(D * (float(np.float32(huge)) * B))
    dmu, dlv = ops.kld_dims_bwd(m, l, None, gate, torch.tensor(1.0, device=DEV))
    assert (dmu == 0).all() and (dlv == 0).all()


def test_no_rows(ops):
    m = torch.empty(0, 5, 8, device=DEV)
    out, kl_dim, gate = ops.kld_dims_fwd(m, m.clone(), None, LAMBDA, 3)
    assert out.tolist() == [8 * 0.75, 0.0, 8.0, 0.0] and (kl_dim == 0).all() and (gate == 0).all()
    dmu, dlv = ops.kld_dims_bwd(m, m.clone(), None, gate, torch.tensor(1.0, device=DEV))
    assert dmu.shape == m.shape and dlv.shape == m.shape


def test_live_shapes(ops):
    """live as [B, Le], [B, 1, Le], [R], bool or uint8: one result."""
    mu, lv, live, _, _ = case((5, 9, 128), "random")
    m, l, lvm = to_dev(mu, lv, live)
    want = ops.kld_dims_fwd(m, l, lvm, LAMBDA, 5)
    for form in (lvm.unsqueeze(1), lvm.view(-1), lvm.to(torch.uint8), lvm.to(torch.uint8).view(-1)):
        got = ops.kld_dims_fwd(m, l, form, LAMBDA, 5)
        assert all(torch.equal(a, b) for a, b in zip(want, got))


def test_limits(ops):
    """Everything outside the limits raises GctError before a launch: the outputs of the raw calls stay NaN."""
    ok = torch.zeros(2, 3, 8, device=DEV)
    gate, g = torch.ones(8, device=DEV), torch.ones((), device=DEV)
    acc = ops.latent_moments_state(8, DEV)
    for D in (2, 6, 1028):
        bad = torch.zeros(2, 3, D, device=DEV)
        with pytest.raises(GctError):
            ops.kld_dims_fwd(bad, bad, None, LAMBDA, 2)
        with pytest.raises(GctError):
            ops.kld_dims_bwd(bad, bad, None, torch.ones(D, device=DEV), g)
        with pytest.raises(GctError):
            ops.latent_moments(bad, bad, None, ops.latent_moments_state(D, DEV))
    for fb in (-0.1, float("nan"), float("inf"), 1e39):
        with pytest.raises(GctError):
            ops.kld_dims_fwd(ok, ok, None, fb, 2)
    for n_mol in (0, -1):
        with pytest.raises(GctError):
            ops.kld_dims_fwd(ok, ok, None, LAMBDA, n_mol)
    off = torch.zeros(2 * 3 * 8 + 1, device=DEV)[1:].view(2, 3, 8)                   # contiguous, 4-B aligned only
    wrong = [(ok.double(), ok, None), (ok, ok[:, :, :4], None), (ok.transpose(0, 1), ok.transpose(0, 1), None),
             (off, ok, None), (ok, off, None), (ok, ok, torch.ones(2, 4, dtype=torch.bool, device=DEV)),
             (ok, ok, torch.ones(2, 3, device=DEV)), (ok, ok, torch.ones(2, 3, dtype=torch.bool))]
    for mu, lv, live in wrong:
        with pytest.raises(GctError):
            ops.kld_dims_fwd(mu, lv, live, LAMBDA, 2)
        with pytest.raises(GctError):
            ops.kld_dims_bwd(mu, lv, live, gate, g)
        with pytest.raises(GctError):
            ops.latent_moments(mu, lv, live, acc)
    with pytest.raises(GctError):
        ops.kld_dims_bwd(ok, ok, None, torch.ones(4, device=DEV), g)
    with pytest.raises(GctError):
        ops.latent_moments(ok, ok, None, acc.float())
    assert (acc == 0).all()
    # the library's own checks, past the Python layer
    L, nan = ops._L(), float("nan")
    out, kd, gt = (torch.full((n,), nan, device=DEV) for n in (4, 8, 8))
    ws = ops.workspace(L.gct_kld_dims_ws_bytes(8), ok.device)
    p = lambda t: t.data_ptr()
    assert L.gct_kld_dims_ws_bytes(6) == 0 and L.gct_kld_dims_ws_bytes(8) > 0
    for R, D, fb, n_mol, mu in ((-1, 8, 0.25, 2, ok), (6, 6, 0.25, 2, ok), (6, 8, -1.0, 2, ok), (6, 8, nan, 2, ok),
                                (6, 8, float("inf"), 2, ok), (6, 8, 0.25, 0, ok), (6, 8, 0.25, 2, off)):
        assert L.gct_kld_dims_fwd(p(mu), p(ok), None, R, D, fb, n_mol, p(out), p(kd), p(gt), p(ws), ops._st()) == -1
    dm, dl = torch.full_like(ok, nan), torch.full_like(ok, nan)
    assert L.gct_kld_dims_bwd(p(ok), p(ok), None, p(gate), p(g), p(dm), p(dl), -1, 8, ops._st()) == -1
    assert L.gct_kld_dims_bwd(p(ok), p(ok), None, p(gate), p(g), p(dm), p(dl), 6, 10, ops._st()) == -1
    assert L.gct_latent_moments(p(ok), p(ok), None, -1, 8, p(acc), p(ws), ops._st()) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (out, kd, gt, dm, dl)) and (acc == 0).all()


def test_latent_moments(ops):
    """Three batches of different Le into one state, against kl_ref.moments.  sum mu, sum mu^2 and sum lv are fp64
    sums of exactly converted values (mu^2: an exact fp64 product), so only the order of the fp64 additions differs:
    1e-12 of the sum of magnitudes.  sum exp(lv) carries expf's 2 ulp and its fp32 rounding; the KL row the bound of
    kl_dim, batch by batch."""
    D = 64
    batches = []
    for B, Le, seed in ((3, 7, 1), (5, 21, 2), (2, 40, 3)):
        mu, lv = kl_ref.latent_inputs(B, Le, D, seed)
        batches.append((mu, lv, kl_ref.live_masks(B, Le, seed)["random"]))
    ref = kl_ref.moments(batches)
    states = []
    for _ in range(2):
        acc = ops.latent_moments_state(D, DEV)
        for mu, lv, live in batches:
            ops.latent_moments(*to_dev(mu, lv, live), acc)
        states.append(acc)
    assert torch.equal(states[0], states[1]), "two accumulations of the same batches differ"
    got = states[0].cpu().numpy()
    cat = lambda k: np.concatenate([b[k].reshape(-1, D)[b[2].reshape(-1)] for b in batches]).astype(np.float64)
    m, l = cat(0), cat(1)
    assert np.all(np.abs(got[0] - ref[0]) <= 1e-12 * np.abs(m).sum(0))
    assert np.all(np.abs(got[1] - ref[1]) <= 1e-12 * (m * m).sum(0))
    assert np.all(np.abs(got[2] - ref[2]) <= 4 * U32 * np.exp(l).sum(0))
    assert np.all(np.abs(got[3] - ref[3]) <= 1e-12 * np.abs(l).sum(0))
    assert np.all(np.abs(got[4] - ref[4]) <= sum(kl_ref.kl_dim_bound(*b) for b in batches))
    assert np.array_equal(got[5], ref[5]) and got[5, 0] == sum(int(b[2].sum()) for b in batches)
    # no mask, and a state that already holds something: the call adds
    acc = states[0].clone()
    mu, lv, _ = batches[0]
    ops.latent_moments(*to_dev(mu, lv, None), acc)
    one = kl_ref.moments([(mu, lv, None)])
    assert np.all(np.abs(acc.cpu().numpy()[[0, 5]] - (got + one)[[0, 5]]) <= 1e-12 * (np.abs(m).sum(0) + 1))
