"""Cross-attention K | V straight from the latent (ops.KvFold, gct_kv_fold_*) at the operator level: kvb, d(z), dW_kv,
db_kv, dW_z and db_z of the folded path against an fp64 evaluation of the UNFOLDED formulas
    e = z W_z^T + b_z,  kvb_l = e W_kv,l^T + b_kv,l,  de = sum_l dkv_l W_kv,l,  dW_kv,l = dkv_l^T e,  db_kv,l = colsum(dkv_l),
    dW_z = de^T z,  db_z = colsum(de),  dz = de W_z,
next to the unfolded path's own error (the same ops calls the engine makes with the fold off) on the same inputs.

The bound.  The fold replaces the rounded intermediate e (and de in the backward) by two rounded intermediates, A_l and
c_l (P_l and s_l in the backward): each result is still a product of two fp32 fma chains, the chains are as long in
total (d_model + latent terms), and every rounding enters the result through one further product, as e's does.  So the
fold's error is of the unfolded path's order; with the roundings of A_l and c_l both landing on one element where the
unfolded path has e's alone it can be twice that, and the maximum over the few elements of the smallest case (Mv = 4)
scatters by about as much again: the fold may exceed max(unfolded error, 2^-24 max|reference|) by FACTOR = 4.
Measured once on the MI355X (max over the cases and tensors of fold error / that floor): 1.26, db_z at 4 and 132 rows;
kvb 0.64-0.72, db_kv 1.00."""
from types import SimpleNamespace

import pytest
import torch

from gct_plus_amd import ops

pytestmark = pytest.mark.gpu
D, LAT, LAYERS = 64, 32, 2            # d_model 64: 2 d = 128 K | V outputs per layer; latent 32
FACTOR = 4.0
NAMES = ("kvb", "dz", "dW_kv", "db_kv", "dW_z", "db_z")


def _inputs(Mv, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
    return dict(z=r(Mv, LAT), wz=r(D, LAT) * LAT ** -0.5, bz=r(D) * 0.1,
                wkv=[r(2 * D, D) * D ** -0.5 for _ in range(LAYERS)], bkv=[r(2 * D) * 0.1 for _ in range(LAYERS)],
                dkv=[r(Mv, 2 * D) for _ in range(LAYERS)])


def _fp64(x):
    z, wz, bz = x["z"].double(), x["wz"].double(), x["bz"].double()
    e = z @ wz.T + bz
    kvb = [e @ w.double().T + b.double() for w, b in zip(x["wkv"], x["bkv"])]
    de = sum(dy.double() @ w.double() for dy, w in zip(x["dkv"], x["wkv"]))
    return dict(kvb=torch.stack(kvb), dz=de @ wz, dW_kv=torch.stack([dy.double().T @ e for dy in x["dkv"]]),
                db_kv=torch.stack([dy.double().sum(0) for dy in x["dkv"]]), dW_z=de.T @ z, db_z=de.sum(0))


def _modules(x):
    """k_linear / v_linear of every layer as views of one [2 d, d] buffer, and fc_z, on the device"""
    kv = []
    for w, b in zip(x["wkv"], x["bkv"]):
        w, b = w.cuda(), b.cuda()
        kv.append((SimpleNamespace(weight=w[:D], bias=b[:D]), SimpleNamespace(weight=w[D:], bias=b[D:])))
    return kv, SimpleNamespace(weight=x["wz"].cuda(), bias=x["bz"].cuda())


def _outputs(Mv):
    f = lambda *s: torch.full(s, float("nan"), device="cuda")                         # noqa: E731
    return dict(kvb=f(LAYERS, Mv, 2 * D), dz=f(Mv, LAT), dW_kv=f(LAYERS, 2 * D, D), db_kv=f(LAYERS, 2 * D),
                dW_z=f(D, LAT), db_z=f(D))


def _unfolded(x):
    Mv = x["z"].shape[0]
    kv, fc_z = _modules(x)
    z, dkv, o = x["z"].cuda(), [t.cuda() for t in x["dkv"]], _outputs(Mv)
    e, de = torch.empty(Mv, D, device="cuda"), torch.empty(Mv, D, device="cuda")
    ops.linear_fwd(z, [fc_z.weight], [fc_z.bias], [e], D)
    for l, (k, v) in enumerate(kv):
        ops.linear_fwd(e, [k.weight, v.weight], [k.bias, v.bias], [o["kvb"][l], o["kvb"][l][:, D:]], 2 * D)
    for l in range(LAYERS - 1, -1, -1):
        k, v = kv[l]
        ops.linear_bwd([dkv[l], dkv[l][:, D:]], 2 * D, e, [k.weight, v.weight], [o["dW_kv"][l][:D], o["dW_kv"][l][D:]],
                       [o["db_kv"][l][:D], o["db_kv"][l][D:]], de,
                       depi=ops.DEPI_STORE if l == LAYERS - 1 else ops.DEPI_ACCUM, M=Mv)
    ops.linear_wgrad([de], D, z, [o["dW_z"]], [o["db_z"]])
    ops.linear_dgrad([de], D, Mv, [fc_z.weight], o["dz"])
    return o


def _folded(x):
    Mv = x["z"].shape[0]
    kv, fc_z = _modules(x)
    z, dkv, o = x["z"].cuda(), [t.cuda() for t in x["dkv"]], _outputs(Mv)
    assert ops.KvFold.usable(kv, fc_z)
    fold = ops.KvFold(kv, fc_z)
    for l in range(LAYERS):
        fold.fwd(l, z, [o["kvb"][l], o["kvb"][l][:, D:]], 2 * D)
    for l in range(LAYERS - 1, -1, -1):
        fold.bwd(l, [dkv[l], dkv[l][:, D:]], 2 * D, z, o["dz"], ops.DEPI_STORE if l == LAYERS - 1 else ops.DEPI_ACCUM, Mv)
        fold.wgrad_layer(l, o["dW_kv"][l][:D], o["dW_kv"][l][D:], o["db_kv"][l][:D], o["db_kv"][l][D:])
    fold.finish(o["dW_z"], o["db_z"])
    return o, fold


@pytest.mark.parametrize("Mv", [4, 12, 132])       # one quad, a ragged count, just past one 128-row tile
def test_fold_against_fp64_and_the_unfolded_path(Mv):
    x = _inputs(Mv, 100 + Mv)
    ref = _fp64(x)
    un, (fo, fold) = _unfolded(x), _folded(x)
    torch.cuda.synchronize()
    # the folded weights themselves: A_l = W_kv,l W_z, c_l = W_kv,l b_z + b_kv,l, and the planes are an exact split of A
    wst = torch.cat(x["wkv"]).double()
    A, c = wst @ x["wz"].double(), wst @ x["bz"].double() + torch.cat(x["bkv"]).double()
    assert torch.equal(fold.wstack.cpu(), torch.cat(x["wkv"]))
    assert (fold.a.cpu().double() - A).abs().max() <= 64 * 2.0 ** -24 * A.abs().max()
    assert (fold.c.cpu().double() - c).abs().max() <= 64 * 2.0 ** -24 * c.abs().max()
    pl = (fold.a_planes.cpu().to(torch.int32) << 16).view(torch.float32).double().sum(0)
    assert torch.equal(pl.float(), fold.a.cpu().view(-1))
    worst = 0.0
    for name in NAMES:
        r = ref[name]
        eu = float((un[name].cpu().double() - r).abs().max())
        ef = float((fo[name].cpu().double() - r).abs().max())
        floor = max(eu, 2.0 ** -24 * float(r.abs().max()))
        print(f"kv_fold Mv={Mv} {name}: unfolded err {eu:.3e} folded err {ef:.3e} ratio to floor {ef / floor:.2f} "
              f"(max|ref| {float(r.abs().max()):.3e})")
        worst = max(worst, ef / floor)
        assert ef == ef and ef <= FACTOR * floor, (name, Mv, ef, eu, floor)
    print(f"kv_fold Mv={Mv}: worst ratio {worst:.2f}")


def test_fold_without_dz_is_the_weight_gradient_alone():
    """need_dz false: KvFold.bwd runs the weight gradient only; P_l and s_l (hence every gradient) are the same bits
    as with the paired call's, up to the slab split -- compared at the fold's own bound."""
    x = _inputs(12, 7)
    ref = _fp64(x)
    kv, fc_z = _modules(x)
    z, dkv, o = x["z"].cuda(), [t.cuda() for t in x["dkv"]], _outputs(12)
    fold = ops.KvFold(kv, fc_z)
    for l in range(LAYERS - 1, -1, -1):
        fold.bwd(l, [dkv[l], dkv[l][:, D:]], 2 * D, z, None, ops.DEPI_STORE, 12)
        fold.wgrad_layer(l, o["dW_kv"][l][:D], o["dW_kv"][l][D:], o["db_kv"][l][:D], o["db_kv"][l][D:])
    fold.finish(o["dW_z"], o["db_z"])
    un = _unfolded(x)
    for name in ("dW_kv", "db_kv", "dW_z", "db_z"):
        r = ref[name]
        eu = float((un[name].cpu().double() - r).abs().max())
        ef = float((o[name].cpu().double() - r).abs().max())
        assert ef <= FACTOR * max(eu, 2.0 ** -24 * float(r.abs().max())), (name, ef, eu)
