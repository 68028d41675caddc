"""Latents for molecule interpolation on the device: gct_latent_stats / gct_latent_interp (csrc/latent.hip) against the
host reference tests/latent_ref.py, and Sampling.interpolate_smiles / reconstruct_smiles end to end on tiny models of
all four types against that reference and the un-cached reference-style decode."""
import functools

import numpy as np
import pytest
import torch

from gct_plus_amd import data, synthetic
from tests import latent_ref as LR

pytestmark = pytest.mark.gpu
TINY = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
EOS, PAD, SOS = synthetic.EOS_ID, synthetic.PAD_ID, synthetic.SOS_ID


# ------------------------------------------------------------------------------------------------ latent_stats
@functools.lru_cache(maxsize=None)
def stats_case(n, Le, D, rows):
    g = np.random.default_rng(n * 1000 + D)
    mu = g.normal(0.3, 1.0, (n, Le, D)).astype(np.float32)
    lv = g.normal(0.3, 1.0, (n, Le, D)).astype(np.float32)
    return mu, lv, LR.stats_ref(mu, lv, rows)


@pytest.mark.parametrize("n,Le,D,rows", [(3, 5, 6, (1, 2, 5)), (2, 200, 128, (200, 67)), (1, 70, 1024, (65,))])
def test_latent_stats_vs_reference(n, Le, D, rows):
    from gct_plus_amd import ops
    mu, lv, want = stats_case(n, Le, D, rows)
    got = ops.latent_stats(torch.from_numpy(mu).cuda(), torch.from_numpy(lv).cuda(), list(rows))
    assert got.shape == (n, 4, D) and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"latent_stats {n}x{Le}x{D}: worst error over tolerance {float((err / (1e-5 + 1e-5 * np.abs(want))).max()):.3f}")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(want))                           # test_kernels_gpu.test_norm's forward tolerance
    for i, r in enumerate(rows):
        if r == 1:                                                              # one row: the mean is the row, std exactly 0
            assert torch.equal(got[i, 0].cpu(), torch.from_numpy(mu[i, 0])) and not got[i, 1].any() and not got[i, 3].any()
    # rows at or beyond rows[i] are never read: poison them
    mu2, lv2 = mu.copy(), lv.copy()
    for i, r in enumerate(rows):
        mu2[i, r:] = np.nan
        lv2[i, r:] = np.nan
    again = ops.latent_stats(torch.from_numpy(mu2).cuda(), torch.from_numpy(lv2).cuda(), torch.tensor(rows))
    assert torch.equal(again, got)
    assert torch.equal(ops.latent_stats(torch.from_numpy(mu).cuda(), torch.from_numpy(lv).cuda(), list(rows)), got)


def test_latent_stats_argument_errors():
    from gct_plus_amd import ops
    from gct_plus_amd._lib import GctError
    x = torch.zeros(2, 5, 8, device="cuda")
    for bad in ([0, 3], [6, 3]):
        with pytest.raises(GctError):
            ops.latent_stats(x, x, bad)
    with pytest.raises(ValueError):
        ops.latent_stats(x, x, [3])
    with pytest.raises(GctError):
        ops.latent_stats(torch.zeros(1, 2, 1025, device="cuda"), torch.zeros(1, 2, 1025, device="cuda"), [2])
    with pytest.raises(GctError):
        ops.latent_stats(torch.zeros(1, 2, 0, device="cuda"), torch.zeros(1, 2, 0, device="cuda"), [2])


# ----------------------------------------------------------------------------------------------- latent_interp
R7 = dict(a=(0, 1, 2, 3, 0, 1, 2), b=(1, 2, 3, 0, 2, 3, 0), lens=(0, 1, 3, 64, 65, 66, 66),
          items=(5, 0, 17, 123456, 7, 2 ** 31 - 1, 99))
T7 = 66
# Philox seeds under which every slerp of the comparison is well conditioned (|c| <= 0.95) in the reference; found on
# the CPU with the reference alone, and asserted below
SEEDS = {6: (7 << 32) | 1, 128: (7 << 32) | 1}


def random_stats(D, n=4, seed=0):
    g = np.random.default_rng(100 + D + seed)
    return np.stack([g.normal(0, 0.5, (n, D)), g.uniform(0.5, 1.5, (n, D)), g.normal(0, 0.5, (n, D)),
                     g.uniform(0.5, 1.5, (n, D))], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def interp_case(D, noise, alpha):
    stats = random_stats(D)
    z, tol, c, sl = LR.interp_tolerance(stats, R7["a"], R7["b"], [alpha] * 7, [noise] * 7, R7["lens"], R7["items"], T7,
                                        SEEDS[D])
    return stats, z, tol, c, sl


def run_interp(stats, a, b, alpha, noise, lens, items, T, seed):
    from gct_plus_amd import ops
    R = len(a)
    al = alpha if isinstance(alpha, (list, tuple)) else [alpha] * R
    ns = noise if isinstance(noise, (list, tuple)) else [noise] * R
    st = stats if isinstance(stats, torch.Tensor) else torch.from_numpy(stats).cuda()
    return ops.latent_interp(st, list(a), list(b), al, ns, list(lens), list(items), T, seed)


@pytest.mark.parametrize("alpha", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("noise", [0.0, 0.3])
@pytest.mark.parametrize("D", [6, 128])
def test_latent_interp_vs_reference(D, noise, alpha):
    stats, want, tol, c, sl = interp_case(D, noise, alpha)
    assert LR.well_conditioned(c, sl), "pick another seed: a slerp of the comparison has |c| > 0.95"
    assert sl[:, :, 0].sum() == sum(R7["lens"]) and sl[:, :, 1].sum() == (sum(R7["lens"]) if noise else 0)
    got = run_interp(stats, R7["a"], R7["b"], alpha, noise, R7["lens"], R7["items"], T7, SEEDS[D])
    assert got.shape == (7, T7, D)
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"latent_interp D={D} noise={noise} alpha={alpha}: worst error over tolerance {float((err / tol).max()):.3f} "
          f"(tolerance {float(tol.min()):.2e} .. {float(tol.max()):.2e})")
    assert np.all(err <= tol)
    for r, L in enumerate(R7["lens"]):                                         # exact zeros behind the row's length
        assert not got[r, L:].any() and np.all(np.signbit(got[r, L:]) == 0)
        assert np.all(got[r, :L] != 0)


@pytest.mark.parametrize("D", [6, 128])
def test_noise_free_rows_are_exactly_m(D):
    """noise_std == 0: the row is m, whatever the log_var statistics (which enter l and nothing else) -- bit for bit,
    under two seeds; and it is the m of the noisy row, which differs from it by the noise term alone."""
    stats = random_stats(D)
    other = stats.copy()
    other[:, 2:] = random_stats(D, seed=1)[:, 2:] * 3 + 1
    for seed in (SEEDS[D], 12345):
        base = run_interp(stats, R7["a"], R7["b"], 0.5, 0.0, R7["lens"], R7["items"], T7, seed)
        assert torch.equal(base, run_interp(other, R7["a"], R7["b"], 0.5, 0.0, R7["lens"], R7["items"], T7, seed))
        mixed = run_interp(stats, R7["a"], R7["b"], 0.5, [0.0, 0.3, 0.0, 0.3, 0.0, 0.3, 0.0], R7["lens"], R7["items"], T7,
                           seed)
        assert torch.equal(mixed[0::2], base[0::2])                            # a row's noise is its own
        assert not torch.equal(mixed[3], base[3]) and not torch.equal(mixed[5], base[5])
        if seed == SEEDS[D]:                                                    # (the tight comparison is the test above)
            want = LR.interp_ref(stats, R7["a"], R7["b"], [0.5] * 7, [0.0] * 7, R7["lens"], R7["items"], T7, seed)[0]
            assert np.allclose(base.cpu().numpy(), want, rtol=1e-4, atol=1e-4)
    assert not torch.equal(run_interp(stats, R7["a"], R7["b"], 0.5, 0.0, R7["lens"], R7["items"], T7, 12345),
                           run_interp(stats, R7["a"], R7["b"], 0.5, 0.0, R7["lens"], R7["items"], T7, 12346))


@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_guard_returns_u_exactly(noise):
    """Statistics of one-row molecules (std 0) and a == b: u == v == the mean, c rounds to 1, the guard's lerp returns
    u exactly; with noise the row is mean_mu + noise n_4 exp(mean_log_var / 2)."""
    from gct_plus_amd import ops
    g = torch.Generator().manual_seed(3)
    D, n = 24, 3
    mu, lv = torch.randn(n, 4, D, generator=g).cuda(), torch.randn(n, 4, D, generator=g).cuda()
    stats = ops.latent_stats(mu, lv, [1, 1, 1])
    assert not stats[:, 1].any() and not stats[:, 3].any()
    lens, items = [5, 2, 4], [3, 4, 5]
    for alpha in (0.1, 0.5, 0.9):
        z = run_interp(stats, [0, 1, 2], [0, 1, 2], alpha, noise, lens, items, 5, 77)
        want, c, sl = LR.interp_ref(stats.cpu().numpy(), [0, 1, 2], [0, 1, 2], [alpha] * 3, [noise] * 3, lens, items, 5, 77)
        assert not sl.any()                                                     # the reference takes the guard everywhere
        for r, L in enumerate(lens):
            if noise == 0:
                assert torch.equal(z[r, :L], mu[r, 0].expand(L, D))
            else:
                assert np.allclose(z[r, :L].cpu().numpy(), want[r, :L], rtol=1e-5, atol=1e-5)
            assert not z[r, L:].any()
    # a zero endpoint is the guard too: |u| == 0 gives alpha v
    zero = stats.clone()
    zero[0] = 0
    z = run_interp(zero, [0], [1], 0.25, 0.0, [3], [9], 3, 77)
    assert torch.equal(z[0], (0.25 * (mu[1, 0] - 0.0)).expand(3, D))


def test_batch_independence():
    """A row is a function of (seed, item, a, b, alpha, noise_std, len): computed alone with T = its own length it
    equals its slice of the 7-row call bit for bit; another item gives another row."""
    for D in (6, 128):
        stats = random_stats(D)
        alphas, noise = [0.1, 0.5, 0.9, 0.3, 0.7, 0.2, 0.6], [0.0, 0.3, 0.1, 0.0, 0.3, 0.2, 0.0]
        full = run_interp(stats, R7["a"], R7["b"], alphas, noise, R7["lens"], R7["items"], T7, SEEDS[D])
        for r, L in enumerate(R7["lens"]):
            if L == 0:
                continue                                                        # nothing to compute: T >= 1
            one = run_interp(stats, [R7["a"][r]], [R7["b"][r]], [alphas[r]], [noise[r]], [L], [R7["items"][r]], L, SEEDS[D])
            assert one.shape == (1, L, D) and torch.equal(one[0], full[r, :L]), (D, r)
        moved = run_interp(stats, R7["a"][::-1], R7["b"][::-1], alphas[::-1], noise[::-1], R7["lens"][::-1],
                           R7["items"][::-1], T7 + 3, SEEDS[D])
        assert torch.equal(moved.flip(0)[:, :T7], full) and not moved[:, T7:].any()
        items = list(R7["items"])
        items[3] += 1
        diff = run_interp(stats, R7["a"], R7["b"], alphas, noise, R7["lens"], items, T7, SEEDS[D])
        assert not torch.equal(diff[3], full[3]) and torch.equal(diff[[0, 1, 2, 4, 5, 6]], full[[0, 1, 2, 4, 5, 6]])
    from gct_plus_amd import ops
    assert ops.latent_interp(torch.from_numpy(random_stats(6)).cuda(), [], [], [], [], [], [], 4, 1).shape == (0, 4, 6)


def test_latent_interp_argument_errors():
    from gct_plus_amd._lib import GctError
    ok = dict(a=[0, 1], b=[1, 0], alpha=0.5, noise=0.1, lens=[2, 3], items=[0, 1], T=3, seed=1)

    def call(stats, **kw):
        k = dict(ok, **kw)
        return run_interp(stats, k["a"], k["b"], k["alpha"], k["noise"], k["lens"], k["items"], k["T"], k["seed"])
    good = torch.from_numpy(random_stats(8, n=2)).cuda()
    assert call(good).shape == (2, 3, 8)
    for D in (0, 1025):
        with pytest.raises(GctError):
            call(torch.zeros(2, 4, D, device="cuda"))
    for bad in (dict(lens=[2, 4]), dict(lens=[-1, 3]), dict(a=[0, 2]), dict(b=[-1, 0]), dict(items=[0, -1]),
                dict(T=0, lens=[0, 0])):
        with pytest.raises(GctError):
            call(good, **bad)
    with pytest.raises(ValueError):
        call(good, lens=[2])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- end to end
SCAFFOLD = "c1ccccc1"
MTYPES = [("VaetfSampling", "vaetf"), ("CvaetfSampling", "pvaetf"), ("ScaVaeSampling", "scavaetf"),
          ("PscavaetfSampling", "pscavaetf")]


def make_sampler(cls_name, mtype, decode_algo="greedy", **kw):
    from gct_plus_amd.Inference import sampling_tool
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    strs = [SCAFFOLD + "<sep>" + s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    nc = synthetic.n_conds(mtype)
    torch.manual_seed(4)
    model = model_dict[mtype](len(SRC), len(TRG), dropout=0.1, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
    # seed 12 (the latents' seed): every slerp of the end-to-end comparison has |c| <= 0.95 for all four model types,
    # found on the CPU with the oracle's encoder and the reference alone; the test asserts it
    return getattr(sampling_tool, cls_name)(model, SRC, TRG, latent_dim=16, max_strlen=24, cond_dim=nc,
                                            decode_algo=decode_algo, toklen_data=[12, 14, 15, 18, 20, 16], seed=12, **kw)


def pairs_for(sp, P=3):
    """P pairs of molecules of different lengths with the arguments the sampler's type takes."""
    from tests.test_data_pipeline import SMILES
    src0, src1 = SMILES[0:P], SMILES[7:7 + P]
    kw = {}
    if sp.uses_scaffold:
        kw.update(scaffolds0=["c1ccccc1", "CC", "C1CCNCC1"][:P], scaffolds1=["CC", "c1ccccc1", "CC"][:P])
    if sp.uses_props:
        g = np.random.default_rng(8)
        kw.update(props0=g.uniform(0, 1, (P, sp.cond_dim)), props1=g.uniform(0, 1, (P, sp.cond_dim)), transform=False)
    return src0, src1, kw


def endpoint_stats_alone(sp, src0, src1, kw):
    """fp64 statistics of every endpoint encoded ALONE (one encode_smiles per molecule), and its latent rows."""
    P = len(src0)
    stats, lens = [], []
    for j, s in enumerate(src0 + src1):
        side, p = ("0", j) if j < P else ("1", j - P)
        args = [[s]] + ([[kw["scaffolds" + side][p]]] if sp.uses_scaffold else []) + \
            ([kw["props" + side][p:p + 1]] if sp.uses_props else [])
        _, mu, lv = sp.encode_smiles(*args, **({"transform": False} if sp.uses_props else {}))
        lens.append(mu.shape[1])
        stats.append(LR.stats_ref(mu.cpu().numpy(), lv.cpu().numpy(), [mu.shape[1]])[0])
    return np.stack(stats), np.asarray(lens)


def upto_eos(ids):
    ids = [int(t) for t in ids]
    return ids[:ids.index(EOS) + 1] if EOS in ids else ids


LADDER = [0.0, 0.0, 0.05, 0.05, 0.1, 0.1, 0.2, 0.2]
# the encoder's rows in a batch against the same molecule alone: the batch-vs-alone bound of
# test_mixed_scaffold_decode_gpu.py (atol 1e-6), added to the latents' tolerance
ENCODER_TOL = 1e-6


@pytest.mark.parametrize("cls_name,mtype", MTYPES)
@torch.no_grad()
def test_interpolate_smiles_end_to_end(cls_name, mtype):
    from gct_plus_amd.decode import reference_style_decode
    from gct_plus_amd.Inference.mol_interpolation import interior_alphas, interp_plan
    sp = make_sampler(cls_name, mtype)
    P, A, K = 3, 3, len(LADDER)
    src0, src1, kw = pairs_for(sp, P)
    res, rounds = sp.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=4, accept=lambda s: False, return_rows=True,
                                        **kw)
    assert res.rows_decoded == P * A * K and len(rounds) == 2 and (res.tries == -1).all()
    assert all(s is None for row in res.smiles for s in row) and np.isnan(res.noise_std).all()
    # 1. the latents of every row against the reference fed with the endpoints encoded alone
    stats, lens = endpoint_stats_alone(sp, src0, src1, kw)
    alphas = interior_alphas(A)
    extras = [len(sp.smi_to_id(s)) + 1 for s in kw["scaffolds0"]] if sp.uses_scaffold else None
    toklen = interp_plan(lens[:P], lens[P:], alphas, extras)
    assert np.array_equal(res.toklen, toklen) and len({int(t) for t in toklen.reshape(-1)}) > 1
    worst = 0.0
    for j, rows in enumerate(rounds):
        p, i, k = (x.reshape(-1) for x in np.meshgrid(np.arange(P), np.arange(A), np.arange(4 * j, 4 * j + 4), indexing="ij"))
        tl, T = toklen[p, i], int(toklen.max())
        items = (p * A + i) * K + k
        want, tol, c, sl = LR.interp_tolerance(stats.astype(np.float32), p, p + P, alphas[i], np.asarray(LADDER)[k], tl,
                                               items, T, sp.latent_seed)
        assert LR.well_conditioned(c, sl)
        assert rows.zs.shape == (P * A * 4, T, 16)
        assert torch.equal(rows.src_mask.cpu().view(len(p), T), torch.arange(T)[None, :] < torch.as_tensor(tl)[:, None])
        err = np.abs(rows.zs.cpu().numpy().astype(np.float64) - want)
        tol = tol + ENCODER_TOL
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (j, float((err / tol).max()))
        # 2. the token rows against the un-cached loop on the same latents, prefix length by prefix length
        lens_r = rows.prefix_lens
        G = rows.ys.shape[1] - int(lens_r.max())                                # row r's tokens: ys[r, t0_r : t0_r + G]
        for t0 in torch.unique(lens_r).tolist():
            idx = (lens_r == t0).nonzero().view(-1)
            dc = None if rows.dconds is None else rows.dconds[idx.cuda()]
            ref = reference_style_decode(sp.model, rows.zs[idx.cuda()], rows.src_mask[idx.cuda()], dc,
                                         rows.ys[idx.cuda(), :t0], PAD, EOS, sp.max_strlen).cpu()
            for jj, r in enumerate(idx.tolist()):
                a, b = upto_eos(rows.ys[r, t0:t0 + G].cpu()), upto_eos(ref[jj, t0:])
                if a != b:                                                      # only at an fp32 near-tie (the tie guard of
                    t = next(q for q, (x, y) in enumerate(zip(a + [None], b + [None])) if x != y)    # the mixed-scaffold tests)
                    ys = ref[jj:jj + 1, :t0 + t].cuda()
                    from gct_plus_amd.Model.modules import get_trg_mask
                    d1 = None if dc is None else dc[jj:jj + 1]
                    lg = sp.model.decode(ys, rows.zs[r:r + 1], rows.src_mask[r:r + 1], get_trg_mask(ys, PAD, False, d1),
                                         d1)[0, -1]
                    top2 = lg.topk(2).values
                    assert float(top2[0] - top2[1]) < 1e-4, (r, t0, t, a, b)
        if sp.uses_props:
            want_c = kw["props0"][p] * (1 - alphas[i])[:, None] + kw["props1"][p] * alphas[i][:, None]
            assert np.allclose(rows.dconds.cpu().numpy(), want_c, rtol=1e-6, atol=1e-6)
    print(f"interpolate_smiles {mtype}: worst latent error over tolerance {worst:.3f}")


@pytest.mark.parametrize("cls_name,mtype", MTYPES)
@torch.no_grad()
def test_interpolate_smiles_options(cls_name, mtype):
    from gct_plus_amd.smiles import SmilesGrammar
    P, A = 3, 3
    sp = make_sampler(cls_name, mtype)
    src0, src1, kw = pairs_for(sp, P)
    base = sp.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=4, **kw)
    assert np.array_equal(base.noise_std[base.tries >= 0], np.asarray(LADDER)[base.tries[base.tries >= 0]])
    for p in range(P):
        for i in range(A):
            assert (base.smiles[p][i] is None) == (base.tries[p, i] < 0) and base.smiles[p][i] != ""
    # chunking and continuous batching change nothing
    assert sp.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=16, **kw).smiles == base.smiles
    st = make_sampler(cls_name, mtype, stream_rows=8)
    got = st.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=4, **kw)
    assert got.smiles == base.smiles and np.array_equal(got.tries, base.tries)
    # the middle pair alone, under its id
    one = {k: (v[1:2] if k != "transform" else v) for k, v in kw.items()}
    mid = sp.interpolate_smiles(src0[1:2], src1[1:2], A, ladder=LADDER, chunk=4, pair_ids=[1], **one)
    assert mid.smiles == base.smiles[1:2] and np.array_equal(mid.tries, base.tries[1:2])
    assert np.array_equal(mid.toklen, base.toklen[1:2])
    # an accept that rejects the tries below 5: every cell resolves at rung 5, and the ladder's value is reported
    seen = {}

    def from_fifth(s):
        seen[len(seen)] = s
        return (len(seen) - 1) % 8 >= 5                                         # chunk 8: a cell's rungs are 8 consecutive rows
    late = sp.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=8, accept=from_fifth, **kw)
    assert (late.tries == 5).all() and (late.noise_std == LADDER[5]).all() and late.rows_decoded == P * A * 8
    assert all(isinstance(s, str) for row in late.smiles for s in row)
    none = sp.interpolate_smiles(src0, src1, A, ladder=LADDER[:4], chunk=16, accept=lambda s: False, **kw)
    assert all(s is None for row in none.smiles for s in row) and none.rows_decoded == P * A * 4
    # constrained decoding: every string that comes back is well formed
    wf = make_sampler(cls_name, mtype, well_formed=True)
    out = wf.interpolate_smiles(src0, src1, A, ladder=LADDER, chunk=4, **kw)
    gram = SmilesGrammar(wf.TRG.itos, wf.pad_id, wf.eos_id)
    strings = [s for row in out.smiles for s in row if s is not None]
    assert strings and all(gram.well_formed(wf.smi_to_id(s) + [wf.eos_id]) for s in strings)
    assert (out.tries >= 0).all()                                               # the grammar ends every row with <eos>
    # the records of the reference-named class
    from gct_plus_amd.Inference.mol_interpolation import SmilesInterpolation
    rec = [dict(src_0=a, src_1=b) for a, b in zip(src0, src1)]
    for r, p in zip(rec, range(P)):
        if sp.uses_scaffold:
            r.update(scaffold_0=kw["scaffolds0"][p], scaffold_1=kw["scaffolds1"][p])
        if sp.uses_props:
            r.update(props_0=kw["props0"][p], props_1=kw["props1"][p])
    df = SmilesInterpolation(sp, A, ladder=LADDER, chunk=4, transform=False).interpolate_smiles(rec)
    assert list(df.columns) == ["pair", "alpha", "smiles", "try", "noise_std", "toklen"] and len(df) == P * A
    assert [s if isinstance(s, str) else None for s in df["smiles"]] == [s for row in base.smiles for s in row]
    assert list(df["try"]) == base.tries.reshape(-1).tolist() and list(df["toklen"]) == base.toklen.reshape(-1).tolist()


@pytest.mark.parametrize("cls_name,mtype", MTYPES)
@torch.no_grad()
def test_reconstruct_smiles(cls_name, mtype):
    from gct_plus_amd.decode import reference_style_decode
    from tests.test_data_pipeline import SMILES
    sp = make_sampler(cls_name, mtype)
    mols = SMILES[:5]
    sca = ["c1ccccc1", "CC", "C1CCNCC1", "CC", "c1ccccc1"] if sp.uses_scaffold else None
    props = np.random.default_rng(2).uniform(0, 1, (5, sp.cond_dim)) if sp.uses_props else None
    smiles, same, rows = sp.reconstruct_smiles(mols, sca, props, transform=False, return_rows=True)
    assert len(smiles) == len(same) == 5
    args = [mols] + ([sca] if sca else []) + ([props] if props is not None else [])
    _, mu, _ = sp.encode_smiles(*args, **({"transform": False} if sp.uses_props else {}))
    assert torch.equal(rows.zs, mu)
    # the encoder's own mask, counted by hand: condition rows, scaffold tokens, <sep>, the molecule's tokens
    own = [sp.cond_dim + (len(data.tokenize(c)) + 1 if sca else 0) + len(data.tokenize(m))
           for m, c in zip(mols, sca or [""] * 5)]
    assert rows.src_mask.shape == (5, 1, mu.shape[1]) and max(own) == mu.shape[1]
    assert torch.equal(rows.src_mask.cpu().view(5, -1), torch.arange(mu.shape[1])[None, :] < torch.tensor(own)[:, None])
    G = rows.ys.shape[1] - int(rows.prefix_lens.max())                          # row r's tokens: ys[r, t0_r : t0_r + G]
    for t0 in torch.unique(rows.prefix_lens).tolist():
        idx = (rows.prefix_lens == t0).nonzero().view(-1).cuda()
        dc = None if rows.dconds is None else rows.dconds[idx]
        ref = reference_style_decode(sp.model, mu[idx], rows.src_mask[idx], dc, rows.ys[idx, :t0], PAD, EOS,
                                     sp.max_strlen).cpu()
        for jj, r in enumerate(idx.tolist()):
            got = upto_eos(rows.ys[r, t0:t0 + G].cpu())
            assert got == upto_eos(ref[jj, t0:]), (r, t0)
            assert smiles[r] == sp.id_to_smi(got)
    for s, m, flag in zip(smiles, mols, same):
        assert flag == (sp.smi_to_id(s) == sp.smi_to_id(m)) and (not flag or s == m)


def test_beam_sampler_refuses():
    sp = make_sampler("VaetfSampling", "vaetf", decode_algo="beam")
    with pytest.raises(ValueError, match="beam"):
        sp.interpolate_smiles(["CCO"], ["CCN"], 2)
    with pytest.raises(ValueError, match="beam"):
        sp.reconstruct_smiles(["CCO"])
    sp = make_sampler("ScaVaeSampling", "scavaetf")
    with pytest.raises(ValueError):
        sp.interpolate_smiles(["CCO"], ["CCN"], 2)                              # a scaffold type without scaffolds
    with pytest.raises(ValueError, match="int32"):
        sp.interpolate_smiles(["CCO"], ["CCN"], 2, scaffolds0=["CC"], scaffolds1=["CC"], pair_ids=[2 ** 31])
