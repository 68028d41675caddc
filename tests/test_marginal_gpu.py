"""Importance-weighted marginal likelihoods on the device: gct_latent_iw / gct_iw_combine (csrc/latent.hip) against the
fp64 host reference tests/iw_ref.py, their exactness and invariance properties bit for bit, the statistical anchor of
tests/test_marginal_host.py on the device's own draws, and decode.marginal_logp / Sampling.marginal_smiles end to end on
tiny models of all four types."""
import functools

import numpy as np
import pytest
import torch

from gct_plus_amd import data, synthetic
from tests import iw_ref as IW

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
ITEMS = (123456, 0, 2 ** 31 - 1)
GCT_ERR_ARG = -1


def case_inputs(n, Le, D, seed=0):
    g = np.random.default_rng(1000 * n + 10 * Le + D + seed)
    return (g.normal(0.3, 1.0, (n, Le, D)).astype(np.float32), g.normal(-0.3, 0.5, (n, Le, D)).astype(np.float32))


def case_rows(n, Le, flip=0):
    """rows covering 1 and Le (and something between when there is room)."""
    return [(1, Le, max(1, Le // 2 + 1))[(i + flip) % 3] for i in range(n)]


def raw_latent_iw(mu, lv, rows, items, k0, Kc, seed):
    """The library call itself on sentinel-filled outputs (ops.latent_iw allocates its own): (status, z, logw, eps)."""
    from gct_plus_amd import ops
    n, Le, D = mu.shape
    z = torch.full((n * Kc * Le * D,), SENTINEL, device="cuda")
    eps = torch.full_like(z, SENTINEL)
    logw = torch.full((n * Kc,), SENTINEL, device="cuda")
    tab = torch.tensor([list(rows), list(items)], dtype=torch.int32).reshape(2, n).cuda()
    st = ops._L().gct_latent_iw(ops._p(mu), ops._p(lv), n, Le, D, ops._p(tab[0]), ops._p(tab[1]), k0, Kc, ops._p(z),
                                ops._p(logw), ops._p(eps), seed, ops._st())
    torch.cuda.synchronize()
    return st, z, logw, eps


# ------------------------------------------------------------------------------------- 1. gct_latent_iw vs reference
@pytest.mark.parametrize("D", [1, 4, 6, 128, 130, 1024])
def test_latent_iw_vs_reference(D):
    seed = (9 << 32) | 77
    worst = dict(eps=0.0, z=0.0, logw=0.0)
    combos = [(Le, n, Kc, k0) for Le in (1, 5) for n in (0, 1, 3) for Kc in (0, 1, 3) for k0 in (0, 7)]
    if D == 1024:                                                              # the widest row: one case is enough
        combos = [(2, 2, 2, 7)]
    for Le, n, Kc, k0 in combos:
        mu, lv = case_inputs(n, Le, D)
        rows, items = case_rows(n, Le, flip=k0), ITEMS[:n]
        st, z, logw, eps = raw_latent_iw(torch.from_numpy(mu).cuda(), torch.from_numpy(lv).cuda(), rows, items, k0, Kc, seed)
        assert st == 0, (D, Le, n, Kc, k0)
        z, eps = (t.cpu().numpy().reshape(n, Kc, Le, D) for t in (z, eps))
        logw = logw.cpu().numpy().reshape(n, Kc)
        if n * Kc == 0:
            continue
        assert np.isfinite(z).all() and np.isfinite(eps).all() and np.isfinite(logw).all()
        assert not (z == SENTINEL).any() and not (eps == SENTINEL).any() and not (logw == SENTINEL).any()
        own = np.broadcast_to(IW.own_rows(rows, Le), z.shape)
        for t in (z, eps):                                                      # exact +0 at and beyond rows[i]
            assert not t[~own].any() and not np.signbit(t[~own]).any()
        # the draws: the reference's normals, within the tolerance the N(0, 1) streams are held to
        want_eps = IW.iw_draws(seed, items, k0, Kc, Le, D)
        e_err = np.abs(eps - want_eps)[own]
        e_tol = (1e-5 * np.maximum(1.0, np.abs(want_eps)))[own]
        # z from the kernel's own eps, gct_reparam_fwd's rule: atol 1e-6, rtol 1e-6
        z64, logw64 = IW.latent_iw_ref(mu, lv, rows, eps)
        z_err, z_tol = np.abs(z - z64), 1e-6 + 1e-6 * np.abs(z64)
        # logw from the kernel's own eps, within the derived bound
        l_err, l_tol = np.abs(logw - logw64), IW.logw_tolerance(mu, lv, rows, eps, z64)
        for key, err, tol in (("eps", e_err, e_tol), ("z", z_err, z_tol), ("logw", l_err, l_tol)):
            worst[key] = max(worst[key], float((err / tol).max()))
            assert np.all(err <= tol), (key, D, Le, n, Kc, k0, float((err / tol).max()))
    print(f"latent_iw D={D}: worst error over tolerance eps {worst['eps']:.3f}, z {worst['z']:.3f}, logw {worst['logw']:.3f}")


# -------------------------------------------------------------------------------- 2. exactness and invariance, bitwise
def run_iw(mu, lv, rows, items, k0, Kc, seed, want_eps=False):
    from gct_plus_amd import ops
    return ops.latent_iw(mu, lv, list(rows), list(items), k0, Kc, seed, want_eps=want_eps)


@pytest.mark.parametrize("D", [6, 128])
def test_zero_posterior_is_the_prior_exactly(D):
    n, Le, K = 3, 5, 4
    zero = torch.zeros(n, Le, D, device="cuda")
    rows = case_rows(n, Le)
    z, logw, eps = run_iw(zero, zero, rows, ITEMS, 0, K, 31, want_eps=True)
    assert torch.equal(z, eps)
    assert torch.equal(logw, torch.zeros(n * K, device="cuda"))
    assert bool((z.view(n, K, Le, D)[1] != 0).all())                           # rows[1] = Le: real draws, not zeros


@pytest.mark.parametrize("D", [6, 128])
def test_draws_do_not_depend_on_the_call(D):
    n, Le, K, seed = 3, 5, 6, (3 << 32) | 5
    mu, lv = (torch.from_numpy(t).cuda() for t in case_inputs(n, Le, D))
    rows = case_rows(n, Le)
    z, logw, eps = run_iw(mu, lv, rows, ITEMS, 0, K, seed, want_eps=True)
    assert z.shape == (n * K, Le, D) and logw.shape == (n * K,)
    again = run_iw(mu, lv, rows, ITEMS, 0, K, seed, want_eps=True)
    assert all(torch.equal(a, b) for a, b in zip((z, logw, eps), again))
    # want_eps on or off
    z0, logw0, none = run_iw(mu, lv, rows, ITEMS, 0, K, seed)
    assert none is None and torch.equal(z0, z) and torch.equal(logw0, logw)
    # k-ranges [0, 2) + [2, 6)
    parts = [run_iw(mu, lv, rows, ITEMS, k0, kc, seed) for k0, kc in ((0, 2), (2, 4))]
    assert torch.equal(torch.cat([p[0].view(n, -1, Le, D) for p in parts], 1), z.view(n, K, Le, D))
    assert torch.equal(torch.cat([p[1].view(n, -1) for p in parts], 1), logw.view(n, K))
    # molecules permuted, and one at a time
    perm = [2, 0, 1]
    zp, lp, _ = run_iw(mu[perm].contiguous(), lv[perm].contiguous(), [rows[i] for i in perm], [ITEMS[i] for i in perm],
                       0, K, seed)
    assert torch.equal(zp.view(n, K, Le, D), z.view(n, K, Le, D)[perm]) and torch.equal(lp.view(n, K), logw.view(n, K)[perm])
    for i in range(n):
        z1, l1, _ = run_iw(mu[i:i + 1].contiguous(), lv[i:i + 1].contiguous(), rows[i:i + 1], ITEMS[i:i + 1], 0, K, seed)
        assert torch.equal(z1, z.view(n, K, Le, D)[i]) and torch.equal(l1, logw.view(n, K)[i])
    # a longer latent buffer (another Le): the molecule's own rows are the same
    pad = lambda t: torch.cat([t, torch.full((n, 3, D), 7.0, device="cuda")], 1).contiguous()       # noqa: E731
    z2, l2, _ = run_iw(pad(mu), pad(lv), rows, ITEMS, 0, K, seed)
    assert torch.equal(z2[:, :Le], z) and not z2[:, Le:].any() and torch.equal(l2, logw)
    # and the seed and the item matter
    assert not torch.equal(run_iw(mu, lv, rows, ITEMS, 0, K, seed + 1)[0], z)
    zi = run_iw(mu, lv, rows, (ITEMS[0], 1, ITEMS[2]), 0, K, seed)[0].view(n, K, Le, D)
    assert torch.equal(zi[[0, 2]], z.view(n, K, Le, D)[[0, 2]]) and not torch.equal(zi[1], z.view(n, K, Le, D)[1])


def test_more_rows_than_workgroups():
    """Beyond 2^20 output rows a workgroup walks several rows: the rows are those of two smaller calls."""
    Le, D, K, seed = 1, 4, (1 << 20) + 5, 8
    mu, lv = (torch.from_numpy(t).cuda() for t in case_inputs(1, Le, D))
    z, logw, _ = run_iw(mu, lv, [1], [42], 0, K, seed)
    half = 1 << 19
    a, b = run_iw(mu, lv, [1], [42], 0, half, seed), run_iw(mu, lv, [1], [42], half, K - half, seed)
    assert torch.equal(z, torch.cat([a[0], b[0]])) and torch.equal(logw, torch.cat([a[1], b[1]]))
    assert abs(float(z.mean()) - float(mu.mean())) < 0.01                      # about 4 M draws around mu


# ------------------------------------------------------------------------------------------------------ 3. refusals
def test_latent_iw_refusals_leave_the_outputs_untouched():
    from gct_plus_amd import ops
    from gct_plus_amd._lib import GctError
    n, Le, D = 2, 3, 8
    mu, lv = (torch.from_numpy(t).cuda() for t in case_inputs(n, Le, D))
    good = dict(rows=[1, 3], items=[0, 5], k0=0, Kc=2, seed=1)
    st, z, logw, eps = raw_latent_iw(mu, lv, **good)
    assert st == 0 and not (z == SENTINEL).any() and not (logw == SENTINEL).any()
    for bad in (dict(D=0), dict(D=1025), dict(Le=0), dict(k0=-1), dict(Kc=-1), dict(Kc=(1 << 25) // (n * Le) + 1),
                dict(Le=(1 << 24) + 1, Kc=1)):
        k = dict(good, **bad)
        # the outputs are sized for the good call: a refused call must not touch them, whatever it was asked for
        z = torch.full((n * 2 * Le * D,), SENTINEL, device="cuda")
        eps, logw = torch.full_like(z, SENTINEL), torch.full((n * 2,), SENTINEL, device="cuda")
        tab = torch.tensor([k["rows"], k["items"]], dtype=torch.int32).cuda()
        st = ops._L().gct_latent_iw(ops._p(mu), ops._p(lv), n, k.get("Le", Le), k.get("D", D), ops._p(tab[0]),
                                    ops._p(tab[1]), k["k0"], k["Kc"], ops._p(z), ops._p(logw), ops._p(eps), k["seed"],
                                    ops._st())
        torch.cuda.synchronize()
        assert st == GCT_ERR_ARG, bad
        assert bool((z == SENTINEL).all()) and bool((eps == SENTINEL).all()) and bool((logw == SENTINEL).all()), bad
    # the wrapper: the same limits, and the per-molecule tables, before a launch
    for shape in ((n, Le, 0), (n, Le, 1025), (n, 0, D)):
        with pytest.raises(GctError):
            ops.latent_iw(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"), [1] * n, [0] * n, 0, 1, 1)
    for bad in (dict(k0=-1), dict(Kc=-1), dict(rows=[0, 3]), dict(rows=[1, 4]), dict(items=[0, -1])):
        k = dict(good, **bad)
        with pytest.raises(GctError):
            ops.latent_iw(mu, lv, k["rows"], k["items"], k["k0"], k["Kc"], k["seed"])
    for bad in (dict(rows=[1]), dict(items=[0, 1, 2])):
        k = dict(good, **bad)
        with pytest.raises(ValueError):
            ops.latent_iw(mu, lv, k["rows"], k["items"], k["k0"], k["Kc"], k["seed"])
    with pytest.raises(ValueError):
        ops.latent_iw(mu, lv[:, :2].contiguous(), good["rows"], good["items"], 0, 2, 1)
    with pytest.raises(ValueError):
        ops.latent_iw(mu.transpose(1, 2), lv.transpose(1, 2), good["rows"], good["items"], 0, 2, 1)
    with pytest.raises(GctError):
        ops.latent_iw(mu.cpu(), lv.cpu(), good["rows"], good["items"], 0, 2, 1)
    # zero molecules / zero draws: nothing to write, no error
    z, logw, _ = ops.latent_iw(mu[:0].contiguous(), lv[:0].contiguous(), [], [], 0, 3, 1)
    assert z.shape == (0, Le, D) and logw.shape == (0,)
    z, logw, _ = ops.latent_iw(mu, lv, good["rows"], good["items"], 4, 0, 1)
    assert z.shape == (0, Le, D) and logw.shape == (0,)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- 4. gct_iw_combine
@functools.lru_cache(maxsize=None)
def combine_case(n, K):
    g = np.random.default_rng(100 * n + K)
    logp = g.uniform(-200, 200, (n, K)).astype(np.float32)                     # a missing max-shift overflows
    logw = g.normal(0, 5, (n, K)).astype(np.float32)
    if n > 1 and K > 1:
        logp[1] = -30 + g.normal(0, 0.3, K).astype(np.float32)                 # one molecule with many live weights
        logw[1] = g.normal(0, 0.3, K).astype(np.float32)
    want = IW.combine_ref(logp, logw)
    assert n < 2 or K < 2 or want[3][1] > K / 2                                # (its effective sample size says so)
    return logp, logw, want


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_iw_combine_vs_reference(n, K):
    from gct_plus_amd import ops
    logp, logw, want = combine_case(n, K)
    got = ops.iw_combine(torch.from_numpy(logp).cuda().view(-1), torch.from_numpy(logw).cuda().view(-1), n, K)
    assert all(t.shape == (n,) and t.dtype == torch.float32 for t in got)
    worst = 0.0
    for name, g, w in zip(("iwae", "elbo", "recon", "ess"), got, want):
        g = g.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), name
        err, tol = np.abs(g - w), IW.combine_tolerance(w)
        worst = max(worst, float((err / tol).max()) if n else 0.0)
        assert np.all(err <= tol), (name, n, K, g, w)
    print(f"iw_combine n={n} K={K}: worst error over tolerance {worst:.3f}")
    iwae, elbo, recon, ess = got
    assert bool((elbo <= iwae).all()) and bool((ess >= 1).all()) and bool((ess <= K).all())
    if K == 1:
        assert torch.equal(iwae, elbo) and torch.equal(ess, torch.ones(n, device="cuda"))
        assert torch.equal(recon.cpu(), torch.from_numpy(logp[:, 0]))


def test_iw_combine_refusals():
    from gct_plus_amd import ops
    x = torch.zeros(6, device="cuda")
    for n, K in ((2, 0), (2, -1), (-1, 3), (2, 2), (3, 3)):
        with pytest.raises(ValueError):
            ops.iw_combine(x, x, n, K)
    with pytest.raises(ValueError):
        ops.iw_combine(x.view(2, 3), x.view(2, 3), 2, 3)
    with pytest.raises(ValueError):
        ops.iw_combine(torch.zeros(12, device="cuda")[::2], x, 2, 3)


# ------------------------------------------------------------------------------------- 5. the statistical anchor
def test_statistical_anchor_on_the_device():
    """tests/test_marginal_host.py's anchor on the device's own draws and terms: same seed, same bound."""
    from gct_plus_amd import ops
    s = IW.STAT
    mu = torch.full((1, s["rows"], s["D"]), s["mu"], device="cuda")
    lv = torch.full((1, s["rows"], s["D"]), s["log_var"], device="cuda")
    _, logw, _ = ops.latent_iw(mu, lv, [s["rows"]], [s["item"]], 0, s["K"], IW.STAT_SEED)
    mean, dist = IW.stat_check(logw.cpu().numpy())
    print(f"anchor on the device: mean {mean:.5f}, {dist:.2f} standard errors from 1")
    assert dist <= 6.0


# ------------------------------------------------------------------------------------------------- 6. end to end
TINY = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
MTYPES = [("VaetfSampling", "vaetf"), ("CvaetfSampling", "pvaetf"), ("ScaVaeSampling", "scavaetf"),
          ("PscavaetfSampling", "pscavaetf")]
SCAFFOLDS = ["c1ccccc1", "CC", "C1CCNCC1", "CC", "c1ccccc1"]
E2E_K, E2E_SEED = 3, 21


def make_sampler(cls_name, mtype):
    from gct_plus_amd.Inference import sampling_tool
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    strs = [s + "<sep>" + m for s in set(SCAFFOLDS) for m in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    nc = synthetic.n_conds(mtype)
    torch.manual_seed(4)
    model = model_dict[mtype](len(SRC), len(TRG), dropout=0.1, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
    return getattr(sampling_tool, cls_name)(model, SRC, TRG, latent_dim=16, max_strlen=40, cond_dim=nc,
                                            toklen_data=[12, 14, 15, 18, 20, 16], seed=12)


def molecule_args(sp, n=5):
    """n molecules of different lengths with the positional arguments the sampler's type takes behind them."""
    from tests.test_data_pipeline import SMILES
    mols = [SMILES[i] for i in (9, 11, 0, 1, 3)][:n]
    assert len({len(m) for m in mols}) > 2
    args = []
    if sp.uses_scaffold:
        args.append(SCAFFOLDS[:n])
    kw = {}
    if sp.uses_props:
        args.append(np.random.default_rng(8).uniform(0, 1, (n, sp.cond_dim)))
        kw["transform"] = False
    return mols, args, kw


@pytest.mark.parametrize("cls_name,mtype", MTYPES)
def test_marginal_smiles_end_to_end(cls_name, mtype, monkeypatch):
    from gct_plus_amd import decode, ops
    from gct_plus_amd.Model.modules import get_src_mask
    sp = make_sampler(cls_name, mtype)
    mols, args, kw = molecule_args(sp)
    n, K = len(mols), E2E_K
    blocks = []
    real = ops.latent_iw

    def recording(mu, lv, rows, items, k0, Kc, seed, want_eps=False):
        out = real(mu, lv, rows, items, k0, Kc, seed, want_eps)
        blocks.append((torch.as_tensor(items).tolist(), k0, Kc, out[0].clone()))
        return out
    monkeypatch.setattr(decode.ops, "latent_iw", recording)

    res, zs = {}, {}
    for chunk in (2, 4, 1000):
        blocks.clear()
        m = sp.marginal_smiles(mols, *args, K=K, seed=E2E_SEED, chunk=chunk, return_weights=True, **kw)
        assert len(blocks) == {2: 2 * n, 4: n, 1000: 1}[chunk]
        assert all(len(it) * kc <= chunk for it, _, kc, _ in blocks)
        Le, D = blocks[0][3].shape[1:]
        z = torch.full((n, K, Le, D), float("nan"), device="cuda")
        for it, k0, kc, zb in blocks:                                           # items default to arange(n)
            z[it[0]:it[-1] + 1, k0:k0 + kc] = zb.view(len(it), kc, Le, D)
        assert not torch.isnan(z).any()
        res[chunk], zs[chunk] = m, z
        # the combine, against the reference fed with this call's own parts
        assert m.logp.shape == (n, K) and m.logw.shape == (n, K) and m.log_w.dtype == torch.float64
        assert torch.equal(m.log_w, m.logp.double() + m.logw.double())
        want = decode.marginal_reference(m.logp, m.logw)
        for name in ("iwae", "elbo", "recon", "ess"):
            g, w = getattr(m, name).double().numpy(), getattr(want, name).numpy()
            assert np.all(np.abs(g - w) <= IW.combine_tolerance(w)), (name, chunk, g, w)
        assert bool((m.elbo <= m.iwae).all()) and bool((m.ess >= 1).all()) and bool((m.ess <= K).all())
        assert bool((m.logp < 0).all()) and torch.isfinite(m.log_w).all()
    for chunk in (2, 4):                                                        # the draws do not depend on the blocks
        assert torch.equal(zs[chunk], zs[1000]) and torch.equal(res[chunk].logw, res[1000].logw)
        assert torch.equal(res[chunk].tokens, res[1000].tokens)

    # tokens: score_smiles'; the decoder's part: Sampling.score of the same rows and latents, at the project's
    # tolerance for log-probabilities under another batching (1e-4 per scored token)
    sc = sp.score_smiles(mols, *args, **kw)
    full = res[1000]
    assert torch.equal(full.tokens, sc.tokens) and int(sc.tokens.min()) >= 2
    ys, lens, _ = sp._score_targets(mols, args[0] if sp.uses_scaffold else None)
    props = args[-1] if sp.uses_props else None
    mu, log_var, src_mask = sp._encode_endpoints(mols, args[0] if sp.uses_scaffold else None, props, False)
    rows = src_mask[:, 0].sum(1).cpu()
    assert len(set(rows.tolist())) > 2 and int(rows.max()) == mu.shape[1]
    if sp.uses_props:
        assert bool(src_mask[:, 0, :sp.cond_dim].all())                        # condition rows are latent rows too
    zfull = zs[1000]
    for i in range(n):                                                          # zeros behind each molecule's own rows
        assert not zfull[i, :, int(rows[i]):].any() and bool((zfull[i, :, :int(rows[i])] != 0).all())
    rep = lambda x: None if x is None else x.repeat_interleave(K, 0)           # noqa: E731
    dconds = sp._conds(props, False)
    each = sp.score(zfull.view(n * K, *zfull.shape[2:]), rep(ys), rep(src_mask), rep(dconds), rep(lens))
    err = (each.logp.view(n, K).double() - full.logp.double()).abs()
    assert bool((err <= 1e-4 * sc.tokens.view(-1, 1)).all()), err
    # logw: the reference from mu, log_var and the latents themselves (eps = (z - mu) / sigma is not needed: the term
    # is a function of z) -- log N(z; 0, I) - log N(z; mu, sigma^2) over the own rows, in fp64
    z64, mu64, lv64 = zfull.double().cpu(), mu.double().cpu().unsqueeze(1), log_var.double().cpu().unsqueeze(1)
    own = (torch.arange(mu.shape[1]).view(1, -1) < rows.view(-1, 1)).view(n, 1, -1, 1)
    term = 0.5 * (-(z64 ** 2) + (z64 - mu64) ** 2 / torch.exp(lv64) + lv64)
    want_logw = torch.where(own, term, torch.zeros((), dtype=torch.float64)).sum((2, 3))
    scale = torch.where(own, (z64.abs() + mu64.abs()) ** 2 / torch.exp(lv64) + z64 ** 2 + lv64.abs(),
                        torch.zeros((), dtype=torch.float64)).sum((2, 3))
    assert bool(((full.logw.double() - want_logw).abs() <= 1e-5 * scale).all())

    # marginal_smiles is Sampling.marginal on hand-built inputs
    hand_ys = []
    for j, mol in enumerate(mols):
        pre = sp.smi_to_id(args[0][j]) + [sp.sep_id] if sp.uses_scaffold else []
        hand_ys.append([sp.sos_id] + pre + sp.smi_to_id(mol) + [sp.eos_id])
    W = max(len(r) for r in hand_ys)
    hand = torch.tensor([r + [sp.pad_id] * (W - len(r)) for r in hand_ys])
    hand_lens = [len(sp.smi_to_id(s)) + 2 for s in args[0]] if sp.uses_scaffold else None
    enc = sp.encode_smiles(mols, *args, **kw)
    strings = [b + "<sep>" + a for a, b in zip(mols, args[0])] if sp.uses_scaffold else mols
    src = sp.tokenize_smiles(strings).cuda()
    econds = None if props is None else torch.as_tensor(props, dtype=torch.float32).cuda()
    hand_mask = get_src_mask(src, sp.pad_id, econds)
    got = sp.marginal(enc[1], enc[2], hand_mask, hand, None if props is None else torch.as_tensor(props, dtype=torch.float32),
                      hand_lens, K=K, seed=E2E_SEED, chunk=4, return_weights=True)
    assert all(torch.equal(a, b) for a, b in zip(got, res[4]))
    assert got.iwae.device.type == "cpu"

    # seed=None advances the sampler's counter: two calls draw different latents; a given seed repeats
    a = sp.marginal_smiles(mols, *args, K=K, **kw)
    b = sp.marginal_smiles(mols, *args, K=K, **kw)
    assert not torch.equal(a.iwae, b.iwae) and torch.equal(a.tokens, b.tokens)
    c = sp.marginal_smiles(mols, *args, K=K, seed=sp.marginal_seed, **kw)
    assert torch.equal(c.iwae, b.iwae) and c.log_w is None
