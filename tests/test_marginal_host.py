"""Importance-weighted marginal likelihoods, host side: the rules of decode.marginal_reference / latent_iw_reference, the
refusals of decode.marginal_logp, the block walk, and the reference random streams of tests/iw_ref.py -- their layout
and the statistical anchor the GPU test repeats on the device's own draws."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd import decode
from tests import iw_ref as IW


def weights(n, K, seed=0, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    return -20 + spread * torch.randn(n, K, generator=g, dtype=torch.float64), torch.randn(n, K, generator=g,
                                                                                           dtype=torch.float64)


# ------------------------------------------------------------------------------------------- marginal_reference
def test_one_draw_is_the_elbo():
    logp, logw = weights(5, 1)
    m = decode.marginal_reference(logp, logw)
    assert torch.equal(m.iwae, m.elbo) and torch.equal(m.ess, torch.ones(5, dtype=torch.float64))
    assert torch.equal(m.elbo, (logp + logw)[:, 0]) and torch.equal(m.recon, logp[:, 0])


@pytest.mark.parametrize("K", [2, 7, 64])
def test_equal_weights(K):
    common = torch.tensor([-31.5, 0.0, 12.25], dtype=torch.float64)
    logp = common.view(-1, 1).expand(3, K) - 1.5
    m = decode.marginal_reference(logp, torch.full((3, K), 1.5, dtype=torch.float64))
    assert torch.allclose(m.ess, torch.full((3,), float(K), dtype=torch.float64), rtol=1e-13, atol=0)
    assert torch.allclose(m.iwae, common, rtol=0, atol=1e-12) and torch.allclose(m.elbo, common, rtol=0, atol=1e-12)
    assert torch.allclose(m.recon, common - 1.5, rtol=0, atol=1e-12)


@pytest.mark.parametrize("K", [2, 3, 64, 1000])
def test_jensen_holds_per_molecule(K):
    logp, logw = weights(40, K, seed=K, spread=30.0)
    m = decode.marginal_reference(logp, logw)
    top = (logp + logw).max(1).values
    assert bool((m.elbo <= m.iwae).all()) and bool((m.iwae <= top).all())
    assert bool((m.iwae >= top - math.log(K)).all())                           # the largest weight alone
    assert bool((m.ess >= 1 - 1e-12).all()) and bool((m.ess <= K + 1e-9).all())
    assert torch.equal(m.log_w, logp + logw)
    # against the textbook form
    assert torch.allclose(m.iwae, torch.logsumexp(logp + logw, 1) - math.log(K), rtol=0, atol=1e-10)


def test_a_constant_shifts_the_bounds_and_leaves_ess():
    logp, logw = weights(9, 17, seed=4, spread=8.0)
    a, b = decode.marginal_reference(logp, logw), decode.marginal_reference(logp + 37.25, logw)
    for x, y in ((a.iwae, b.iwae), (a.elbo, b.elbo), (a.recon, b.recon)):
        assert torch.allclose(y, x + 37.25, rtol=0, atol=1e-11)
    assert torch.allclose(a.ess, b.ess, rtol=1e-12, atol=0)


def test_weights_far_apart_do_not_overflow():
    logp = torch.tensor([[-200.0, 200.0, 0.0], [700.0, 700.0, -700.0]], dtype=torch.float64)
    m = decode.marginal_reference(logp, torch.zeros(2, 3, dtype=torch.float64))
    assert torch.isfinite(m.iwae).all() and torch.isfinite(m.ess).all()
    assert m.iwae[0].item() == pytest.approx(200 - math.log(3), abs=1e-12) and m.ess[0].item() == pytest.approx(1.0)
    assert m.iwae[1].item() == pytest.approx(700 + math.log(2 / 3), abs=1e-12) and m.ess[1].item() == pytest.approx(2.0)


def test_reference_from_the_draws_matches_iw_ref():
    """marginal_reference(eps=) goes through latent_iw_reference, which states the kernel's arithmetic in torch; the
    numpy reference of tests/iw_ref.py was written separately from the header.  They agree, and the closed forms hold:
    logw = log N(z; 0, I) - log N(z; mu, sigma^2) over the molecule's own rows."""
    g = np.random.default_rng(5)
    n, K, Le, D, rows = 3, 4, 5, 6, [1, 5, 3]
    mu, lv = g.normal(0.2, 0.7, (n, Le, D)), g.normal(-0.3, 0.5, (n, Le, D))
    eps = IW.iw_draws(11, [4, 0, 9], 2, K, Le, D)
    z, logw = decode.latent_iw_reference(mu, lv, rows, eps)
    z2, logw2 = IW.latent_iw_ref(mu, lv, rows, eps)
    assert np.allclose(z.numpy(), z2, rtol=0, atol=1e-14) and np.allclose(logw.numpy(), logw2, rtol=1e-13, atol=1e-13)
    for i, r in enumerate(rows):
        assert not z[i, :, r:].any()
        zz, m, l = z[i, :, :r].numpy(), mu[i, :r], lv[i, :r]
        logn = lambda x, mean, logvar: (-0.5 * (math.log(2 * math.pi) + logvar + (x - mean) ** 2 / np.exp(logvar)))  # noqa: E731
        want = (logn(zz, 0.0, 0.0) - logn(zz, m, l)).sum((1, 2))
        assert np.allclose(logw[i].numpy(), want, rtol=1e-12, atol=1e-12)
    logp = torch.from_numpy(g.normal(-20, 2, (n, K)))
    a, b = decode.marginal_reference(logp, mu=mu, log_var=lv, rows=rows, eps=eps), decode.marginal_reference(logp, logw)
    assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    want = IW.combine_ref(logp.numpy(), logw2)
    assert all(np.allclose(x.numpy(), y, rtol=1e-13, atol=1e-13) for x, y in zip(a[:4], want))


def test_reference_refusals():
    with pytest.raises(ValueError):
        decode.marginal_reference(torch.zeros(3, 0), torch.zeros(3, 0))         # K < 1
    with pytest.raises(ValueError):
        decode.marginal_reference(torch.zeros(3, 2), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        decode.marginal_reference(torch.zeros(3, 2))                            # neither logw nor the draws
    with pytest.raises(ValueError):
        decode.latent_iw_reference(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), [1, 4], torch.zeros(2, 1, 3, 4))
    with pytest.raises(ValueError):
        decode.latent_iw_reference(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), [1, 3], torch.zeros(2, 1, 3, 5))


# ------------------------------------------------------------------------------------------- marginal_logp, host part
def tiny_cpu_model():
    from gct_plus_amd.Model import model_dict
    torch.manual_seed(0)
    return model_dict["vaetf"](12, 12, N=1, d_model=16, dff=32, h=2, latent_dim=8, dropout=0.0, nconds=0)


def test_marginal_logp_refusals_come_before_any_device_work():
    """Everything lives on the CPU here: a call that got as far as a launch would raise something else."""
    model = tiny_cpu_model()
    n, Le, D, W = 3, 5, 8, 6
    mu, lv = torch.zeros(n, Le, D), torch.zeros(n, Le, D)
    mask = torch.arange(Le).view(1, 1, Le) < torch.tensor([5, 2, 1]).view(n, 1, 1)
    ys = torch.randint(2, 12, (n, W))
    ok = dict(mu=mu, log_var=lv, src_mask=mask, dconds=None, ys=ys)
    for bad in (dict(K=0), dict(K=-3), dict(K=2.0), dict(K=True), dict(chunk=0), dict(chunk=1.5),
                dict(log_var=torch.zeros(n, Le, D + 1)), dict(mu=torch.zeros(n, Le), log_var=torch.zeros(n, Le)),
                dict(src_mask=mask[:2]), dict(src_mask=mask[:, 0]), dict(src_mask=torch.ones(n, 1, Le + 1, dtype=torch.bool)),
                dict(ys=ys[:2]), dict(ys=ys[:, 0]), dict(ys=ys.float()), dict(ys=ys + 100),
                dict(prefix_lens=[1, 2]), dict(prefix_lens=[1, 2, W + 1]), dict(items=[0, 1]), dict(items=[0, -1, 2])):
        with pytest.raises(ValueError):
            decode.marginal_logp(model, **dict(ok, **bad))
    holes = mask.clone()
    holes[0, 0, 2] = False                                                      # marked rows that are not a prefix
    empty = mask.clone()
    empty[1] = False
    late = mask.roll(1, 2)
    for m in (holes, empty, late):
        with pytest.raises(ValueError, match="prefix"):
            decode.marginal_logp(model, mu, lv, m, None, ys)
    assert decode.latent_rows(mask, n, Le).tolist() == [5, 2, 1]


@pytest.mark.parametrize("n,K,chunk", [(5, 3, 2), (5, 3, 4), (5, 3, 1000), (0, 3, 4), (4, 1, 1), (3, 64, 64), (3, 64, 63),
                                       (7, 4, 9), (2, 10, 3)])
def test_blocks_cover_every_row_once(n, K, chunk):
    seen = np.zeros((n, K), dtype=int)
    for i0, i1, k0, k1 in decode.marginal_blocks(n, K, chunk):
        assert 0 <= i0 < i1 <= n and 0 <= k0 < k1 <= K and (i1 - i0) * (k1 - k0) <= chunk
        assert (k0, k1) == (0, K) or i1 - i0 == 1                               # whole molecules, or one molecule's k-range
        seen[i0:i1, k0:k1] += 1
    assert (seen == 1).all()


# ------------------------------------------------------------------------------------------- the reference's streams
def test_draws_depend_on_seed_item_k_t_d_alone():
    seed, D, Le = 77, 10, 6
    full = IW.iw_draws(seed, [5, 0, 123456, 2 ** 31 - 1], 0, 9, Le, D)          # [4, 9, Le, D]
    # another n and order of molecules, another Le, another D, another split of k
    assert np.array_equal(IW.iw_draws(seed, [123456], 0, 9, Le, D)[0], full[2])
    assert np.array_equal(IW.iw_draws(seed, [2 ** 31 - 1, 5], 0, 9, Le, D), full[[3, 0]])
    assert np.array_equal(IW.iw_draws(seed, [0], 0, 9, 2, D)[0], full[1][:, :2])
    assert np.array_equal(IW.iw_draws(seed, [0], 0, 9, Le + 3, D)[0][:, :Le], full[1])
    assert np.array_equal(IW.iw_draws(seed, [5], 0, 9, Le, 3)[0], full[0][:, :, :3])
    assert np.array_equal(IW.iw_draws(seed, [5], 0, 9, Le, 128)[0][:, :, :D], full[0])
    parts = [IW.iw_draws(seed, [5, 0], k0, kc, Le, D) for k0, kc in ((0, 2), (2, 4), (6, 3))]
    assert np.array_equal(np.concatenate(parts, 1), full[:2])
    assert np.array_equal(IW.iw_draws(seed, [0], 7, 1, Le, D)[0, 0], full[1, 7])
    # and every coordinate matters
    flat = full.reshape(-1)
    assert np.unique(flat).size == flat.size
    assert not np.array_equal(IW.iw_draws(seed + 1, [5], 0, 9, Le, D)[0], full[0])
    # the stated counter, by hand: element (item 5, k 3, t 4, d 9) is element 1 of the call (5, 3, 256 * 4 + 2, C3)
    from tests import rng_ref as R
    x, y, _, _ = (int(w) for w in R.philox4x32_10((5, 3, 256 * 4 + 2, IW.IW_C3), R.rng_key(seed, IW.IW_SITE)))
    rad = math.sqrt(-2 * math.log(((x >> 8) + 1) / 2 ** 24))
    ang = float(np.float32(6.283185307179586)) * ((y >> 8) + 1) / 2 ** 24
    assert full[0, 3, 4, 8] == pytest.approx(rad * math.cos(ang), abs=1e-14)
    assert full[0, 3, 4, 9] == pytest.approx(rad * math.sin(ang), abs=1e-14)


def test_draws_are_standard_normal_and_apart_from_the_interpolation_stream():
    from tests import latent_ref as LR
    e = IW.iw_draws(42, [7], 0, 500, 4, 128).reshape(-1)                        # 256 000 values
    n = e.size
    assert abs(e.mean()) < 5 / math.sqrt(n) and abs(e.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs((e ** 4).mean() - 3) < 5 * math.sqrt(96 / n)
    other = IW.iw_draws(42, [8], 0, 500, 4, 128).reshape(-1)
    assert abs(np.corrcoef(e, other)[0, 1]) < 5 / math.sqrt(n)
    assert (IW.IW_SITE, IW.IW_C3) != (LR.LATENT_SITE, LR.LATENT_C3)
    assert not np.array_equal(IW.iw_draws(42, [7], 0, 1, 4, 128)[0, 0], LR.token_normals(42, 7, 4, 128)[:, 0])


def test_statistical_anchor():
    """E_q[p / q] = 1: the mean of exp(logw) over 65 536 reference draws lies within 6 standard errors of 1, the
    standard error from the closed-form second moment.  A wrong sign, a missing 0.5, a missing log_var term or a draw
    that is not N(0, 1) moves the mean by far more."""
    s = IW.STAT
    mu = np.full((1, s["rows"], s["D"]), s["mu"])
    lv = np.full((1, s["rows"], s["D"]), s["log_var"])
    eps = IW.iw_draws(IW.STAT_SEED, [s["item"]], 0, s["K"], s["rows"], s["D"])
    logw = IW.latent_iw_ref(mu, lv, [s["rows"]], eps)[1]
    mean, dist = IW.stat_check(logw)
    second = float(np.exp(2 * logw).mean())
    print(f"anchor: mean {mean:.5f}, {dist:.2f} standard errors from 1; second moment {second:.3f} "
          f"(closed form {IW.stat_second_moment():.3f})")
    assert 3.0 < IW.stat_second_moment() < 4.5
    assert dist <= 6.0
    for wrong in (-logw, 2 * logw, logw + 0.5 * s["log_var"] * s["rows"] * s["D"]):
        assert IW.stat_check(wrong)[1] > 6.0
