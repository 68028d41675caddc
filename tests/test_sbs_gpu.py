"""Stochastic beam search on the device: gct_beam_select_gumbel against the host statement of the rules in fp64
(decode.sbs_step_reference) and its draw against tests/sbs_ref.py; KVDecoder.generate_sbs -- distinct beams, scores
against score_tokens, seeds, graph replay, the un-cached reference-style loop, the first token's distribution; the
sampling front end (decode_algo="stochastic_beam", decode_unique and its rows in a policy-gradient step).

Tolerances.  Scores: test_beam_decode_gpu.py's for gct_beam_select (rtol 1e-6, atol 0).  Gumbel values: atol 1e-3 = GAP,
the near-tie bound of tests/sbs_ref.py.  Draw: rtol = atol = 1e-5 -- two chained logf at 2 ulp each; the inner one's
relative error enters the outer absolutely, about 2.4e-7; the outer's own error is at most 2 ulp of at most 17, about
4e-6.  logp against score_tokens: tests/test_score_gpu.py's device-path rule, 2e-4 + 1e-4 |logp| per token, summed."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd import ops, synthetic
from gct_plus_amd.decode import KVDecoder, SbsSamples, reference_style_sbs_decode, sbs_root_gumbels, score_tokens
from tests import sbs_ref
from tests.sbs_ref import GAP
from tests.test_beam_decode_gpu import TINY, build

pytestmark = pytest.mark.gpu
PAD, EOS, SOS = synthetic.PAD_ID, synthetic.EOS_ID, synthetic.SOS_ID
GCT_ERR_ARG = -1


def chi2_quantile_1e3(dof):
    """Upper 1e-3 quantile of chi-square by Wilson-Hilferty (within 1 % for dof >= 2; z = 3.0902)."""
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + 3.0902323 * math.sqrt(a)) ** 3


# ----------------------------------------------------------------------------------------- gct_beam_select_gumbel
def run_select(case, k, p, off, seed=0, seed_dev=None, noise_in=True, sentinel=-7.5):
    n = case["scores"].shape[0]
    rows = n * k
    d = dict(logits=case["logits"].cuda(), scores=case["scores"].reshape(-1).float().cuda(),
             gumbels=case["gumbels"].reshape(-1).float().cuda(), fin=case["fin"].reshape(-1).to(torch.uint8).cuda(),
             lens=case["lens"].reshape(-1).to(torch.int32).cuda(), ys=case["ys"].cuda(), valid=case["valid"].cuda(),
             kv_src=case["kv_src"].cuda(), done=torch.zeros(n, dtype=torch.uint8, device="cuda"),
             parent=torch.full((rows,), -7, dtype=torch.int32, device="cuda"),
             pos=torch.tensor([p - 1], dtype=torch.int32, device="cuda"),
             noise_out=torch.full(case["logits"].shape, sentinel, device="cuda"))
    ops.beam_select_gumbel(d["logits"], k, d["scores"], d["gumbels"], d["fin"], d["lens"], d["ys"], d["valid"], off,
                           d["kv_src"], d["done"], d["pos"], PAD, EOS, seed=seed, seed_dev=seed_dev,
                           noise_in=case["noise"].cuda() if noise_in else None, noise_out=d["noise_out"],
                           parent_i32=d["parent"])
    torch.cuda.synchronize()
    return {key: v.cpu() for key, v in d.items()}


@pytest.mark.parametrize("k,V", sbs_ref.kernel_cases())
def test_select_gumbel_matches_reference(k, V):
    n, T, off, p = sbs_ref.KERNEL_N, sbs_ref.KERNEL_T, sbs_ref.KERNEL_OFF, sbs_ref.KERNEL_P
    rows = n * k
    case = sbs_ref.kernel_case(k, V, PAD, EOS)
    (parent, tok, sc, gu, f2, l2), top, top_idx = sbs_ref.kernel_reference(case, k, PAD, EOS)
    tie = sbs_ref.near_tie(top)
    d = run_select(case, k, p, off)
    g_par, g_tok = d["parent"].view(n, k).long(), d["ys"][:, p].view(n, k)
    g_sc, g_gu = d["scores"].view(n, k), d["gumbels"].view(n, k)
    g_fin, g_len = d["fin"].view(n, k).bool(), d["lens"].view(n, k).long()
    assert not torch.isnan(g_sc).any() and not torch.isnan(g_gu).any()
    clear = ~tie.view(n, 1) & torch.isfinite(sc) & torch.isfinite(g_sc)
    if clear.any():
        rel = ((g_sc.double() - sc).abs() / sc.abs().clamp(min=1e-30))[clear].max().item()
        print(f"k={k} V={V}: near-tie samples {tie.tolist()}; worst relative score difference {rel:.3e}, worst Gumbel "
              f"difference {(g_gu.double() - gu).abs()[clear].max().item():.3e}")
    for s in range(n):
        if not tie[s]:
            assert torch.equal(g_par[s], parent[s]) and torch.equal(g_tok[s], tok[s]), (s, g_par[s], parent[s])
            assert torch.equal(g_fin[s], f2[s]) and torch.equal(g_len[s], l2[s])
            assert bool(d["done"][s]) == bool(f2[s].all())
            torch.testing.assert_close(g_sc[s], sc[s].float(), rtol=1e-6, atol=0)
            torch.testing.assert_close(g_gu[s].double(), gu[s], rtol=0, atol=GAP)
        else:
            # each child is a reference candidate whose value lies within GAP of the reference's value at that place
            for c in range(k):
                flat = int(g_par[s, c]) * V + int(g_tok[s, c])
                j = (top_idx[s] == flat).nonzero()
                assert j.numel() == 1, (s, c, flat, top_idx[s].tolist())
                assert abs(float(top[s, int(j)]) - float(top[s, c])) < GAP
                assert abs(float(g_gu[s, c]) - float(top[s, int(j)])) <= GAP
    # the variates used are the ones given: all V of every live beam's row, nothing for the others
    live = (~case["fin"] & (case["scores"] > -math.inf)).reshape(-1)
    assert torch.equal(d["noise_out"][live], case["noise"][live])
    assert bool((d["noise_out"][~live] == -7.5).all())
    # everything else of ys / valid untouched; the new slot's flag
    ys_want, valid_want = case["ys"].clone(), case["valid"].clone()
    ys_want[:, p] = g_tok.reshape(-1)
    valid_want[:, off + p] = (g_tok.reshape(-1) != PAD).to(torch.uint8)
    assert torch.equal(d["ys"], ys_want) and torch.equal(d["valid"], valid_want)
    # the map: each child takes its parent's row (before the call), plus its own new slot
    src_rows = (torch.arange(n).view(n, 1) * k + g_par).reshape(-1)
    want = case["kv_src"][src_rows].clone()
    want[:, off + p] = torch.arange(rows, dtype=torch.int32)
    assert torch.equal(d["kv_src"], want)
    # on the device's own output: each parent's best child carries the parent's Gumbel value bit for bit
    g0 = case["gumbels"].float()
    for s in range(n):
        seen = set()
        for c in range(k):
            b = int(g_par[s, c])
            if g_gu[s, c] == -math.inf or b in seen:
                continue
            seen.add(b)
            assert g_gu[s, c].view(torch.int32).item() == g0[s, b].view(torch.int32).item(), (s, c, b)
        assert bool((g_gu[s, :-1] >= g_gu[s, 1:]).all())
    # sample 1: every beam frozen, passed through in order; sample 4: <eos> certain for beam 0
    assert torch.equal(g_gu[1], g0[1]) and torch.equal(g_sc[1], case["scores"][1].float()) and bool(d["done"][1])
    assert bool((g_tok[1] == PAD).all()) and torch.equal(g_len[1], case["lens"][1])
    kids = [c for c in range(k) if int(g_par[4, c]) == 0]          # (a margin of 50 against variates below 17)
    assert not kids or (int(g_tok[4, kids[0]]) == EOS and bool(g_fin[4, kids[0]]))
    assert all(int(g_tok[3, c]) % 2 == 1 for c in range(k) if g_gu[3, c] > -math.inf)    # sample 3: even tokens at -inf


def test_select_gumbel_rejects_out_of_range_arguments():
    """gct_beam_select's refusals, and a missing Gumbel array: GCT_ERR_ARG before any launch."""
    L = ops._L()
    x = torch.zeros(8, 30, device="cuda")
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    b_ = buf.data_ptr()
    #    logits   V   n  k  scores fin lens parent ys ld_ys valid sb off kv_src ld_src T  done pos  pad  eos gumbels seed
    ok = [x.data_ptr(), 30, 2, 4, b_, b_, b_, b_, b_, 40, b_, 40, 0, b_, 40, 40, b_, b_, PAD, EOS, b_, 0, None, None, None,
          None]
    for i, bad in [(3, 0), (3, 17), (1, 3), (1, 65537), (15, 257), (14, 39), (11, 39), (9, 30), (18, 30), (18, -1),
                   (17, None), (20, None)]:
        args = list(ok)
        args[i] = bad
        assert L.gct_beam_select_gumbel(*args) == GCT_ERR_ARG, (i, bad)


# ----------------------------------------------------------------------------------------- the draw
def live_case(k, V, n=3):
    case = sbs_ref.kernel_case(k, V, PAD, EOS)
    case = {key: v[:n] if key in ("scores", "gumbels", "fin", "lens") else v[:n * k] for key, v in case.items()}
    case["fin"] = torch.zeros(n, k, dtype=torch.bool)
    case["scores"] = -torch.arange(1, n * k + 1, dtype=torch.float32).view(n, k)
    case["gumbels"] = case["scores"] + 0.5
    case["kv_src"] = case["kv_src"] % (n * k)
    return case


@pytest.mark.parametrize("V", [30, 301])
def test_draw_matches_the_host_restatement(V):
    k, n, off = 4, 3, sbs_ref.KERNEL_OFF
    seed, other = 0x1234_5678_9ABC_DEF, 77
    case = live_case(k, V, n)
    rows = np.arange(n * k)
    got = {}
    for p in (0, 17):
        out = run_select(case, k, p, off, seed=seed, noise_in=False)["noise_out"].double().numpy()
        got[p] = out
        want = sbs_ref.sbs_noise(seed, rows, p, V)
        np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-5)
        # a wrong output word or swapped counter words would be noticed
        assert np.abs(out - sbs_ref.sbs_noise(seed, rows, p, V, word_shift=1)).max() > 1.0
        assert np.abs(out - sbs_ref.sbs_noise(seed, rows, p, V, swap=True)).max() > 1.0
        u = sbs_ref.sbs_uniform(seed, rows, p, V)
        assert u.dtype == np.float32 and 0.0 < u.min() and u.max() < 1.0
    # another position, row or seed changes the noise
    assert not np.array_equal(got[0], got[17])
    assert not np.array_equal(got[17][0], got[17][1])
    out2 = run_select(case, k, 17, off, seed=other, noise_in=False)["noise_out"].double().numpy()
    assert not np.array_equal(out2, got[17])
    np.testing.assert_allclose(out2, sbs_ref.sbs_noise(other, rows, 17, V), rtol=1e-5, atol=1e-5)
    # seed_dev overrides seed
    sd = torch.tensor([seed], dtype=torch.int64, device="cuda")
    out3 = run_select(case, k, 17, off, seed=other, seed_dev=sd, noise_in=False)["noise_out"].double().numpy()
    assert np.array_equal(out3, got[17])


# ----------------------------------------------------------------------------------------- generate_sbs
def tiny_model(mtype, c2d=False, seed=1):
    """A tiny model that never draws <pad> as a token (score_tokens does not score pad columns) and ends some rows."""
    model = build(mtype, seed=seed, c2d=c2d)
    with torch.no_grad():
        model.out.bias[PAD] = -1e9
        model.out.bias[EOS] += 2.0
    return model


def inputs(mtype, c2d, n, seed, same_latent=False):
    nc = synthetic.n_conds(mtype)
    Le = 24 + (0 if c2d else nc)
    g = torch.Generator().manual_seed(seed)
    m = 1 if same_latent else n
    z = torch.randn(m, Le, TINY["latent_dim"], generator=g).repeat(n // m, 1, 1).cuda()
    dconds = torch.randn(m, nc, generator=g).repeat(n // m, 1).cuda() if nc else None
    lens = torch.randint(6, Le + 1, (m,), generator=g).repeat(n // m)
    src_mask = (torch.arange(Le)[None, :] < lens[:, None]).unsqueeze(1).cuda()
    if mtype in ("scavaetf", "pscavaetf"):
        pre = torch.randint(5, 30, (m, 5), generator=g).repeat(n // m, 1)
        ys0 = torch.cat([torch.full((n, 1), SOS), pre, torch.full((n, 1), synthetic.SEP_ID)], 1).cuda()
    else:
        ys0 = torch.full((n, 1), SOS, dtype=torch.long, device="cuda")
    return z, src_mask, dconds, ys0


def same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def models():
    return {("vaetf", False): tiny_model("vaetf"), ("pscavaetf", False): tiny_model("pscavaetf"),
            ("pvaetf", True): tiny_model("pvaetf", c2d=True)}


@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("mtype,c2d", [("vaetf", False), ("pscavaetf", False), ("pvaetf", True)])
def test_generate_sbs(models, mtype, c2d, k):
    model = models[(mtype, c2d)]
    n, steps = 6, 12
    z, src_mask, dconds, ys0 = inputs(mtype, c2d, n, seed=3)
    t0 = ys0.shape[1]
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=t0 + steps + 2, beams=k)
    out = kd.generate_sbs(ys0, k, steps, seed=5)
    assert isinstance(out, SbsSamples) and out.ys.shape[:2] == (n, k) and out.ys.dtype == torch.int64
    assert out.logp.shape == out.gumbel.shape == out.lengths.shape == (n, k)
    ys, lengths = out.ys.cpu(), out.lengths.cpu()
    assert torch.equal(ys[:, :, :t0], ys0.cpu().unsqueeze(1).expand(n, k, t0))
    assert bool(torch.isfinite(out.logp).all()) and bool(torch.isfinite(out.gumbel).all())
    assert bool((out.gumbel[:, :-1] >= out.gumbel[:, 1:]).all())               # drawing order
    for s in range(n):
        assert len({tuple(r) for r in ys[s].tolist()}) == k                    # pairwise distinct
        for i in range(k):
            gen = ys[s, i, t0:].tolist()
            L = int(lengths[s, i])
            assert L == (gen.index(EOS) + 1 if EOS in gen else steps - 1)      # lengths match the rows
            assert PAD not in gen[:L] and all(t == PAD for t in gen[L:])
    assert ys.shape[2] == t0 + int(lengths.max())
    # logp is the model's log-probability of the returned rows: pins the ancestry gather and the accumulation
    rep = lambda x: None if x is None else x.repeat_interleave(k, 0)       # noqa: E731
    flat = out.ys.reshape(n * k, -1)
    lp, tokens, _, _ = score_tokens(model, rep(z), rep(src_mask), rep(dconds), flat,
                                    prefix_lens=torch.full((n * k,), t0), pad_id=PAD)
    assert torch.equal(tokens.cpu().long(), lengths.reshape(-1))
    tol = 2e-4 * tokens.float() + 1e-4 * lp.abs()
    diff = (out.logp.reshape(-1) - lp).abs()
    print(f"{mtype} k={k}: worst logp difference {diff.max().item():.3e} (bound there {tol[diff.argmax()].item():.3e})")
    assert bool((diff <= tol).all())
    # seeds
    again = kd.generate_sbs(ys0, k, steps, seed=5)
    assert same(out, again)
    other = kd.generate_sbs(ys0, k, steps, seed=6)
    assert not same(out, other)
    # graph replay: bit for bit
    kd2 = KVDecoder(model, PAD, SOS, EOS)
    kd2.start(z, src_mask, dconds, max_total_len=t0 + steps + 2, beams=k)
    replayed = kd2.generate_sbs(ys0, k, steps, seed=5, use_graphs=True)
    assert "sbeam" in kd2.graphs
    assert same(out, replayed)


def test_generate_sbs_refuses():
    model = tiny_model("vaetf")
    z, src_mask, dconds, ys0 = inputs("vaetf", False, 4, seed=2)
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=20, beams=4)
    with pytest.raises(ValueError, match="mixed prefix"):
        kd.generate_sbs(ys0, 4, 8, prefix_lens=[1, 1, 1, 1])
    with pytest.raises(ValueError, match="prepared 4"):
        kd.generate_sbs(ys0, 2, 8)
    with pytest.raises(ValueError, match="rows"):
        kd.generate_sbs(ys0[:3], 4, 8)
    with pytest.raises(ValueError, match="at least 2"):
        kd.generate_sbs(ys0, 4, 1)
    with pytest.raises(ValueError, match="cache length"):
        kd.generate_sbs(ys0, 4, 40)


REF_SEED = 3          # the seed of the comparison below: with it at least half of the samples meet no near tie


def test_generate_sbs_matches_uncached_loop():
    """Sample by sample, up to the first step at which the reference's own candidates lie within GAP of each other."""
    mtype, n, k, steps = "pscavaetf", 16, 4, 12
    model = tiny_model(mtype)
    z, src_mask, dconds, ys0 = inputs(mtype, False, n, seed=8)
    t0, V = ys0.shape[1], model.out.weight.shape[0]
    rows = np.arange(n * k)
    noise_fn = lambda step: torch.from_numpy(sbs_ref.sbs_noise(REF_SEED, rows, t0 + step, V))     # noqa: E731
    root = sbs_root_gumbels(n, REF_SEED).double()
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=t0 + steps + 2, beams=k)

    def both(max_strlen):
        trace = []
        ref = reference_style_sbs_decode(model, z, src_mask, dconds, ys0, PAD, EOS, k, noise_fn, max_strlen, trace=trace,
                                         root=root.cuda())
        return kd.generate_sbs(ys0, k, max_strlen, seed=REF_SEED), ref, trace

    def compare(got, ref, s):
        L = max(got.ys.shape[2], ref.ys.shape[2])
        pad = lambda t: torch.nn.functional.pad(t, (0, L - t.shape[1]), value=PAD)    # noqa: E731
        assert torch.equal(pad(got.ys[s].cpu()), pad(ref.ys[s].cpu())), s
        assert torch.equal(got.lengths[s].cpu(), ref.lengths[s].cpu())
        lp, rlp = got.logp[s].cpu().double(), ref.logp[s].cpu().double()
        assert bool(((lp - rlp).abs() <= 2e-4 * ref.lengths[s].cpu().double() + 1e-4 * rlp.abs()).all()), (s, lp, rlp)
        torch.testing.assert_close(got.gumbel[s].cpu().double(), ref.gumbel[s].cpu().double(), rtol=0, atol=GAP)

    got, ref, trace = both(steps)
    first_tie = [next((t for t, top in enumerate(trace) if bool(sbs_ref.near_tie(top[s:s + 1]))), None) for s in range(n)]
    whole = [s for s in range(n) if first_tie[s] is None]
    print(f"seed {REF_SEED}: first near-tie step per sample {first_tie}")
    assert len(whole) >= n // 2
    for s in whole:
        compare(got, ref, s)
    for t in sorted({t for t in first_tie if t}):                  # t selections happen before the tie at step t
        got_t, ref_t, _ = both(t + 1)
        for s in range(n):
            if first_tie[s] == t:
                compare(got_t, ref_t, s)


def test_first_token_follows_the_softmax():
    """One latent 2 048 times, k = 1: the first generated token is an ordinary sample of the prefill's distribution."""
    from gct_plus_amd.Model.modules import get_trg_mask
    mtype, n = "vaetf", 2048
    model = tiny_model(mtype)
    z, src_mask, dconds, ys0 = inputs(mtype, False, n, seed=4, same_latent=True)
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=8, beams=1)
    out = kd.generate_sbs(ys0, 1, 3, seed=11)
    first = out.ys[:, 0, ys0.shape[1]].cpu()
    with torch.no_grad():
        logits = model.decode(ys0[:1], z[:1], src_mask[:1], get_trg_mask(ys0[:1], PAD, False, None), None)[0, -1]
    probs = torch.softmax(logits.double(), -1).cpu()
    counts = torch.bincount(first, minlength=probs.numel()).double()
    big = probs * n >= 5.0                                          # tokens expected under 5 times share one bin
    obs = torch.cat([counts[big], counts[~big].sum().view(1)])
    exp = torch.cat([probs[big], probs[~big].sum().view(1)]) * n
    if exp[-1] < 5.0:                                               # (the shared bin itself too thin: into the smallest)
        j = int(exp[:-1].argmin())
        obs[j] += obs[-1]
        exp[j] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    print(f"chi-square {chi2:.2f} over {obs.numel()} bins (bound {chi2_quantile_1e3(obs.numel() - 1):.2f})")
    assert obs.numel() >= 5 and chi2 < chi2_quantile_1e3(obs.numel() - 1)
    # k = 1 draws one ordinary sample per row: the rows differ, and the Gumbel value is the root's
    assert len(set(first.tolist())) > 3
    torch.testing.assert_close(out.gumbel[:, 0].cpu(), sbs_root_gumbels(n, 11))


# ----------------------------------------------------------------------------------------- the sampling front end
def make_sampler(decode_algo="stochastic_beam", **kw):
    from gct_plus_amd import data
    from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    strs = ["c1ccccc1<sep>" + s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    torch.manual_seed(4)
    model = model_dict["pscavaetf"](len(SRC), len(TRG), dropout=0.1, nconds=3, use_cond2lat=True, **TINY).cuda().eval()
    with torch.no_grad():
        model.out.bias[TRG.stoi["<pad>"]] = -1e9
        model.out.bias[TRG.stoi["<eos>"]] += 2.0
    kw.setdefault("beam_size", 4)
    return PscavaetfSampling(model, SRC, TRG, latent_dim=16, max_strlen=16, cond_dim=3, decode_algo=decode_algo,
                             toklen_data=[12, 14, 15, 18, 20, 16], **kw)


def sampler_inputs(sp, n):
    ys0 = sp.init_y(n, True, sp.smi_to_id("c1ccccc1"), True)
    z = torch.randn(n, 26, 16, generator=torch.Generator().manual_seed(9))
    return z, ys0, torch.ones(n, 1, 26, dtype=torch.bool), torch.full((n, 3), 0.3)


def test_sampler_decode_and_decode_unique():
    sp = make_sampler()
    n, k = 6, 4
    z, ys0, src_mask, dc = sampler_inputs(sp, n)
    sp.seed = 20
    first = sp.decode(z, ys0, src_mask, dc)
    assert sp.seed == 21 and first.dim() == 2 and first.shape[0] == n
    sp.seed = 20
    out = sp.decode_unique(z, ys0, src_mask, dc)
    assert sp.seed == 21 and out.ys.shape[:2] == (n, k) and torch.equal(first, out.ys[:, 0])
    # sample_smiles keeps its shapes; every string is the first draw
    sp.seed = 20
    smiles, toklen, gen = sp.sample_smiles(np.ones((n, 3)) * 0.3, "c1ccccc1", zs=z, transform=False)
    assert len(smiles) == n and smiles == [sp.id_to_smi(r[ys0.shape[1]:]) for r in first.cpu().numpy()]
    many = sp.sample_multiple_smiles(np.ones((n, 3)) * 0.3, ["c1ccccc1", "CC", "C1CCNCC1"] * 2, zs=z, transform=False)
    assert len(many[0]) == n
    # k of the call; any decode_algo has decode_unique
    sp2 = make_sampler("multinomial")
    sp2.seed = 20
    out2 = sp2.decode_unique(z, ys0, src_mask, dc, k=4)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    assert sp2.decode_unique(z, ys0, src_mask, dc, k=2).ys.shape[:2] == (n, 2)


def test_decode_unique_rows_feed_a_policy_gradient_step():
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import reinforce_step
    from gct_plus_amd.decode import sbs_importance_weights
    sp = make_sampler("multinomial")
    n, k = 5, 4
    z, ys0, src_mask, dc = sampler_inputs(sp, n)
    out, rows = sp.decode_unique(z, ys0, src_mask, dc, k=k, return_rows=True)
    assert isinstance(rows, DecodedRows) and rows.ys.shape == (n * k, out.ys.shape[2])
    assert torch.equal(rows.ys, out.ys.reshape(n * k, -1))             # sample-major; rows past <eos> are pad already
    assert torch.equal(rows.zs, z.cuda().repeat_interleave(k, 0)) and rows.dconds.shape == (n * k, 3)
    assert rows.src_mask.shape == (n * k, 1, 26) and rows.prefix_lens.tolist() == [ys0.shape[1]] * (n * k)
    with torch.no_grad():
        sc = sp.logp(*rows)
    tol = 2e-4 * sc.tokens.float() + 1e-4 * sc.logp.abs()
    assert bool(((sc.logp - out.logp.reshape(-1)).abs() <= tol).all())
    assert torch.equal(sc.tokens.cpu().long(), out.lengths.reshape(-1).cpu())
    w, wn = sbs_importance_weights(out.logp, out.gumbel)
    assert w.shape == (n, k) and bool(torch.isfinite(w).all()) and bool((w[:, -1] == 0).all())
    start = {key: p.detach().clone() for key, p in sp.model.named_parameters()}
    opt = FusedAdam(sp.model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9, model=sp.model)
    stats = reinforce_step(sp, opt, rows, out.lengths.reshape(-1).float())
    assert stats["tokens"] == int(out.lengths.sum()) and math.isfinite(stats["loss"])
    assert any(not torch.equal(p.detach(), start[key]) for key, p in sp.model.named_parameters()
               if key.startswith("decoder."))


def test_sampler_refusals_come_before_device_work():
    for kw in (dict(well_formed=True), dict(with_logp=True), dict(stream_rows=8), dict(top_k=5), dict(top_p=0.9),
               dict(temperature=0.7), dict(beam_size=17), dict(beam_size=0)):
        with pytest.raises(ValueError):
            make_sampler(**kw)
    sp = make_sampler()
    z, ys0, src_mask, dc = sampler_inputs(sp, 4)
    seed = sp.seed
    with pytest.raises(ValueError, match="stochastic_beam"):
        sp.decode(z, ys0, src_mask, dc, return_rows=True)
    with pytest.raises(ValueError, match="one length"):
        sp.decode(z, ys0, src_mask, dc, prefix_lens=[3, 3, 3, 3])
    with pytest.raises(ValueError, match="stochastic_beam"):
        sp.interpolate_smiles(["CCO"], ["CCN"], scaffolds0=["CC"], scaffolds1=["CC"], props0=np.zeros((1, 3)),
                              props1=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="stochastic_beam"):
        sp.reconstruct_smiles(["CCO"], ["CC"], np.zeros((1, 3)))
    with pytest.raises(ValueError, match="stochastic_beam"):
        sp.sample_multiple_smiles(np.zeros((2, 3)), ["CC", "CCC"], return_rows=True)
    with pytest.raises(ValueError):
        sp.decode_unique(z, ys0, src_mask, dc, k=17)
    assert sp.seed == seed and sp.kv._shape is None                 # nothing ran
    wf = make_sampler("multinomial", well_formed=True)
    with pytest.raises(ValueError, match="well_formed"):
        wf.decode_unique(z, ys0, src_mask, dc)
    assert wf.kv._shape is None
