"""Top-k / nucleus / temperature sampling on the gfx950 kernel (gct_select_token with a GctSampleFilter): the filtered
distribution against decode.sample_filter_reference, the draws, the neutral settings against the plain draw, and the
decoder end to end -- uniform and mixed prefixes, eager and graph replay -- plus the sampler front end."""
import numpy as np
import pytest
import torch

from gct_plus_amd import ops, synthetic
from gct_plus_amd.decode import sample_filter_reference
from tests.test_mixed_scaffold_decode_gpu import TINY, build, mixed_prefixes, upto_eos

pytestmark = pytest.mark.gpu
EOS, PAD, SOS = synthetic.EOS_ID, synthetic.PAD_ID, synthetic.SOS_ID
MTYPES = ["vaetf", "pvaetf", "scavaetf", "pscavaetf"]


def select(logits, filt=None, seed=123, mode=1, probs=True):
    """One select_token launch at position 1 of fresh buffers: (tokens [n], probs [n, V] or None)."""
    n, V = logits.shape
    ys = torch.zeros(n, 2, dtype=torch.int64, device="cuda")
    valid = torch.zeros(n, 2, dtype=torch.uint8, device="cuda")
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pr = torch.full((n, V), -1.0, device="cuda") if probs else None
    fd = None if filt is None else ops.sample_filter_settings(*filt, V).cuda()
    ops.select_token(logits, ys, 1, valid, done, mode, PAD, EOS, seed=seed, probs_out=pr, filt_dev=fd)
    tok = ys[:, 1].cpu()
    assert torch.equal(valid[:, 1].cpu().bool(), tok != PAD)
    assert torch.equal(done.cpu().bool(), tok == EOS)
    return tok, None if pr is None else pr.cpu()


def mass_above(s):
    """fp64 mass of the tokens with a strictly larger s, per token (sorted cumulative sums, O(V log V) per row)."""
    s = s.double().contiguous()
    V = s.shape[-1]
    asc = s.sort(-1).values
    larger = V - torch.searchsorted(asc, s, right=True)
    top = asc.flip(-1).cumsum(-1)
    return torch.where(larger > 0, top.gather(-1, (larger - 1).clamp(min=0)), torch.zeros_like(s))


def rows_away_from_the_boundary(V, k, T, p, n, seed):
    """n logit rows [n, V] none of whose nucleus masses lies within 1e-5 of p (the device sums in another order); any
    rows when the nucleus is off (p = 1)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(50):
        x = torch.randn(4 * n, V, generator=g) * 2
        if p >= 1:
            return x[:n].contiguous()
        s = sample_filter_reference(x, top_k=k, temperature=T)                 # the top-k stage, normalised
        out.append(x[((mass_above(s) - p).abs() > 1e-5).all(-1)])
        if sum(len(o) for o in out) >= n:
            return torch.cat(out)[:n].contiguous()
    raise AssertionError(f"no {n} rows away from the nucleus boundary {p} (V {V}, k {k}, T {T})")


@pytest.mark.parametrize("V", [30, 64, 65, 1024])
def test_filtered_probabilities_match_the_rules(V):
    n = 64
    for T in (0.7, 1.0, 1.5):
        for k in (1, 4, V):
            for p in (0.5, 0.9, 1.0):
                x = rows_away_from_the_boundary(V, k, T, p, n, seed=V * 7 + k)
                tok, pr = select(x.cuda(), (k, p, T))
                want = sample_filter_reference(x, top_k=k, top_p=p, temperature=T)
                err = float((pr.double() - want.double()).abs().max())
                assert err < 1e-6, (V, T, k, p, err)
                assert bool((want[torch.arange(n), tok] > 0).all()), (V, T, k, p)   # never a token of weight 0


@pytest.mark.parametrize("V,filt", [(30, (8, 0.9, 0.8)), (30, (None, 0.7, 1.3)), (200, (12, 0.95, 0.9)),
                                    (40, (3, None, 1.0))])
def test_draw_frequencies_follow_the_filtered_distribution(V, filt):
    n = 8192
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(V)) * 1.5
    want = sample_filter_reference(x, *filt)[0].double()
    tok, pr = select(x.repeat(n, 1).cuda().contiguous(), filt, seed=99)
    assert torch.allclose(pr[0].double(), want, atol=1e-6, rtol=0)
    assert bool((want[tok] > 0).all())                                          # weight-0 tokens are never drawn
    freq = torch.bincount(tok, minlength=V).double() / n
    assert float((freq - want).abs().max()) < 0.03


@pytest.mark.parametrize("V", [30, 64, 100, 1024])
def test_neutral_settings_draw_as_the_plain_path(V):
    n = 4096
    x = (torch.randn(n, V, generator=torch.Generator().manual_seed(V)) * 2).cuda()
    t_plain, p_plain = select(x, None, seed=7)
    t_filt, p_filt = select(x, (V, 1.0, 1.0), seed=7)
    assert torch.equal(t_plain, t_filt)
    assert torch.equal(p_plain, p_filt)


def test_filter_limits():
    x = torch.randn(8, 1025, device="cuda")
    with pytest.raises(ops._lib.GctError):
        select(x, (4, 0.9, 1.0))
    x = torch.randn(8, 30, device="cuda")
    with pytest.raises(ops._lib.GctError):                                     # multinomial only
        select(x, (4, 0.9, 1.0), mode=0)


def start_decoder(model, n, Le, nc, seed, total=64):
    from gct_plus_amd.decode import KVDecoder
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g).cuda()
    dconds = torch.randn(n, nc, generator=g).cuda() if nc else None
    klen = torch.randint(6, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1).cuda()
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=total)
    return kd, z, src_mask, dconds


@pytest.mark.parametrize("mtype", MTYPES)
@pytest.mark.parametrize("graphs", [False, True])
def test_tiny_top_p_decodes_greedily(mtype, graphs):
    """top_p = 1e-9 leaves only the argmax: the filtered multinomial decode equals greedy and the un-cached loop
    (uniform prefixes), and greedy on mixed prefixes."""
    from gct_plus_amd.decode import FILTERED, generated_tokens, reference_style_decode
    model = build(mtype, seed=11)
    nc = synthetic.n_conds(mtype)
    n, Le = 12, 20 + nc
    kd, z, src_mask, dconds = start_decoder(model, n, Le, nc, seed=5)
    ys0 = torch.full((n, 1), SOS, dtype=torch.long, device="cuda")
    ys_f = kd.generate(ys0, 24, algo="multinomial", seed=4, top_p=1e-9, use_graphs=graphs)
    kd.start(z, src_mask, dconds, max_total_len=64)
    ys_g = kd.generate(ys0, 24, use_graphs=graphs)
    ref = reference_style_decode(model, z, src_mask, dconds, ys0, PAD, EOS, 24)
    assert torch.equal(ys_f, ys_g) and torch.equal(ys_f, ref)
    g = torch.Generator().manual_seed(3)
    ys0m, lens = mixed_prefixes([2, 6, 4], 4, g)
    gens = []
    for kw in (dict(algo="multinomial", seed=4, top_p=1e-9, top_k=3, temperature=0.9), dict()):
        kd.start(z, src_mask, dconds, max_total_len=64)
        ys = kd.generate(ys0m.cuda(), 20, use_graphs=graphs, prefix_lens=lens, **kw).cpu()
        gens.append(generated_tokens(ys, lens))
    assert torch.equal(gens[0], gens[1])
    if graphs:
        assert (FILTERED, "mixed") in kd.graphs


def test_filtered_mixed_batch_matches_uniform_rows():
    """As test_mixed_prefixes_multinomial_matches_uniform_rows, through the filter: the rows of scaffold A in a mixed
    batch and in a batch of scaffold A everywhere draw with the same keys from the same filtered distribution."""
    from gct_plus_amd.decode import KVDecoder, generated_tokens
    model = build("scavaetf", seed=5)
    g = torch.Generator().manual_seed(13)
    ys0, lens = mixed_prefixes([6, 3, 11, 8], 64, g)
    n, Le = ys0.shape[0], 30
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g).cuda()
    src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
    rows = (lens == 6).nonzero().view(-1)
    ysu = ys0[rows[0]].view(1, -1)[:, :6].repeat(n, 1)
    filt = dict(top_k=4, top_p=0.9, temperature=0.8)
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, None, max_total_len=64)
    gm = generated_tokens(kd.generate(ys0.cuda(), 40, algo="multinomial", seed=77, prefix_lens=lens, **filt).cpu(), lens)
    kd.start(z, src_mask, None, max_total_len=64)
    yu = kd.generate(ysu.cuda(), 40, algo="multinomial", seed=77, **filt).cpu()
    same = sum(upto_eos(gm[r]) == upto_eos(yu[r, 6:]) for r in rows.tolist())
    assert same >= 0.99 * len(rows), (same, len(rows))
    kd.start(z, src_mask, None, max_total_len=64)
    yp = kd.generate(ysu.cuda(), 40, algo="multinomial", seed=77).cpu()
    assert not torch.equal(yp, yu)                                              # the filter does change the draws


def test_graphs_serve_any_settings():
    """One geometry, two filtered calls with different settings: replayed ids equal eager launches, the filtered mode
    captures one graph, and plain greedy / multinomial calls afterwards equal a fresh decoder's."""
    from gct_plus_amd.decode import FILTERED, KVDecoder
    model = build("pscavaetf", seed=6)
    n, Le = 16, 22
    kd, z, src_mask, dconds = start_decoder(model, n, Le, 3, seed=9)
    eager = KVDecoder(model, PAD, SOS, EOS)
    ys0 = torch.full((n, 1), SOS, dtype=torch.long, device="cuda")

    def run(dec, graphs, **kw):
        dec.start(z, src_mask, dconds, max_total_len=64)
        return dec.generate(ys0, 30, seed=21, use_graphs=graphs, **kw)

    run(kd, True)                                                               # greedy graph
    assert len(kd.graphs) == 1
    outs = []
    for filt in (dict(top_k=3, temperature=0.7), dict(top_p=0.8, temperature=1.4)):
        got = run(kd, True, algo="multinomial", **filt)
        assert torch.equal(got, run(eager, False, algo="multinomial", **filt)), filt
        assert len(kd.graphs) == 2 and FILTERED in kd.graphs
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])
    for algo in ("greedy", "multinomial"):
        fresh = KVDecoder(model, PAD, SOS, EOS)
        assert torch.equal(run(kd, True, algo=algo), run(fresh, True, algo=algo)), algo


def make_sampler(mtype, **kw):
    from gct_plus_amd import data
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    sep = mtype in ("scavaetf", "pscavaetf")
    strs = [("c1ccccc1<sep>" + s) if sep else s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, sep), data.Vocab.build(strs, True, sep)
    nc = synthetic.n_conds(mtype)
    torch.manual_seed(4)
    model = model_dict[mtype](len(SRC), len(TRG), dropout=0.1, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
    return get_sampler(mtype, model, SRC, TRG, latent_dim=16, max_strlen=24, cond_dim=nc,
                       toklen_data=[12, 14, 15, 18, 20, 16], **kw)


@pytest.mark.parametrize("mtype", MTYPES)
def test_sample_smiles_with_top_k(mtype):
    sp = make_sampler(mtype, decode_algo="multinomial", top_k=4, use_graphs=True)
    n = 6
    args = {"vaetf": (n,), "pvaetf": (np.zeros((n, 3)),), "scavaetf": (n, "c1ccccc1"),
            "pscavaetf": (np.ones((n, 3)) * 0.3, "c1ccccc1")}[mtype]
    kw = {} if synthetic.n_conds(mtype) == 0 else {"transform": False}
    smiles, toklen, toklen_gen = sp.sample_smiles(*args, **kw)
    assert len(smiles) == n and all(isinstance(s, str) for s in smiles) and len(toklen) == len(toklen_gen) == n
    assert sp.kv.filt.tolist()[0] == 4


@pytest.mark.parametrize("mtype", ["scavaetf", "pscavaetf"])
def test_sample_multiple_smiles_tiny_top_p_is_greedy(mtype):
    scaffolds = ["c1ccccc1", "C1CCNCC1", "c1ccccc1", "CC", "O=C1CCCN1", "CC"]
    n = len(scaffolds)
    g = torch.Generator().manual_seed(2)
    toklen = torch.randint(8, 20, (n,), generator=g).tolist()
    z = torch.randn(n, 40, 16, generator=g)
    out = []
    for kw in (dict(decode_algo="multinomial", top_p=1e-9), dict(decode_algo="greedy")):
        sp = make_sampler(mtype, **kw)
        if mtype == "pscavaetf":
            dconds = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).numpy()
            out.append(sp.sample_multiple_smiles(dconds, scaffolds, zs=z, toklen=toklen, transform=False)[0])
        else:
            out.append(sp.sample_multiple_smiles(scaffolds, zs=z, toklen=toklen)[0])
    assert out[0] == out[1]
