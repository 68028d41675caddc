"""Mixed-scaffold batches on the KV-cached decoder (KVDecoder.generate(prefix_lens=), sample_multiple_smiles): every
row of a batch of prefixes of different lengths must decode exactly what it decodes alone -- against the oracle's loop,
the un-cached loop, the cond2dec loop, the multinomial draws of a uniform batch and the per-scaffold sampler."""
import numpy as np
import pytest
import torch

from gct_plus_amd import data, synthetic

pytestmark = pytest.mark.gpu
TINY = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
EOS, PAD, SOS = synthetic.EOS_ID, synthetic.PAD_ID, synthetic.SOS_ID


def build(mtype, full=False, seed=1, **extra):
    from gct_plus_amd.Model import model_dict
    vs, vt = synthetic.vocab_sizes(mtype)
    kw = dict(N=6, d_model=512, dff=2048, h=8, latent_dim=128) if full else TINY
    nc = extra.pop("nconds", synthetic.n_conds(mtype))
    torch.manual_seed(seed)
    return model_dict[mtype](vs, vt, dropout=0.1, nconds=nc, **dict(dict(use_cond2lat=True), **extra),
                             **kw).cuda().eval()


def mixed_prefixes(lengths, per, g):
    """len(lengths) scaffold-style prefixes (<sos> tokens <sep>) of the given lengths, `per` rows each, rows
    interleaved (row r uses prefix r % len(lengths)): (ys0 [n, t0_max] right-padded with pad, lens [n])."""
    k = len(lengths)
    pres = [torch.cat([torch.tensor([SOS]), torch.randint(5, 30, (t - 2,), generator=g), torch.tensor([4])])
            if t >= 2 else torch.tensor([SOS]) for t in lengths]
    n = k * per
    lens = torch.tensor([lengths[r % k] for r in range(n)])
    ys0 = torch.full((n, max(lengths)), PAD, dtype=torch.long)
    for r in range(n):
        ys0[r, :lens[r]] = pres[r % k]
    return ys0, lens


def upto_eos(ids):
    ids = [int(t) for t in ids]
    return ids[:ids.index(EOS) + 1] if EOS in ids else ids


def groups(lens):
    return [(int(t), (lens == t).nonzero().view(-1)) for t in torch.unique(lens).tolist()]


def decode_mixed(model, z, src_mask, dconds, ys0, lens, max_strlen, graphs=False, eos=EOS, algo="greedy", seed=0,
                 kd=None, total=None):
    from gct_plus_amd.decode import KVDecoder, generated_tokens
    kd = kd or KVDecoder(model, PAD, SOS, eos)
    kd.start(z.cuda(), src_mask.cuda(), None if dconds is None else dconds.cuda(),
             max_total_len=total or ys0.shape[1] + max_strlen + 8)
    ys = kd.generate(ys0.cuda(), max_strlen, use_graphs=graphs, prefix_lens=lens, algo=algo, seed=seed).cpu()
    assert torch.equal(ys[:, :ys0.shape[1]][ys0 != PAD], ys0[ys0 != PAD])         # prefixes intact
    return ys, generated_tokens(ys, lens)


@pytest.mark.parametrize("mtype", ["scavaetf", "pscavaetf"])
def test_mixed_prefixes_vs_oracle_per_length_group(mtype):
    """Tiny config: four prefix lengths in one batch against the oracle's greedy loop run once per length group.  Ids
    must be equal up to each row's first <eos>; a difference is allowed only at an fp32 near-tie of the oracle (top-2
    logit gap < 1e-4 at the first differing step)."""
    from oracle import gct_oracle as O
    model = build(mtype)
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    g = torch.Generator().manual_seed(41)
    ys0, lens = mixed_prefixes([3, 9, 5, 14], 3, g)
    n, Le = ys0.shape[0], 24 + nc
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    dconds = torch.randn(n, nc, generator=g) if nc else None
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    _, gen = decode_mixed(model, z, src_mask, dconds, ys0, lens, 30)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY)
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    for t0, idx in groups(lens):
        trace = []
        ref = O.greedy_decode(P, cfg, z[idx], src_mask[idx], None if dconds is None else dconds[idx], SOS, EOS, PAD,
                              max_strlen=30, ys0=ys0[idx, :t0], trace=trace)
        for j, r in enumerate(idx.tolist()):
            a, b = upto_eos(gen[r]), upto_eos(ref[j, t0:])
            if a == b:
                continue
            t = next(i for i, (x, y) in enumerate(zip(a + [None], b + [None])) if x != y)
            top2 = trace[t][j].topk(2).values
            assert float(top2[0] - top2[1]) < 1e-4, (r, t0, t, top2.tolist(), a, b)


@pytest.mark.parametrize("graphs", [False, True])
def test_mixed_prefixes_full_size_pscavaetf_vs_uncached_groups(graphs):
    """Full size, 64 rows, 8 scaffold prefixes of 3..30 tokens, ragged source masks: each row equals (up to its first
    <eos>) the un-cached reference-style loop run on its own length group with the same z / dconds."""
    from gct_plus_amd.decode import reference_style_decode
    mtype = "pscavaetf"
    model = build(mtype, full=True, seed=3)
    nc = synthetic.n_conds(mtype)
    g = torch.Generator().manual_seed(17)
    ys0, lens = mixed_prefixes([3, 30, 7, 12, 4, 21, 16, 9], 8, g)
    n, Le = ys0.shape[0], 40 + nc
    z = torch.randn(n, Le, 128, generator=g)
    dconds = torch.randn(n, nc, generator=g)
    klen = torch.randint(10, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    _, gen = decode_mixed(model, z, src_mask, dconds, ys0, lens, 40, graphs=graphs)
    for t0, idx in groups(lens):
        ref = reference_style_decode(model, z[idx].cuda(), src_mask[idx].cuda(), dconds[idx].cuda(),
                                     ys0[idx, :t0].cuda(), PAD, EOS, 40).cpu()
        for j, r in enumerate(idx.tolist()):
            assert upto_eos(gen[r]) == upto_eos(ref[j, t0:]), (r, t0)


@pytest.mark.parametrize("graphs", [False, True])
def test_mixed_prefixes_cond2dec(graphs):
    """-use_cond2dec: the n_c condition rows sit in front of every prefix (positions off + p); mixed prefixes against
    the un-cached cond2dec loop (test_decode_gpu.test_kv_decode_use_cond2dec's) run per length group."""
    from gct_plus_amd.Model.modules import get_trg_mask
    model = build("pvaetf", seed=2, nconds=3, use_cond2dec=True, use_cond2lat=False)
    g = torch.Generator().manual_seed(8)
    ys0, lens = mixed_prefixes([1, 4, 2, 6], 3, g)
    n, Le = ys0.shape[0], 19
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    dconds = torch.randn(n, 3, generator=g)
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    _, gen = decode_mixed(model, z, src_mask, dconds, ys0, lens, 25, graphs=graphs, eos=-1)
    assert gen.shape == (n, 24)
    for t0, idx in groups(lens):
        zz, mm, dd = z[idx].cuda(), src_mask[idx].cuda(), dconds[idx].cuda()
        ys = ys0[idx, :t0].cuda()
        for _ in range(24):
            tm = get_trg_mask(ys, PAD, True, dd)
            logits = model.decode(ys, zz, mm, tm, dd)[:, 3:]
            ys = torch.cat([ys, logits[:, -1].argmax(-1)[:, None]], dim=1)
        assert torch.equal(gen[idx], ys[:, t0:].cpu()), t0


def test_mixed_prefixes_multinomial_matches_uniform_rows():
    """Same seed, same z: the rows of scaffold A in a mixed batch and the same rows of a batch that holds scaffold A
    everywhere see the same first-step probabilities (to 1e-6) and draw the same Philox keys (row, token position), so
    (almost) all of them produce the same ids."""
    from gct_plus_amd.decode import KVDecoder, check_prefix_lens
    mtype = "scavaetf"
    model = build(mtype, seed=5)
    g = torch.Generator().manual_seed(13)
    ys0, lens = mixed_prefixes([6, 3, 11, 8], 64, g)
    n, Le = ys0.shape[0], 30
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g).cuda()
    src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
    rows = (lens == 6).nonzero().view(-1)                                        # scaffold A: 6 tokens, rows 0, 4, ...
    ysu = ys0[rows[0]].view(1, -1)[:, :6].repeat(n, 1)
    kd = KVDecoder(model, PAD, SOS, EOS)
    probs = []
    for y, pl in ((ys0, lens), (ysu, None)):
        kd.start(z, src_mask, None, max_total_len=64)
        probs.append(torch.softmax(kd.prefill(y.cuda(), check_prefix_lens(pl, n, y.shape[1])).double(), -1)[rows].cpu())
    assert torch.allclose(probs[0], probs[1], atol=1e-6, rtol=0)
    _, gm = decode_mixed(model, z, src_mask, None, ys0, lens, 40, algo="multinomial", seed=77, kd=kd)
    kd.start(z, src_mask, None, max_total_len=64)
    yu = kd.generate(ysu.cuda(), 40, algo="multinomial", seed=77).cpu()
    same = sum(upto_eos(gm[r]) == upto_eos(yu[r, 6:]) for r in rows.tolist())
    assert same >= 0.99 * len(rows), (same, len(rows))


def test_uniform_lengths_and_uniform_after_mixed_unchanged():
    """prefix_lens all equal to the width gives exactly the call without it; a uniform generate after a mixed one on the
    same decoder (and graphs dict) equals a fresh decoder's; the two kinds of step keep graphs of their own."""
    from gct_plus_amd.decode import KVDecoder
    model = build("pscavaetf", seed=6)
    g = torch.Generator().manual_seed(29)
    ys0, lens = mixed_prefixes([5, 8, 3], 4, g)
    n, Le = ys0.shape[0], 22
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g).cuda()
    dconds = torch.randn(n, 3, generator=g).cuda()
    src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
    yu0 = ys0[:, :3].cuda()                                                      # every row has >= 3 real tokens
    for graphs in (False, True):
        for algo in ("greedy", "multinomial"):
            fresh = KVDecoder(model, PAD, SOS, EOS)
            fresh.start(z, src_mask, dconds, max_total_len=64)
            want = fresh.generate(yu0, 30, algo=algo, seed=3, use_graphs=graphs)
            kd = KVDecoder(model, PAD, SOS, EOS)
            kd.start(z, src_mask, dconds, max_total_len=64)
            same_w = kd.generate(yu0, 30, algo=algo, seed=3, use_graphs=graphs, prefix_lens=torch.full((n,), 3))
            assert torch.equal(same_w, want), (graphs, algo)
            decode_mixed(model, z, src_mask, dconds, ys0, lens, 30, graphs=graphs, algo=algo, seed=3, kd=kd, total=64)
            kd.start(z, src_mask, dconds, max_total_len=64)
            again = kd.generate(yu0, 30, algo=algo, seed=3, use_graphs=graphs)
            assert torch.equal(again, want), (graphs, algo)
            if graphs:
                mode = {"greedy": 0, "multinomial": 1}[algo]
                assert mode in kd.graphs and (mode, "mixed") in kd.graphs


def make_sampler(decode_algo):
    from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    strs = ["c1ccccc1<sep>" + s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    torch.manual_seed(4)
    model = model_dict["pscavaetf"](len(SRC), len(TRG), dropout=0.1, nconds=3, use_cond2lat=True, **TINY).cuda().eval()
    return PscavaetfSampling(model, SRC, TRG, latent_dim=16, max_strlen=24, cond_dim=3, decode_algo=decode_algo,
                             toklen_data=[12, 14, 15, 18, 20, 16], beam_size=3)


@pytest.mark.parametrize("algo,graphs", [("greedy", False), ("greedy", True), ("beam", False)])
def test_sample_multiple_smiles_equals_per_scaffold_calls(algo, graphs):
    sp = make_sampler(algo)
    sp.use_graphs = graphs
    scaffolds = ["c1ccccc1", "C1CCNCC1", "c1ccccc1", "CC", "c1ccc2ccccc2c1", "C1CCNCC1", "O=C1CCCN1", "CC"]
    n = len(scaffolds)
    g = torch.Generator().manual_seed(2)
    toklen = torch.randint(8, 20, (n,), generator=g).tolist()
    z = torch.randn(n, 40, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    smiles, tl, tl_gen = sp.sample_multiple_smiles(dconds, scaffolds, zs=z, toklen=toklen, transform=False)
    assert tl == toklen and len(smiles) == len(tl_gen) == n
    want = [None] * n
    for s in dict.fromkeys(scaffolds):
        idx = [r for r in range(n) if scaffolds[r] == s]
        extra = len(sp.smi_to_id(s)) + 1
        tk = [toklen[r] for r in idx]
        out, _, _ = sp.sample_smiles(dconds[idx], s, zs=z[idx, :extra + max(tk)], toklen=tk, transform=False)
        for r, smi in zip(idx, out):
            want[r] = smi
    assert smiles == want


def test_mixed_prefix_limits():
    from gct_plus_amd.decode import KVDecoder
    model = build("pscavaetf", seed=7)
    n, Le = 4, 12
    z = torch.randn(n, Le, TINY["latent_dim"]).cuda()
    src_mask = torch.ones(n, 1, Le, dtype=torch.bool, device="cuda")
    dconds = torch.randn(n, 3).cuda()
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, src_mask, dconds, max_total_len=60)
    ys0 = torch.full((n, 6), SOS, dtype=torch.long, device="cuda")
    for bad in (torch.tensor([0, 6, 6, 6]), torch.tensor([7, 6, 6, 6]), torch.tensor([6, 6, 6]),
                torch.tensor([2.0, 6, 6, 6])):
        with pytest.raises(ValueError):
            kd.generate(ys0, 20, prefix_lens=bad)
    kd.start(z, src_mask, dconds, max_total_len=200)
    long0 = torch.full((n, 150), 7, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="positional table"):                   # 150 + 79 tokens > 200 PE rows
        kd.generate(long0, 80, prefix_lens=torch.tensor([3, 150, 40, 9]))
    kd.start(z, src_mask, dconds, max_total_len=60, beams=2)
    with pytest.raises(ValueError):
        kd.generate_beam(ys0, 2, 20, prefix_lens=torch.tensor([2, 6, 6, 6]))
