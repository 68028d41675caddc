"""Beam-search decoding on the device: gct_beam_select and gct_attn_decode_beam against the host statement of the rules
(decode.beam_step_reference) and fp64 attention; KVDecoder.generate_beam against the un-cached reference-style loop,
greedy decode and the CPU oracle; the sampling front end with decode_algo="beam"."""
import math

import pytest
import torch

from gct_plus_amd import ops, synthetic
from gct_plus_amd.decode import (BEAM_ALPHA, KVDecoder, beam_candidates, beam_finalize, beam_init, beam_log_softmax,
                                 beam_step_reference, reference_style_beam_decode)

pytestmark = pytest.mark.gpu
TINY = dict(N=2, d_model=64, dff=128, h=4, latent_dim=16)
PAD, EOS = synthetic.PAD_ID, synthetic.EOS_ID
GCT_ERR_ARG = -1
GAP = 1e-4                     # near-tie rule: fp32 candidates closer than this may order either way


def build(mtype, full=False, seed=1, c2d=False):
    from gct_plus_amd.Model import model_dict
    vs, vt = synthetic.vocab_sizes(mtype)
    kw = dict(N=6, d_model=512, dff=2048, h=8, latent_dim=128) if full else TINY
    torch.manual_seed(seed)
    return model_dict[mtype](vs, vt, dropout=0.1, nconds=synthetic.n_conds(mtype), use_cond2lat=not c2d,
                             use_cond2dec=c2d, **kw).cuda().eval()


# ----------------------------------------------------------------------------------------- gct_beam_select
@pytest.mark.parametrize("k", [1, 2, 5, 16])
@pytest.mark.parametrize("V", [30, 64, 100, 4096])
def test_beam_select_matches_reference(k, V):
    if k > V:
        pytest.skip("k > V")
    g = torch.Generator().manual_seed(1000 * k + V)
    n, T, off, p = 5, 40, 3, 17                          # p = index of the token chosen now (pos = p - 1)
    rows = n * k
    logits = torch.randn(rows, V, generator=g) * 3
    scores = -torch.rand(n, k, generator=g) * 20
    fin = torch.rand(n, k, generator=g) < 0.3
    lens = torch.randint(1, 15, (n, k), generator=g)
    scores0, fin0, lens0 = beam_init(1, k)             # sample 0: the first expansion after the prefill
    scores[0], fin[0], lens[0] = scores0[0], fin0[0], lens0[0]
    fin[1] = True                                      # sample 1: every beam finished
    if k >= 2:
        # sample 2: ties within a row (tokens 5..8) and across two identical beams
        r = 2 * k
        logits[r] = -1e4
        logits[r, 5:9] = 1.0
        logits[r + 1] = logits[r]
        scores[2, :2], fin[2, :2] = -1.0, False
        scores[2, 2:] -= 3.0
        # sample 4: a frozen beam tying exactly with a live beam's best (the log-softmax of a one-hot row is exact)
        r = 4 * k
        logits[r] = -1e4
        logits[r, 5] = 2.0
        scores[4, :2] = -0.5
        fin[4, 0], fin[4, 1] = False, True
        scores[4, 2:] -= 3.0
    logits[3 * k, EOS] = 50.0                          # sample 3: <eos> certainly chosen for beam 0 (if live)
    ys = torch.randint(0, V, (rows, T), generator=g)
    valid = torch.randint(0, 2, (rows, T), generator=g).to(torch.uint8)
    kv_src = torch.randint(0, rows, (rows, T), generator=g).to(torch.int32)

    d = dict(logits=logits.cuda(), scores=scores.reshape(-1).cuda(), fin=fin.reshape(-1).to(torch.uint8).cuda(),
             lens=lens.reshape(-1).to(torch.int32).cuda(), ys=ys.cuda(), valid=valid.cuda(), kv_src=kv_src.cuda(),
             done=torch.zeros(n, dtype=torch.uint8, device="cuda"), parent=torch.full((rows,), -7, dtype=torch.int32,
                                                                                        device="cuda"),
             pos=torch.tensor([p - 1], dtype=torch.int32, device="cuda"))
    ops.beam_select(d["logits"], k, d["scores"], d["fin"], d["lens"], d["ys"], d["valid"], off, d["kv_src"], d["done"],
                    d["pos"], PAD, EOS, parent_i32=d["parent"])
    torch.cuda.synchronize()
    parent, tok, sc, f2, l2 = beam_step_reference(scores, fin, lens, beam_log_softmax(logits), k, PAD, EOS)
    assert torch.equal(d["parent"].cpu().view(n, k).long(), parent)
    assert torch.equal(d["ys"][:, p].cpu().view(n, k), tok)
    assert torch.equal(d["fin"].cpu().view(n, k).bool(), f2)
    assert torch.equal(d["lens"].cpu().view(n, k).long(), l2)
    torch.testing.assert_close(d["scores"].cpu().view(n, k), sc, rtol=1e-6, atol=0)
    assert torch.equal(d["done"].cpu().bool(), f2.all(1))
    # everything else of ys / valid untouched; the new slot's flag
    ys_want, valid_want = ys.clone(), valid.clone()
    ys_want[:, p] = tok.reshape(-1)
    valid_want[:, off + p] = (tok.reshape(-1) != PAD).to(torch.uint8)
    assert torch.equal(d["ys"].cpu(), ys_want) and torch.equal(d["valid"].cpu(), valid_want)
    # the map: each child takes its parent's row (before the call), plus its own new slot
    src_rows = (torch.arange(n).view(n, 1) * k + parent).reshape(-1)
    want = kv_src[src_rows].clone()
    want[:, off + p] = torch.arange(rows, dtype=torch.int32)
    assert torch.equal(d["kv_src"].cpu(), want)
    if k >= 2:
        assert parent[2, :2].tolist() == [0, 0] and tok[2, :2].tolist() == [5, 6]
        assert parent[4, :2].tolist() == [0, 1] and tok[4, :2].tolist() == [5, PAD]


def test_beam_select_rejects_out_of_range_arguments():
    """Bad sizes return GCT_ERR_ARG before any launch."""
    L = ops._L()
    x = torch.zeros(8, 30, device="cuda")
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    b_ = buf.data_ptr()
    #    logits   V   n  k  scores fin lens parent ys ld_ys valid sb off kv_src ld_src T  done pos  pad  eos  stream
    ok = [x.data_ptr(), 30, 2, 4, b_, b_, b_, b_, b_, 40, b_, 40, 0, b_, 40, 40, b_, b_, PAD, EOS, None]
    for i, bad in [(3, 0), (3, 17), (1, 3), (1, 65537), (15, 257), (14, 39), (11, 39), (9, 30), (18, 30), (18, -1),
                   (17, None)]:
        args = list(ok)
        args[i] = bad
        assert L.gct_beam_select(*args) == GCT_ERR_ARG, (i, bad)


# ----------------------------------------------------------------------------------------- gct_attn_decode_beam
@pytest.mark.parametrize("H,dk,Lold", [(8, 64, 37), (4, 16, 1), (2, 32, 130), (8, 64, 200)])
def test_attn_decode_beam_identity_and_random_map(H, dk, Lold):
    g = torch.Generator().manual_seed(H * dk + Lold)
    n, T, off = 12, 208, 3
    d = H * dk
    kc = torch.randn(n, T, d, generator=g).cuda()
    vc = torch.randn(n, T, d, generator=g).cuda()
    valid = (torch.rand(n, T, generator=g) < 0.8).to(torch.uint8).cuda()
    qkv = torch.randn(n, 3 * d, generator=g).cuda()
    pos = torch.tensor([Lold - off], dtype=torch.int32, device="cuda")
    out1, out2, out3 = (torch.empty(n, d, device="cuda") for _ in range(3))
    kc2, vc2 = kc.clone(), vc.clone()
    ops.attn_decode(qkv, 3 * d, kc, vc, d, T * d, valid, T, out1, n, H, 0, dk, pos=pos, cache_off=off,
                    knew=qkv[:, d:], vnew=qkv[:, 2 * d:], ldn=3 * d)
    ident = torch.arange(n, dtype=torch.int32, device="cuda").view(n, 1).expand(n, T).contiguous()
    ops.attn_decode_beam(qkv, 3 * d, kc2, vc2, d, T * d, valid, T, out2, n, H, T, dk, pos, off, qkv[:, d:],
                         qkv[:, 2 * d:], 3 * d, ident)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)                              # same bytes
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)        # the step's key / value appended to row b
    # random ancestry: key j of row b from row src[b, j]
    src = torch.randint(0, n, (n, T), generator=g).to(torch.int32)
    src[:, Lold] = torch.arange(n, dtype=torch.int32)
    ops.attn_decode_beam(qkv, 3 * d, kc2, vc2, d, T * d, valid, T, out3, n, H, T, dk, pos, off, qkv[:, d:],
                         qkv[:, 2 * d:], 3 * d, src.cuda())
    torch.cuda.synchronize()
    K, Vv, M = kc.double().cpu(), vc.double().cpu(), valid.cpu()
    jj = torch.arange(Lold + 1)
    rows = src[:, :Lold + 1].long()
    keys = K[rows, jj]                                           # [n, Lold+1, d]
    vals = Vv[rows, jj]
    msk = M[rows, jj]
    keys[:, Lold], vals[:, Lold] = qkv[:, d:2 * d].double().cpu(), qkv[:, 2 * d:].double().cpu()
    q = qkv[:, :d].double().cpu().view(n, H, dk)
    s = torch.einsum("nhd,njhd->nhj", q, keys.view(n, Lold + 1, H, dk)) / math.sqrt(dk)
    s = s.masked_fill(msk.view(n, 1, Lold + 1) == 0, -1e9)
    want = torch.einsum("nhj,njhd->nhd", torch.softmax(s, -1), vals.view(n, Lold + 1, H, dk)).reshape(n, d)
    torch.testing.assert_close(out3.double().cpu(), want, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------------------- generate_beam
def near_tie(trace, b, upto=None):
    """Some step of sample b (up to `upto`) had two of its k+1 best candidates within GAP."""
    for t, top in enumerate(trace):
        if upto is not None and t > upto:
            break
        v = top[b]
        v = v[torch.isfinite(v)]
        if v.numel() > 1 and float((v[:-1] - v[1:]).min()) < GAP:
            return True
    return False


def compare_beams(got, ref, trace, alpha=BEAM_ALPHA):
    ys, sc, ln = got
    rys, rsc, rln = ref
    L = max(ys.shape[2], rys.shape[2])
    pad = lambda t: torch.nn.functional.pad(t, (0, L - t.shape[2]), value=PAD)    # noqa: E731
    ys, rys = pad(ys.cpu()), pad(rys.cpu())
    sc, rsc, ln, rln = sc.cpu(), rsc.cpu(), ln.cpu(), rln.cpu()
    differ = 0
    for b in range(ys.shape[0]):
        if torch.equal(ys[b], rys[b]):
            torch.testing.assert_close(sc[b], rsc[b], rtol=0, atol=1e-4)
            assert torch.equal(ln[b], rln[b])
            continue
        differ += 1
        norm = rsc[b] / rln[b].clamp(min=1).float() ** alpha
        final_tie = norm.numel() > 1 and float((norm[:-1] - norm[1:]).abs().min()) < GAP
        assert near_tie(trace, b) or final_tie, (b, ys[b].tolist(), rys[b].tolist(), rsc[b].tolist())
    return differ


def beam_case(mtype, full, c2d, n, k, graphs, seed, steps=30):
    model = build(mtype, full=full, seed=seed, c2d=c2d)
    nc = synthetic.n_conds(mtype)
    lat = 128 if full else TINY["latent_dim"]
    Le = 24 + (0 if c2d else nc)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, Le, lat, generator=g).cuda()
    dconds = torch.randn(n, nc, generator=g).cuda() if nc else None
    lens = torch.randint(6, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < lens[:, None]).unsqueeze(1).cuda()
    if mtype in ("scavaetf", "pscavaetf"):
        pre = torch.randint(5, 30, (n, 5), generator=g)
        ys0 = torch.cat([torch.full((n, 1), synthetic.SOS_ID), pre, torch.full((n, 1), synthetic.SEP_ID)], 1).cuda()
    else:
        ys0 = torch.full((n, 1), synthetic.SOS_ID, dtype=torch.long, device="cuda")
    trace = []
    ref = reference_style_beam_decode(model, z, src_mask, dconds, ys0, PAD, EOS, k, steps, trace=trace)
    kd = KVDecoder(model, PAD, synthetic.SOS_ID, EOS)
    kd.start(z, src_mask, dconds, max_total_len=ys0.shape[1] + steps + 2, beams=k)
    got = kd.generate_beam(ys0, k, steps, use_graphs=graphs)
    if graphs:
        assert "beam" in kd.graphs
    return got, ref, trace, kd


@pytest.mark.parametrize("mtype,full,c2d,k,graphs", [
    ("vaetf", False, False, 4, False), ("vaetf", False, False, 4, True), ("vaetf", False, False, 1, True),
    ("pscavaetf", False, False, 4, False), ("pscavaetf", False, False, 4, True),
    ("pvaetf", False, True, 4, False), ("pvaetf", False, True, 4, True), ("pvaetf", False, True, 1, False),
    ("vaetf", True, False, 4, True), ("pscavaetf", True, False, 4, False), ("pscavaetf", True, False, 1, True)])
def test_generate_beam_matches_uncached_loop(mtype, full, c2d, k, graphs):
    n = 4 if full else 6
    got, ref, trace, _ = beam_case(mtype, full, c2d, n, k, graphs, seed=7 + k)
    assert got[0].shape[:2] == (n, k)
    differ = compare_beams(got, ref, trace)
    assert differ <= max(1, n // 4), differ


@pytest.mark.parametrize("graphs", [False, True])
def test_beam_size_one_is_greedy(graphs):
    """k = 1: the same tokens as generate(..., "greedy") up to and including the first <eos>, unless an fp32 tie."""
    from gct_plus_amd.Model.modules import get_trg_mask
    mtype = "pscavaetf"
    model = build(mtype, seed=5)
    n, Le, nc = 10, 27, 3
    g = torch.Generator().manual_seed(5)
    z = torch.randn(n, Le, 16, generator=g).cuda()
    dconds = torch.randn(n, nc, generator=g).cuda()
    src_mask = (torch.arange(Le)[None, :] < torch.randint(8, Le + 1, (n,), generator=g)[:, None]).unsqueeze(1).cuda()
    ys0 = torch.full((n, 1), synthetic.SOS_ID, dtype=torch.long, device="cuda")
    kd = KVDecoder(model, PAD, synthetic.SOS_ID, EOS)
    kd.start(z, src_mask, dconds, max_total_len=48)
    greedy = kd.generate(ys0, 40, use_graphs=graphs).cpu()
    kd.start(z, src_mask, dconds, max_total_len=48, beams=1)
    ys, sc, ln = kd.generate_beam(ys0, 1, 40, use_graphs=graphs)
    ys = ys[:, 0].cpu()
    for b in range(n):
        L = int(ln[b, 0]) + 1                            # prefix <sos> + the generated tokens through <eos>
        a, r = ys[b, :L], greedy[b, :L]
        m = min(a.numel(), r.numel())
        if torch.equal(a[:m], r[:m]):
            assert a.numel() == r.numel()
            continue
        t = int((a[:m] != r[:m]).nonzero()[0])
        pre = r[None, :t].cuda()
        logits = model.decode(pre, z[b:b + 1], src_mask[b:b + 1], get_trg_mask(pre, PAD, False, dconds[b:b + 1]),
                              dconds[b:b + 1])[0, -1]
        top2 = beam_log_softmax(logits).topk(2).values
        assert float(top2[0] - top2[1]) < GAP, (b, t, a.tolist(), r.tolist())


def test_generate_beam_matches_cpu_oracle():
    """A tiny-model beam search written here over the oracle's un-cached CPU decoder."""
    from oracle import gct_oracle as O
    from gct_plus_amd.Model.modules import get_trg_mask
    mtype, k, steps = "pvaetf", 4, 24
    model = build(mtype, seed=11)
    vs, vt = synthetic.vocab_sizes(mtype)
    n, nc, Le = 5, 3, 20
    g = torch.Generator().manual_seed(11)
    z = torch.randn(n, Le + nc, 16, generator=g)
    dconds = torch.randn(n, nc, generator=g)
    src_mask = (torch.arange(Le + nc)[None, :] < torch.randint(10, Le + nc + 1, (n,), generator=g)[:, None]).unsqueeze(1)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, use_cond2lat=True, **TINY)
    P = {key: v.detach().cpu() for key, v in model.state_dict().items()}
    rep = lambda x: x.repeat_interleave(k, 0)          # noqa: E731
    zr, mr, dr = rep(z), rep(src_mask), rep(dconds)
    ys = torch.full((n * k, 1), synthetic.SOS_ID, dtype=torch.long)
    scores, fin, lens = beam_init(n, k)
    trace = []
    for _ in range(steps - 1):
        logits = O.decode(P, cfg, ys, zr, mr, get_trg_mask(ys, PAD, False, dr), dr)
        logp = beam_log_softmax(logits[:, -1])
        cand = beam_candidates(scores, fin, logp, k, PAD)
        trace.append(cand.topk(k + 1, dim=1).values)
        parent, tok, scores, fin, lens = beam_step_reference(scores, fin, lens, logp, k, PAD, EOS)
        ys = torch.cat([ys[(torch.arange(n).view(n, 1) * k + parent).view(-1)], tok.view(-1, 1)], 1)
        if fin.all():
            break
    ref = beam_finalize(ys.view(n, k, -1), scores, lens, 1)
    kd = KVDecoder(model, PAD, synthetic.SOS_ID, EOS)
    kd.start(z.cuda(), src_mask.cuda(), dconds.cuda(), max_total_len=steps + 2, beams=k)
    got = kd.generate_beam(torch.full((n, 1), synthetic.SOS_ID, dtype=torch.long, device="cuda"), k, steps)
    assert compare_beams(got, ref, trace) <= 1


def test_sampling_front_end_beam_all_model_types():
    import numpy as np
    from gct_plus_amd import data
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    for mtype in ("vaetf", "pvaetf", "scavaetf", "pscavaetf"):
        sep = mtype in ("scavaetf", "pscavaetf")
        strs = [("c1ccccc1<sep>" + s) if sep else s for s in SMILES]
        SRC, TRG = data.Vocab.build(strs, False, sep), data.Vocab.build(strs, True, sep)
        nc = synthetic.n_conds(mtype)
        torch.manual_seed(4)
        model = model_dict[mtype](len(SRC), len(TRG), dropout=0.1, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
        sp = get_sampler(mtype, model, SRC, TRG, latent_dim=16, max_strlen=24, cond_dim=nc, decode_algo="beam",
                         beam_size=4, toklen_data=[12, 14, 15, 18, 20, 16])
        n = 6
        extra = (1 + len(sp.smi_to_id("c1ccccc1")) + 1) if sep else 0
        z = torch.randn(n, 16 + nc + extra, 16, generator=torch.Generator().manual_seed(9))
        args = {"vaetf": (n,), "pvaetf": (np.zeros((n, 3)),), "scavaetf": (n, "c1ccccc1"),
                "pscavaetf": (np.ones((n, 3)) * 0.3, "c1ccccc1")}[mtype]
        kw = {} if nc == 0 else {"transform": False}
        s1, toklen, _ = sp.sample_smiles(*args, zs=z, **kw)
        s2, _, _ = sp.sample_smiles(*args, zs=z, **kw)
        assert len(s1) == n and all(isinstance(s, str) for s in s1) and len(toklen) == n
        assert s1 == s2, mtype
    # decode returns the best of decode_beams
    ys0 = sp.init_y(n, True, sp.smi_to_id("c1ccccc1"), True)
    src_mask = torch.ones(n, 1, z.shape[1], dtype=torch.bool)
    dc = torch.full((n, 3), 0.3)
    best = sp.decode(z, ys0, src_mask, dc)
    allb, sc, ln = sp.decode_beams(z, ys0, src_mask, dc)
    assert allb.shape[:2] == (n, 4) and torch.equal(best, allb[:, 0])
    norm = sc / ln.float() ** BEAM_ALPHA
    assert bool((norm[:, :-1] >= norm[:, 1:]).all())
