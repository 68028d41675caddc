"""Grammar-constrained decoding on the device: gct_grammar_mask against SmilesGrammar.mask_reference bit for bit (uniform
rows, mixed prefixes, the stream layout with a parked row and a row inside its prefix, V = 31 and V = 70, histories longer
than a wave), and generate / generate_stream / the sampler with a grammar: every row ends with <eos> inside its limit and
passes the independent parser of tests/test_grammar_host.py; greedy picks are replayed against teacher-forced logits."""
import random

import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd.decode import (GRAMMAR, KVDecoder, generated_tokens, reference_style_decode, sample_filter_reference,
                                 score_tokens)
from gct_plus_amd.smiles import SmilesGrammar, grammar_min_finish
from tests.test_grammar_host import EOS, PAD, SOS, VOCAB31, VOCAB70, parses
from tests.test_mixed_scaffold_decode_gpu import TINY, mixed_prefixes
from tests.test_sample_filter_gpu import select
from tests.test_score_gpu import close_sums, close_tokens
from tests.test_stream_decode_gpu import make_pool, make_sampler

pytestmark = pytest.mark.gpu

SENT = 7.25
GR31, GR70 = SmilesGrammar(VOCAB31, PAD, EOS), SmilesGrammar(VOCAB70, PAD, EOS)
_MODELS = {}


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def cu(t):
    return None if t is None else t.cuda()


def model_of(mtype):
    """The tiny config of the G2 fixtures (N = 2, d_model = 64) with the 31-token target vocabulary, built once."""
    if mtype not in _MODELS:
        from gct_plus_amd.Model import model_dict
        torch.manual_seed(21)
        _MODELS[mtype] = model_dict[mtype](29, 31, dropout=0.1, nconds=synthetic.n_conds(mtype), use_cond2lat=True,
                                           **TINY).cuda().eval()
    return _MODELS[mtype]


def walk(gr, G, rng, length):
    """`length` tokens of a random walk through gr.allowed under the budget G; <eos> is taken only when nothing else is
    allowed or with probability 0.1, so that histories grow long; behind the end of the walk the row writes pad."""
    toks = []
    while len(toks) < length:
        ok = gr.allowed(toks, G - len(toks))
        if len(ok) > 1 and rng.random() < 0.9:
            ok = [t for t in ok if t != EOS]
        toks.append(rng.choice(ok))
    return toks


def same_bits(got, ref):
    return torch.equal(got.cpu().view(torch.int32), ref.cpu().view(torch.int32))


# ------------------------------------------------------------------------------------ 1. the mask against the reference
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("gr", [GR31, GR70], ids=["V31", "V70"])
def test_mask_equals_the_reference_plain_rows(ops, gr, layout):
    """n = 37 rows (not a multiple of the 4 rows of a workgroup) that have all generated g tokens, for g = 0, 1, 6, the
    last slot, and one past the budget; the columns behind a row's position hold tokens the kernel must not read."""
    rng = random.Random(len(gr) + len(layout))
    n, V, T, G = 37, len(gr), 40, 14
    g_t = torch.Generator().manual_seed(V)
    lens = [rng.randint(1, 7) for _ in range(n)] if layout == "mixed" else [3] * n
    t0 = max(lens)
    for g in (0, 1, 6, 13, 14, 15):
        ys = torch.randint(0, V, (n, T), generator=g_t)                            # (also behind the rows' positions)
        for r in range(n):
            ys[r, lens[r]:lens[r] + g] = torch.tensor(walk(gr, G, rng, g), dtype=torch.long)
        x = torch.randn(n, V, generator=g_t) * 3
        x[0, 0], x[1, V - 1] = -0.0, 3.0e38
        ref = gr.mask_reference(x, ys, lens, [t + g for t in lens], G)
        out = torch.full((n, V), SENT).cuda()
        row_off = torch.tensor([t0 - t for t in lens], dtype=torch.int32).cuda() if layout == "mixed" else None
        ops.grammar_mask(x.cuda(), out, gr.table.cuda(), ys.cuda(), torch.tensor([t0 + g - 1], dtype=torch.int32).cuda(),
                         row_off=row_off, gram=torch.tensor([G, t0], dtype=torch.int32).cuda())
        assert same_bits(out, ref), (layout, g)
        kept = torch.isfinite(ref).sum(1)
        assert int(kept.min()) >= 1                                                 # the allowed set is never empty
        if g >= G - 1:
            assert int(kept.max()) == 1                                             # <eos> (last slot) or <pad> only


def test_mask_with_histories_longer_than_a_wave(ops):
    """150 generated tokens per row (three per lane) under a budget of 199, branches and rings open along the way."""
    rng = random.Random(3)
    gr, n, T, G, t0, g = GR70, 6, 256, 199, 4, 150
    ys = torch.full((n, T), PAD)
    for r in range(n):
        ys[r, t0:t0 + g] = torch.tensor(walk(gr, G, rng, g), dtype=torch.long)
    states = [gr.state(ys[r, t0:t0 + g].tolist()) for r in range(n)]
    assert max(s[1] for s in states) >= 2 and any(s[2] for s in states)          # open branches, open rings
    x = torch.randn(n, len(gr), generator=torch.Generator().manual_seed(1))
    out = torch.full_like(x, SENT).cuda()
    ops.grammar_mask(x.cuda(), out, gr.table.cuda(), ys.cuda(), torch.tensor([t0 + g - 1], dtype=torch.int32).cuda(),
                     gram=torch.tensor([G, t0], dtype=torch.int32).cuda())
    assert same_bits(out, gr.mask_reference(x, ys, t0, t0 + g, G))
    # the budget binds: 150 + what the state needs to finish
    tight = [g + max(1, grammar_min_finish(s)) for s in states]
    for r in range(n):
        out.fill_(SENT)
        ops.grammar_mask(x.cuda(), out, gr.table.cuda(), ys.cuda(), torch.tensor([t0 + g - 1], dtype=torch.int32).cuda(),
                         gram=torch.tensor([tight[r], t0], dtype=torch.int32).cuda())
        ref = gr.mask_reference(x[r:r + 1], ys[r:r + 1], t0, t0 + g, tight[r])
        assert same_bits(out[r:r + 1], ref) and int(torch.isfinite(ref).sum()) >= 1


@pytest.mark.parametrize("gr", [GR31, GR70], ids=["V31", "V70"])
def test_mask_equals_the_reference_stream_layout(ops, gr):
    """Rows at their own positions behind one counter, each with its item's prefix length and limit; row 5 is parked and
    row 9 is still inside its prefix: both are left untouched."""
    rng = random.Random(11 + len(gr))
    n, N, V, T, pos = 37, 45, len(gr), 64, 40
    g_t = torch.Generator().manual_seed(2)
    item = torch.randperm(N, generator=g_t)[:n].int()
    item[5] = -1
    prefix_len = torch.randint(1, 7, (N,), generator=g_t).int()
    limit = torch.randint(2, 15, (N,), generator=g_t).int()
    ys = torch.randint(0, V, (n, T), generator=g_t)
    row_off, starts, cols, budgets = torch.zeros(n, dtype=torch.int32), [], [], []
    for r in range(n):
        it = int(item[r])
        t0, G = (int(prefix_len[it]), int(limit[it])) if it >= 0 else (1, 2)
        g = rng.randint(0, G + 1) if r != 9 else -2                                  # (G + 1: one past the budget)
        if g > 0:
            ys[r, t0:t0 + g] = torch.tensor(walk(gr, G, rng, g), dtype=torch.long)
        row_off[r] = pos + 1 - (t0 + g)
        starts.append(t0), cols.append(t0 + g), budgets.append(G)
    x = torch.randn(n, V, generator=g_t) * 3
    ref = gr.mask_reference(x, ys, starts, cols, budgets)
    ref[5] = SENT
    ref[9] = SENT
    out = torch.full((n, V), SENT).cuda()
    ops.grammar_mask(x.cuda(), out, gr.table.cuda(), ys.cuda(), torch.tensor([pos], dtype=torch.int32).cuda(),
                     row_off=row_off.cuda(), item=item.cuda(), prefix_len=prefix_len.cuda(), limit=limit.cuda())
    assert same_bits(out, ref)
    live = [r for r in range(n) if r not in (5, 9)]
    assert int(torch.isfinite(ref[live]).sum(1).min()) >= 1 and bool(torch.isneginf(ref[live]).any(1).all())


# --------------------------------------------------------------------------- 1b. the selection on masked logits
def masked_rows(gr, n, seed):
    """n rows of logits masked by the reference after random-walk histories of 0 .. 8 tokens: (masked, forbidden)."""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, len(gr), generator=g) * 2
    hists = [walk(gr, 12, rng, rng.randint(0, 8)) for _ in range(64)]
    ys = torch.full((n, 10), PAD)
    cols = []
    for r in range(n):
        h = hists[r % 64]
        ys[r, 1:1 + len(h)] = torch.tensor(h, dtype=torch.long)
        cols.append(1 + len(h))
    masked = gr.mask_reference(x, ys, 1, cols, 12)
    return masked, torch.isneginf(masked)


@pytest.mark.parametrize("gr", [GR31, GR70], ids=["V31", "V70"])
def test_filtered_probabilities_on_masked_logits(gr):
    """probs_out of the filtered selection on grammar-masked logits against sample_filter_reference: a forbidden token
    weighs exactly 0 -- with top_k below V it does not get the 1e-6 floor -- and is never drawn."""
    masked, off = masked_rows(gr, 256, 7)
    V = len(gr)
    for filt in ((3, None, 1.0), (V - 1, None, 1.0), (3, 0.9, 1.5), (None, 0.8, 0.7)):
        want = sample_filter_reference(masked, *filt)
        tok, pr = select(masked.cuda(), filt, seed=11)
        assert bool((pr[off] == 0).all()), filt
        assert torch.allclose(pr.double(), want.double(), atol=1e-6, rtol=0), filt
        assert not bool(off[torch.arange(256), tok].any()), filt


@pytest.mark.parametrize("gr", [GR31, GR70], ids=["V31", "V70"])
def test_no_forbidden_token_in_65536_draws(ops, gr):
    """Plain multinomial, the filtered kernel with neutral settings (a row it leaves unchanged) and with top-k: 65 536
    draws each on masked logits, none of them a forbidden token, and the plain and the neutral draws coincide."""
    masked, off = masked_rows(gr, 65536, 8)
    rows = torch.arange(masked.shape[0])
    dev = masked.cuda()
    plain, _ = select(dev, None, seed=5, probs=False)
    # (neutral settings straight to the kernel: select()'s front end would be free to drop them)
    ys = torch.zeros(len(rows), 2, dtype=torch.int64, device="cuda")
    ops.select_token(dev, ys, 1, torch.zeros(len(rows), 2, dtype=torch.uint8, device="cuda"),
                     torch.zeros(len(rows), dtype=torch.uint8, device="cuda"), 1, PAD, EOS, seed=5,
                     filt_dev=ops.sample_filter_settings(None, None, 1.0, len(gr)).cuda())
    neutral = ys[:, 1].cpu()
    topk, _ = select(dev, (4, None, 1.0), seed=5, probs=False)
    for name, tok in (("plain", plain), ("neutral", neutral), ("top-k", topk)):
        assert not bool(off[rows, tok].any()), name
    assert torch.equal(plain, neutral)


# ------------------------------------------------------------------------------------------------ 2. generate
def rows_of(mtype, seed):
    """12 rows: pscavaetf with mixed scaffold prefixes of 3 / 6 / 2 / 5 tokens, vaetf with <sos> alone."""
    g = torch.Generator().manual_seed(seed)
    nc = synthetic.n_conds(mtype)
    if mtype == "pscavaetf":
        ys0, lens = mixed_prefixes([3, 6, 2, 5], 3, g)
    else:
        ys0, lens = torch.full((12, 1), SOS), None
    n, Le = ys0.shape[0], 20 + nc
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    return dict(z=z, src_mask=src_mask, dconds=torch.randn(n, nc, generator=g) if nc else None, ys0=ys0, lens=lens)


def constrained(model, p, max_strlen, kd=None, gr=GR31, **kw):
    kd = kd or KVDecoder(model, PAD, SOS, EOS)
    kd.start(cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), max_total_len=p["ys0"].shape[1] + 30)
    return kd.generate(p["ys0"].cuda(), max_strlen, prefix_lens=p["lens"], grammar=gr, **kw)


def check_rows(ys, lens, G, gr=GR31):
    """Every row: <eos> within its G tokens, pad behind it up to the end of the row, and the parser accepts it.
    Returns the generated lengths."""
    ys = ys.cpu()
    n, W = ys.shape
    out = []
    for r in range(n):
        t0 = int(lens[r])
        gen = ys[r, t0:].tolist()
        assert EOS in gen[:G], (r, gen)
        k = gen.index(EOS) + 1
        assert all(t == PAD for t in gen[k:]), (r, gen)
        assert parses([gr.itos[t] for t in gen]), (r, [gr.itos[t] for t in gen])
        assert gr.well_formed(gen)
        out.append(k)
    return out


HOW = {"greedy": dict(algo="greedy"), "multinomial": dict(algo="multinomial", seed=5),
       "filtered": dict(algo="multinomial", seed=5, top_k=3, top_p=0.9, temperature=1.5)}


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_generate_rows_are_well_formed(mtype, how):
    """max_strlen = 12: the budget of 11 tokens binds.  Graphs on and off give the same ids; greedy picks are replayed on
    the teacher-forced logits of the returned rows: every chosen token is allowed by the reference and its logit is within
    the project's logit tolerance (atol 1e-4) of the best allowed one -- every row, every generated column."""
    from gct_plus_amd.Model.modules import get_trg_mask
    model, p, G = model_of(mtype), rows_of(mtype, 31), 11
    n, t0 = p["ys0"].shape
    lens = p["lens"] if p["lens"] is not None else torch.full((n,), t0)
    ys = constrained(model, p, G + 1, **HOW[how])
    kd = KVDecoder(model, PAD, SOS, EOS)
    ys_g = constrained(model, p, G + 1, kd=kd, use_graphs=True, **HOW[how])
    assert torch.equal(ys, ys_g)
    assert any(isinstance(k, tuple) and GRAMMAR in k for k in kd.graphs)
    ys = ys.cpu()
    assert torch.equal(ys[:, :t0][p["ys0"] != PAD], p["ys0"][p["ys0"] != PAD])      # prefixes intact
    took = check_rows(ys, lens, G)
    print(f"{mtype} {how}: generated lengths {sorted(took)}")
    if how == "multinomial":
        assert len({tuple(generated_tokens(ys, lens)[r].tolist()) for r in range(n)}) > n // 2   # rows do differ
    if how != "greedy":
        return
    trg = ys[:, :-1].cuda()
    d = cu(p["dconds"])
    with torch.no_grad():
        logits = model.decode(trg, cu(p["z"]), cu(p["src_mask"]), get_trg_mask(trg, PAD, False, d), d).float().cpu()
    worst = 0.0
    for r in range(n):
        for c in range(int(lens[r]), ys.shape[1]):
            hist = ys[r, int(lens[r]):c].tolist()
            ok = GR31.allowed(hist, G - len(hist))
            assert int(ys[r, c]) in ok, (r, c, hist)
            gap = float(logits[r, c - 1, ok].max() - logits[r, c - 1, int(ys[r, c])])
            worst = max(worst, gap)
            assert gap <= 1e-4, (r, c, gap)
    print(f"{mtype} greedy replay: worst logit gap to the best allowed token {worst:.3e}")
    # the constraint did something: the unconstrained greedy rows are not all well formed
    kd.start(cu(p["z"]), cu(p["src_mask"]), d, max_total_len=t0 + 30)
    free = generated_tokens(kd.generate(p["ys0"].cuda(), G + 1, prefix_lens=p["lens"]).cpu(), lens)
    assert not all(GR31.well_formed(free[r].tolist()) for r in range(n))


@pytest.mark.parametrize("mtype", ["pscavaetf", "vaetf"])
def test_greedy_equals_the_uncached_constrained_loop(mtype):
    """Constrained greedy generate against reference_style_decode(grammar=) -- the un-cached model.decode loop with
    mask_reference in front of its argmax -- token for token; a difference only at a near-tie of that loop (its two best
    ALLOWED logits closer than 1e-4 at the first differing column)."""
    from gct_plus_amd.Model.modules import get_trg_mask
    model, p, G = model_of(mtype), rows_of(mtype, 34), 11
    n = p["ys0"].shape[0]
    ys0 = torch.full((n, 1), SOS)
    q = dict(p, ys0=ys0, lens=None)
    got = constrained(model, q, G + 1).cpu()
    z, m, d = cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"])
    ref = reference_style_decode(model, z, m, d, ys0.cuda(), PAD, EOS, G + 1, grammar=GR31).cpu()
    check_rows(ref, torch.ones(n, dtype=torch.long), G)
    w = min(got.shape[1], ref.shape[1])
    assert bool((got[:, w:] == PAD).all()) and bool((ref[:, w:] == PAD).all())
    for r in range(n):
        if torch.equal(got[r, :w], ref[r, :w]):
            continue
        c = int((got[r, :w] != ref[r, :w]).nonzero()[0])
        ys = ref[r:r + 1, :c].cuda()
        dd = None if d is None else d[r:r + 1]
        with torch.no_grad():
            x = model.decode(ys, z[r:r + 1], m[r:r + 1], get_trg_mask(ys, PAD, False, dd), dd)[:, -1].float().cpu()
        top2 = GR31.mask_reference(x, ref[r:r + 1], 1, c, G)[0].topk(2).values
        assert float(top2[0] - top2[1]) < 1e-4, (r, c, top2.tolist())


def test_the_budget_lives_in_device_memory():
    """One decoder, graphs on: max_strlen 12, then 6 and another prefix width through the graphs captured by the first
    call -- every row still ends inside the new limit.  Then without a grammar: what a fresh decoder gives."""
    model, p = model_of("pscavaetf"), rows_of("pscavaetf", 32)
    kd = KVDecoder(model, PAD, SOS, EOS)
    kw = dict(kd=kd, use_graphs=True, algo="multinomial", seed=3)
    check_rows(constrained(model, p, 12, **kw), p["lens"], 11)
    keys = set(kd.graphs)
    assert any(isinstance(k, tuple) and GRAMMAR in k for k in keys)
    took = check_rows(constrained(model, p, 6, **kw), p["lens"], 5)
    assert max(took) <= 5 and set(kd.graphs) == keys
    q = dict(p, ys0=torch.cat([p["ys0"], torch.full((12, 2), PAD)], 1))              # prefix width 8 instead of 6
    eager = constrained(model, q, 6, algo="multinomial", seed=3)
    assert torch.equal(constrained(model, q, 6, **kw), eager) and set(kd.graphs) == keys
    check_rows(eager, p["lens"], 5)
    free = [constrained(model, p, 12, gr=None, kd=k, use_graphs=True, algo="multinomial", seed=3)
            for k in (kd, KVDecoder(model, PAD, SOS, EOS))]
    assert torch.equal(free[0], free[1])


# ------------------------------------------------------------------------------------------------ 3. the stream
def test_stream_items_end_inside_their_own_limits():
    """50 items through 8 rows, limits of 2 .. 11 tokens, mixed prefix lengths, multinomial: every item ends with <eos>
    inside its own limit and parses; and its tokens are what constrained generate() draws for it with the same seed and
    the same limit (keys (item, position) = (row, position); the two differ by prefill-versus-step rounding only: the
    0.99 bound of test_one_wave_multinomial_matches_generate)."""
    model = model_of("pscavaetf")
    N, R = 50, 8
    p = make_pool("pscavaetf", torch.randint(1, 9, (N,), generator=torch.Generator().manual_seed(4)).tolist(), 1, 19)
    caps = torch.randint(2, 12, (N,), generator=torch.Generator().manual_seed(6))
    lens = p["lens"]
    outs = []
    for graphs in (False, True):
        kd = KVDecoder(model, PAD, SOS, EOS)
        kd.start_stream(cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), rows=R, max_total_len=40)
        ys, rec = kd.generate_stream(p["ys0"].cuda(), 12, algo="multinomial", seed=7, prefix_lens=lens,
                                     max_new_tokens=caps, grammar=GR31, use_graphs=graphs)
        assert rec["harvested"] == N and int(rec["start_step"].max()) > 0         # refills did happen
        outs.append((ys.cpu(), rec["out_len"]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ys, out_len = outs[0]
    gen = generated_tokens(ys, lens)
    for i in range(N):
        k = int(out_len[i])
        row = gen[i].tolist()
        assert 2 <= k <= int(caps[i]) and row[k - 1] == EOS and EOS not in row[:k - 1], (i, row, int(caps[i]))
        assert all(t == PAD for t in row[k:]) and parses([VOCAB31[t] for t in row]), (i, row)
    assert any(int(out_len[i]) == int(caps[i]) for i in range(N))                   # limits did bind
    same = 0
    kd = KVDecoder(model, PAD, SOS, EOS)
    for cap in sorted(set(caps.tolist())):
        kd.start(cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), max_total_len=40)
        alone = generated_tokens(kd.generate(p["ys0"].cuda(), cap + 1, algo="multinomial", seed=7, prefix_lens=lens,
                                             grammar=GR31).cpu(), lens)
        for i in (caps == cap).nonzero().view(-1).tolist():
            k = int(out_len[i])
            same += alone[i, :k].tolist() == gen[i, :k].tolist() and bool((alone[i, k:] == PAD).all())
    assert same >= 0.99 * N, (same, N)


# ------------------------------------------------------------------------------------------- 4. log-probabilities
@pytest.mark.parametrize("graphs", [False, True])
def test_log_probs_stay_the_models_own(graphs):
    """return_logp with a grammar: the log-probabilities are those of the RAW logits -- score_tokens of the returned
    rows, within the tolerance tests/test_score_gpu.py uses for the same comparison -- for generate and for the stream."""
    model, p = model_of("pscavaetf"), rows_of("pscavaetf", 33)
    lens = p["lens"]
    ys, tl, lp = constrained(model, p, 12, algo="multinomial", seed=9, use_graphs=graphs, return_logp=True)
    took = check_rows(ys, lens, 11)
    cols = torch.arange(ys.shape[1])[None, :]
    span = (cols >= lens[:, None]) & (cols < (lens + torch.tensor(took))[:, None])
    tl = tl.cpu()
    assert bool((tl[~span] == 0).all()) and bool((tl[span] < 0).all())
    z, m, d = cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"])
    _, nt, _, ref_tl = score_tokens(model, z, m, d, ys, prefix_lens=lens, pad_id=PAD)
    assert torch.equal(nt.cpu().long(), span.sum(1))
    close_tokens(tl, ref_tl, f"constrained generate graphs={graphs} token_logp vs score_tokens")
    close_sums(lp, ref_tl, f"constrained generate graphs={graphs} logp vs score_tokens")
    caps = torch.randint(2, 12, (12,), generator=torch.Generator().manual_seed(8))
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start_stream(z, m, d, rows=4, max_total_len=40)
    ys, rec, tl, lp = kd.generate_stream(p["ys0"].cuda(), 12, algo="multinomial", seed=9, prefix_lens=lens,
                                         max_new_tokens=caps, grammar=GR31, use_graphs=graphs, return_logp=True)
    cols = torch.arange(ys.shape[1])[None, :]
    span = (cols >= lens[:, None]) & (cols < (lens + rec["out_len"])[:, None])
    tl = tl.cpu()
    assert bool((tl[~span] == 0).all()) and bool((tl[span] < 0).all())
    _, nt, _, ref_tl = score_tokens(model, z, m, d, ys, prefix_lens=lens, pad_id=PAD)
    assert torch.equal(nt.cpu().long(), span.sum(1))
    close_tokens(tl, ref_tl, f"constrained stream graphs={graphs} token_logp vs score_tokens")
    close_sums(lp, ref_tl, f"constrained stream graphs={graphs} logp vs score_tokens")


# ------------------------------------------------------------------------------------------------ 5. front end
@pytest.mark.parametrize("stream_rows", [None, 8])
@pytest.mark.parametrize("algo", ["greedy", "multinomial"])
def test_sampler_returns_well_formed_smiles(algo, stream_rows):
    from gct_plus_amd.data import tokenize
    n = 24
    g = torch.Generator().manual_seed(6)
    toklen = torch.randint(8, 20, (n,), generator=g).tolist()
    z = torch.randn(n, max(toklen), 16, generator=g)
    sp = make_sampler("VaetfSampling", "vaetf", algo, stream_rows, well_formed=True)
    smiles, _, toklen_gen = sp.sample_smiles(n, zs=z, toklen=toklen)
    assert len(smiles) == n
    for s, k in zip(smiles, toklen_gen):
        toks = tokenize(s)
        assert 1 <= len(toks) == k <= sp.max_strlen - 2, s                          # the <eos> took a slot of its own
        assert sp.grammar.well_formed(sp.smi_to_id(s, add_eos=True)), s
        assert parses(toks + ["<eos>"]), s
    free = make_sampler("VaetfSampling", "vaetf", algo, stream_rows).sample_smiles(n, zs=z, toklen=toklen)[0]
    assert not all(parses(tokenize(s) + ["<eos>"]) for s in free)                   # the option did something


# ----------------------------------------------------------------- 6. calls on one decoder do not leak into each other
def _call_sequence(graphs):
    """[(graph key of the call's step unit, call)]: the six kinds of call, each returning a tuple of tensors.  4 plain rows
    with prefixes of 3 / 9 / 5 / 3 tokens in ONE start() geometry; a pool of 6 items on 2 stream rows (each row refills);
    max_strlen 12, max_total_len 40."""
    rows, pool = make_pool("pscavaetf", [3, 9, 5, 3], 1, 41), make_pool("pscavaetf", [3, 9, 5, 3, 6, 2], 1, 42)
    lens = rows["lens"]
    uniform, mixed = rows["ys0"][:, :3].cuda(), rows["ys0"].cuda()               # (every row has >= 3 real tokens)

    def plain(kd, ys0, **kw):
        kd.start(cu(rows["z"]), cu(rows["src_mask"]), cu(rows["dconds"]), max_total_len=40)
        out = kd.generate(ys0, 12, use_graphs=graphs, **kw)
        return out if isinstance(out, tuple) else (out,)

    def stream(kd):
        kd.start_stream(cu(pool["z"]), cu(pool["src_mask"]), cu(pool["dconds"]), rows=2, max_total_len=40)
        ys, rec, tl, lp = kd.generate_stream(pool["ys0"].cuda(), 12, prefix_lens=pool["lens"], grammar=GR31,
                                             return_logp=True, use_graphs=graphs)
        assert rec["harvested"] == 6 and all(int((rec["row_of"] == r).sum()) >= 2 for r in range(2))
        return ys, tl, lp, rec["out_len"], rec["row_of"], rec["start_step"]

    return [
        (0, lambda kd: plain(kd, uniform)),
        ((1, "mixed", "logp"), lambda kd: plain(kd, mixed, prefix_lens=lens, algo="multinomial", seed=5,
                                                return_logp=True)),
        ((0, "mixed", "grammar"), lambda kd: plain(kd, mixed, prefix_lens=lens, grammar=GR31)),
        ((0, "stream", "grammar", "logp"), stream),
        (0, lambda kd: plain(kd, uniform)),
        (("filtered", "mixed"), lambda kd: plain(kd, mixed, prefix_lens=lens, **HOW["filtered"])),
    ], (rows, uniform)


def _same(got, want):
    """Token ids, lengths and log-probabilities alike: the same kernels on the same shapes, so bit for bit."""
    return len(got) == len(want) and all(g.dtype == w.dtype and torch.equal(g.cpu(), w.cpu()) and
                                         (not g.dtype.is_floating_point or same_bits(g, w)) for g, w in zip(got, want))


@pytest.mark.parametrize("graphs", [True, False])
def test_calls_on_one_decoder_do_not_leak_into_each_other(graphs):
    """Uniform greedy, mixed multinomial with log-probabilities, mixed greedy with a grammar, a stream with grammar and
    log-probabilities, uniform greedy again, mixed filtered multinomial with neither -- on ONE decoder, each result equal
    to the same call on a fresh decoder.  Then beam search (k = 2, another geometry) and uniform greedy once more.
    Graph keys: every call's unit is captured under the key StepPlan.key predicts and none is False.  The dict is
    checked after every call rather than once at the end, because a captured graph holds the addresses of the rows it
    was captured against: the three plain calls share the 4-row geometry and their graphs, the 2 stream rows and the
    beam rows are other buffers, and start() drops the graphs of the rows it replaces."""
    model = model_of("pscavaetf")
    calls, (rows, uniform) = _call_sequence(graphs)
    kd = KVDecoder(model, PAD, SOS, EOS)
    held = [{0}, {0, (1, "mixed", "logp")}, {0, (1, "mixed", "logp"), (0, "mixed", "grammar")},
            {(0, "stream", "grammar", "logp")}, {0}, {0, ("filtered", "mixed")}]
    seen = set()
    for i, ((key, call), want_keys) in enumerate(zip(calls, held)):
        got, want = call(kd), call(KVDecoder(model, PAD, SOS, EOS))
        assert _same(got, want), (graphs, i, key)
        assert key in want_keys
        if graphs and kd.graph_replay:                   # (the replay guard may choose eager launches on a box)
            assert set(kd.graphs) == want_keys, (i, set(kd.graphs))
            assert all(g is not False for g in kd.graphs.values()), (i, kd.graphs)
            seen |= set(kd.graphs)
        elif not graphs:
            assert kd.graphs == {}
    if graphs and kd.graph_replay:
        assert seen == {k for k, _ in calls}

    def beam(d):
        d.start(cu(rows["z"]), cu(rows["src_mask"]), cu(rows["dconds"]), max_total_len=40, beams=2)
        return d.generate_beam(uniform, 2, 12, use_graphs=graphs)

    assert _same(beam(kd), beam(KVDecoder(model, PAD, SOS, EOS)))
    if graphs and kd.graph_replay:
        assert set(kd.graphs) == {"beam"} and kd.graphs["beam"] is not False
    assert _same(calls[0][1](kd), calls[0][1](KVDecoder(model, PAD, SOS, EOS)))
    if graphs and kd.graph_replay:
        assert set(kd.graphs) == {0} and kd.graphs[0] is not False
