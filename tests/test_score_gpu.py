"""Log-likelihoods on the device: gct_seq_logp / gct_chosen_logp against the rule (decode.score_reference) in fp64,
score_tokens against the oracle and against itself under other chunkings / row plans, the log-probabilities
generate / generate_stream(return_logp=True) return against score_tokens on what they decoded, and the front end.

Tolerances.  Kernel against fp64 log-softmax of the SAME logits: fp32 x - m, expf, a V-term sum, logf and one
subtraction -- a few ulp of a magnitude <= 40 plus V * 2^-24 relative in the sum: under 1e-4 absolute for V <= 1024 and
|logits| <= 16, so atol 1e-4 per token and tokens * 1e-4 per sequence sum.  Device path against the oracle or the
un-cached path: the project's logits tolerance is atol 1e-4, rtol 1e-4, and a log-probability is a logit
minus a log-sum-exp of such logits: 2e-4 + 1e-4 * |logp| per token, the sum of that over a sequence's tokens."""
import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd._lib import GctError
from gct_plus_amd.decode import LOGP, KVDecoder, score_reference, score_tokens
from tests.test_mixed_scaffold_decode_gpu import EOS, PAD, SOS, TINY, build, mixed_prefixes
from tests.test_stream_decode_gpu import emitted_token, make_pool, make_sampler

pytestmark = pytest.mark.gpu

SENT = 7.25


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def cu(t):
    return None if t is None else t.cuda()


def close_tokens(got, ref, what):
    """Per token: |got - ref| <= 2e-4 + 1e-4 |ref| (the device-path tolerance of the module docstring)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    ratio = (got - ref).abs() / (2e-4 + 1e-4 * ref.abs())
    print(f"{what}: worst token error / tolerance {float(ratio.max()):.4f}, worst abs {float((got - ref).abs().max()):.3e}")
    assert bool((ratio <= 1).all()), what


def close_sums(got, ref_token_logp, what):
    """Per sequence: the per-token tolerance summed over the sequence's tokens."""
    ref = ref_token_logp.detach().cpu().double()
    tol = (2e-4 * (ref != 0) + 1e-4 * ref.abs()).sum(1)
    err = (got.detach().cpu().double() - ref.sum(1)).abs()
    print(f"{what}: worst sum error {float(err.max()):.3e}, tolerance there {float(tol[err.argmax()]):.3e}")
    assert bool((err <= tol + 1e-12).all()), what


# ------------------------------------------------------------------------------------------------ 1. gct_seq_logp
SHAPES = [(1, 2, 2), (3, 8, 30), (5, 200, 31), (2, 9, 1024), (67, 5, 30)]


def kernel_case(n, W, V, seed):
    """ys [n, W], prefix_lens [n], logits [n, W - 1, V] fp32 with |x| <= 16.  Row 0 is full and scored from column 1:
    column 1 holds a tie the target wins (lower index), column 2 one it loses, column 3 a -1e4 logit beside the target.
    Row 2 is all pad; the last row's prefix fills it (prefix_lens = W); the other rows end at random columns."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.randint(0, V, (n, W), generator=g)
    ys[ys == PAD] = 0
    end = torch.randint(1, W + 1, (n,), generator=g)
    lens = torch.randint(1, W + 1, (n,), generator=g)
    end[0], lens[0] = W, 1
    if n > 2:
        end[2] = 0
    if n > 1:
        lens[-1] = W
    ys[torch.arange(W)[None, :] >= end[:, None]] = PAD
    x = (torch.randn(n, W - 1, V, generator=g) * 4).clamp(-15, 15)
    ys[0, 1] = 0
    x[0, 0, 0] = x[0, 0, V - 1] = 16.0                                            # tie, the target is the first maximum
    if W > 2:
        ys[0, 2] = V - 1
        x[0, 1, 0] = x[0, 1, V - 1] = 16.0                                        # tie, the target is the second one
    if W > 3:
        x[0, 2, (int(ys[0, 3]) + 1) % V] = -1e4
    return ys, lens, x


@pytest.mark.parametrize("variant", ["plain", "ld", "shift", "no_lens"])
@pytest.mark.parametrize("n,W,V", SHAPES)
def test_seq_logp_against_the_rule(ops, n, W, V, variant):
    ys, lens, x = kernel_case(n, W, V, seed=n * 1000 + W)
    if variant == "no_lens":
        lens = None
    ref_tl, ref_lp, ref_nt, ref_nh = score_reference(x.double(), ys, lens, PAD)
    t0 = torch.ones(n, dtype=torch.long) if lens is None else lens
    scored = (torch.arange(W)[None, :] >= t0[:, None]) & (ys != PAD)
    assert int(ref_nh[0]) >= 1 and int(ref_nh[0]) < int(ref_nt[0]) or W == 2      # the ties are in the scored set
    # device buffer: NaN wherever the kernel has no business reading -- the columns behind V of a strided view, the
    # condition rows in front of a shifted sequence, and the logits rows of columns that are not scored
    shift = 3 if variant == "shift" else 0
    ld = V + 3 if variant == "ld" else V
    R = W - 1 + shift
    big = torch.full((n, R, ld), float("nan"))
    xs = x.clone()
    xs[~scored[:, 1:]] = float("nan")
    big[:, shift:, :V] = xs
    dev = big.cuda().view(n * R, ld)[:, :V]
    args = (dev, ys.cuda(), None if lens is None else lens.int().cuda(), PAD)
    kw = dict(row_shift=shift, rows_per_seq=R)
    tl, lp, nt, nh = ops.seq_logp(*args, **kw)
    tl2, lp2, nt2, nh2 = ops.seq_logp(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(tl, tl2) and torch.equal(lp, lp2) and torch.equal(nt, nt2) and torch.equal(nh, nh2)
    tl, lp = tl.cpu().double(), lp.cpu().double()
    assert bool(torch.isfinite(tl).all()) and bool(torch.isfinite(lp).all())
    assert bool((tl[~scored] == 0).all())
    err = (tl - ref_tl).abs()
    print(f"seq_logp {n, W, V} {variant}: worst token error {float(err.max()):.3e}, worst sum error "
          f"{float((lp - ref_lp).abs().max()):.3e}")
    assert float(err.max()) <= 1e-4
    assert bool(((lp - ref_lp).abs() <= ref_nt.double() * 1e-4 + 1e-12).all())
    assert torch.equal(nt.cpu(), ref_nt) and torch.equal(nh.cpu(), ref_nh)
    if n > 2:
        assert float(lp[2]) == 0 and int(nt[2]) == 0 and int(nh[2]) == 0          # the all-pad row
    if n > 1 and lens is not None:
        assert float(lp[-1]) == 0 and int(nt[-1]) == 0                            # the row its prefix fills


def test_seq_logp_refuses_before_a_launch(ops):
    ys = torch.zeros(1, 257, dtype=torch.long, device="cuda")
    with pytest.raises(GctError, match="257"):
        ops.seq_logp(torch.zeros(256, 30, device="cuda"), ys, None, PAD)
    with pytest.raises(GctError, match="null"):
        ops.seq_logp(None, ys[:, :9], None, PAD, V=30)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------- 2. gct_chosen_logp
def chosen_case():
    g = torch.Generator().manual_seed(3)
    n, V, T = 5, 30, 10
    logits = (torch.randn(n, V, generator=g) * 4).clamp(-16, 16)
    ys = torch.randint(4, V, (n, T), generator=g)
    row_off = torch.tensor([0, 2, 6, 0, 3], dtype=torch.int32)
    p = 6 + 1 - row_off.long()                                                    # [7, 5, 1, 7, 4]
    ys[3, 7] = PAD                                                                # a finished row
    want = torch.log_softmax(logits.double(), -1).gather(1, ys.gather(1, p.view(-1, 1))).view(-1)
    want[3] = 0.0
    return n, V, T, logits, ys, row_off, p, want


def test_chosen_logp_plain_rows(ops):
    n, V, T, logits, ys, row_off, p, want = chosen_case()
    pos = torch.tensor([6], dtype=torch.int32).cuda()
    out = torch.full((n, T), SENT).cuda()
    ops.chosen_logp(logits.cuda(), ys.cuda(), pos, out, PAD, row_off=row_off.cuda())
    out = out.cpu()
    mask = torch.zeros(n, T, dtype=torch.bool)
    mask[torch.arange(n), p] = True
    assert bool((out[~mask] == SENT).all())
    assert float((out[mask].double() - want).abs().max()) <= 1e-4 and float(out[3, 7]) == 0.0
    # without offsets every row sits at *pos + 1
    out = torch.full((n, T), SENT).cuda()
    ops.chosen_logp(logits.cuda(), ys.cuda(), pos, out, PAD)
    out = out.cpu()
    want7 = torch.log_softmax(logits.double(), -1).gather(1, ys[:, 7:8]).view(-1)
    want7[3] = 0.0
    assert float((out[:, 7].double() - want7).abs().max()) <= 1e-4
    out[:, 7] = SENT
    assert bool((out == SENT).all())
    # a column outside the table: nothing is written
    out = torch.full((n, 7), SENT).cuda()
    ops.chosen_logp(logits.cuda(), ys.cuda(), pos, out, PAD)
    assert bool((out == SENT).all())


def test_chosen_logp_streamed_rows(ops):
    """Row 1 is parked; row 2 (item 0) sits at column 1 of an item whose prefix has 2 tokens: both write nothing."""
    n, V, T, logits, ys, row_off, p, want = chosen_case()
    item = torch.tensor([3, -1, 0, 1, 2], dtype=torch.int32)
    prefix_len = torch.tensor([2, 1, 1, 1], dtype=torch.int32)
    pos = torch.tensor([6], dtype=torch.int32).cuda()
    out = torch.full((4, T), SENT).cuda()
    ops.chosen_logp(logits.cuda(), ys.cuda(), pos, out, PAD, row_off=row_off.cuda(), item=item.cuda(),
                    prefix_len=prefix_len.cuda())
    out = out.cpu()
    expect = torch.full((4, T), SENT, dtype=torch.float64)
    expect[3, 7], expect[1, 7], expect[2, 4] = want[0], 0.0, want[4]
    assert bool((out[0] == SENT).all())                                           # item 0: a prefix token
    written = expect != SENT
    assert bool((out[~written] == SENT).all())
    assert float((out[written].double() - expect[written]).abs().max()) <= 1e-4 and float(out[1, 7]) == 0.0
    with pytest.raises(ValueError):
        ops.chosen_logp(logits.cuda(), ys.cuda(), pos, out.cuda(), PAD, row_off=row_off.cuda(), item=item.cuda())


# ------------------------------------------------------------------------------------------------ 3. score_tokens
def target_rows(mtype, seed, lengths=(5, 20, 8, 12, 6, 16)):
    """Full target rows of the given lengths (a multiple of three of them; <sos> [scaffold <sep>] tokens <eos>, pad
    behind), mixed prefixes of 3 / 5 / 4 tokens for the scaffold types: dict(ys, lens or None, z, src_mask, dconds)."""
    g = torch.Generator().manual_seed(seed)
    n, W = len(lengths), max(lengths)
    nc = synthetic.n_conds(mtype)
    if mtype in ("scavaetf", "pscavaetf"):
        ys0, lens = mixed_prefixes([3, 5, 4], n // 3, g)
    else:
        ys0, lens = torch.full((n, 1), SOS), None
    ys = torch.full((n, W), PAD, dtype=torch.long)
    for r, ln in enumerate(lengths):
        t0 = 1 if lens is None else int(lens[r])
        ys[r, :t0] = ys0[r, :t0]
        ys[r, t0:ln - 1] = torch.randint(5, 30, (ln - 1 - t0,), generator=g)
        ys[r, ln - 1] = EOS
    Le = 24
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    return dict(ys=ys, lens=lens, z=z, src_mask=src_mask, dconds=torch.randn(n, nc, generator=g) if nc else None)


NEAR_TIES = []                                            # columns of the whole oracle test that took the allowance


@pytest.mark.parametrize("mtype,c2d", [("vaetf", False), ("pvaetf", False), ("scavaetf", False), ("pscavaetf", False),
                                       ("pvaetf", True)])
def test_score_tokens_vs_oracle(mtype, c2d):
    from oracle import gct_oracle as O
    extra = dict(use_cond2dec=True, use_cond2lat=False) if c2d else {}
    model = build(mtype, seed=31, **extra)
    t = target_rows(mtype, 7)
    ys, lens = t["ys"], t["lens"]
    logp, tokens, hits, tl = score_tokens(model, cu(t["z"]), cu(t["src_mask"]), cu(t["dconds"]), ys.cuda(),
                                          prefix_lens=lens, pad_id=PAD)
    vs, vt = synthetic.vocab_sizes(mtype)
    nc = synthetic.n_conds(mtype)
    cfg = O.make_cfg(mtype, vs, vt, dropout=0.0, nconds=nc, **dict(dict(use_cond2lat=True), **extra), **TINY)
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    trg = ys[:, :-1]
    ref_logits = O.decode(P, cfg, trg, t["z"], t["src_mask"],
                          O.get_trg_mask(trg, PAD, c2d, t["dconds"] if nc else None), t["dconds"])
    ref_logits = ref_logits[:, nc if c2d else 0:]
    ref_tl, ref_lp, ref_nt, ref_nh = score_reference(ref_logits.double(), ys, lens, PAD)
    close_tokens(tl, ref_tl, f"{mtype} c2d={c2d} token_logp vs oracle")
    close_sums(logp, ref_tl, f"{mtype} c2d={c2d} logp vs oracle")
    assert bool((tl.cpu()[ref_tl == 0] == 0).all())
    assert torch.equal(tokens.cpu(), ref_nt)
    assert int(ref_nt.min()) >= 1 and (lens is None or int(ref_nt.sum()) == int(((ys != PAD).sum(1) - lens).sum()))
    top2 = ref_logits.double().topk(2, dim=-1).values
    near = ((top2[..., 0] - top2[..., 1]) < 1e-4) & (ref_tl[:, 1:] != 0)          # scored columns at an oracle near-tie
    for r in range(ys.shape[0]):
        diff = abs(int(hits[r]) - int(ref_nh[r]))
        if diff:
            assert diff <= int(near[r].sum()), (r, int(hits[r]), int(ref_nh[r]))
            NEAR_TIES.extend([(mtype, c2d, r)] * diff)
    assert len(NEAR_TIES) <= 1, NEAR_TIES


def test_score_tokens_does_not_depend_on_chunks_or_the_row_plan(monkeypatch):
    from gct_plus_amd import engine
    model = build("pscavaetf", seed=32)
    # 24 rows: the compact rows come in multiples of 128, and the planner takes them only below 0.85 of all rows --
    # 178 live rows of 456 here.  A chunk of 4 rows (76 rows) is always declined: the results must not care
    t = target_rows("pscavaetf", 8, lengths=(5, 20, 8, 12, 6, 16) + (6, 7, 9, 5, 8, 10) * 3)
    seen = []
    finish = engine.RowPlan.finish

    def spy(self):
        plan = finish(self)
        seen.append(plan.live is not None)
        return plan
    monkeypatch.setattr(engine.RowPlan, "finish", spy)
    res = {}
    for compact in (True, False):
        monkeypatch.setattr(engine, "COMPACT_FWD", compact)
        for chunk in (512, 4):
            seen.clear()
            res[compact, chunk] = score_tokens(model, cu(t["z"]), cu(t["src_mask"]), cu(t["dconds"]), t["ys"].cuda(),
                                               prefix_lens=t["lens"], pad_id=PAD, chunk=chunk)
            assert len(seen) >= (1 if chunk == 512 else 6)
            assert any(seen) == (compact and chunk == 512)  # the planner took the live rows, and only when it may
    lp0, nt0, nh0, tl0 = res[True, 512]
    assert int(nt0.min()) >= 1
    for key, (lp, nt, nh, tl) in res.items():
        close_tokens(tl, tl0, f"compact / chunk {key} vs (True, 512)")
        close_sums(lp, tl0, f"logp, compact / chunk {key}")
        assert torch.equal(nt, nt0)


def test_score_tokens_refuses_before_device_work():
    model = build("vaetf", seed=33)
    z, m = torch.randn(2, 8, TINY["latent_dim"]).cuda(), torch.ones(2, 1, 8, dtype=torch.bool).cuda()
    with pytest.raises(ValueError, match="positional table"):
        score_tokens(model, z, m, None, torch.full((2, 202), 5), pad_id=PAD)
    with pytest.raises(ValueError):
        score_tokens(model, z, m, None, torch.full((2, 9), 999), pad_id=PAD)
    with pytest.raises(ValueError):
        score_tokens(model, z, m, None, torch.full((2, 9), 5), prefix_lens=[0, 1], pad_id=PAD)
    lp, nt, nh, tl = score_tokens(model, z, m, None, torch.full((2, 9), PAD), pad_id=PAD)   # nothing to score
    assert not lp.any() and not nt.any() and not nh.any() and not tl.any()


# -------------------------------------------------------------------------------- 4. what the decoder draws
def first_eos_cut(ys, lens, eos):
    """ys with the columns behind each row's first generated <eos> set to pad, and that span as a mask."""
    n, L = ys.shape
    cols = torch.arange(L)[None, :]
    gen = cols >= lens[:, None]
    is_eos = (ys == eos) & gen
    first = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full((n,), L))
    span = gen & (cols <= first[:, None]) & (ys != PAD)
    clean = torch.where(cols <= first[:, None], ys, torch.full_like(ys, PAD))
    return clean, span


SAMPLING = {"greedy": dict(algo="greedy"), "multinomial": dict(algo="multinomial"),
            "filtered": dict(algo="multinomial", top_k=5, top_p=0.9, temperature=0.7)}


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("how", list(SAMPLING))
def test_generate_returns_the_models_log_probs(how, graphs):
    model = build("pscavaetf", seed=12)
    p = make_pool("pscavaetf", [3, 9, 5, 14], 3, 31)
    eos = emitted_token(model, p, 30) if how == "greedy" else EOS
    kw = dict(SAMPLING[how], seed=5, use_graphs=graphs, prefix_lens=p["lens"])
    kd = KVDecoder(model, PAD, SOS, eos)
    z, m, d = cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"])
    kd.start(z, m, d, max_total_len=60)
    plain = kd.generate(p["ys0"].cuda(), 30, **kw)
    kd.start(z, m, d, max_total_len=60)
    ys, tl, lp = kd.generate(p["ys0"].cuda(), 30, return_logp=True, **kw)
    assert torch.equal(ys, plain)
    assert tl.shape == ys.shape and tl.dtype == torch.float32 and lp.shape == (ys.shape[0],)
    if graphs:
        mode = kd.graphs.keys()
        assert any(isinstance(k, tuple) and k[-1] == LOGP for k in mode) and any(
            isinstance(k, tuple) and k[-1] != LOGP for k in mode)                # a graph of its own per variant
    clean, span = first_eos_cut(ys.cpu(), p["lens"], eos)
    if how == "greedy":
        assert bool((clean != ys.cpu()).any())                                    # rows did end before the last column
    tl = tl.cpu()
    assert bool((tl[~span] == 0).all())
    assert bool((tl[span] <= 0).all()) and bool((tl[span] < 0).any())
    _, nt, _, ref_tl = score_tokens(model, z, m, d, clean.cuda(), prefix_lens=p["lens"], pad_id=PAD)
    assert torch.equal(nt.cpu().long(), span.sum(1))
    close_tokens(tl, ref_tl, f"generate {how} graphs={graphs} token_logp vs score_tokens")
    close_sums(lp, ref_tl, f"generate {how} graphs={graphs} logp vs score_tokens")


def stream_logp(model, p, R, max_strlen, caps, lo=0, hi=None, kd=None, **kw):
    hi = p["ys0"].shape[0] if hi is None else hi
    kd = kd or KVDecoder(model, PAD, SOS, EOS)
    cut = lambda t: None if t is None else t[lo:hi].cuda()                      # noqa: E731
    kd.start_stream(cut(p["z"]), cut(p["src_mask"]), cut(p["dconds"]), rows=R,
                    max_total_len=p["ys0"].shape[1] + max_strlen + 8, item_base=lo)
    ys, rec, tl, lp = kd.generate_stream(p["ys0"][lo:hi].cuda(), max_strlen, prefix_lens=p["lens"][lo:hi],
                                         max_new_tokens=caps[lo:hi], return_logp=True, **kw)
    assert rec["harvested"] == hi - lo and tl.shape == ys.shape
    return ys.cpu(), rec, tl.cpu(), lp.cpu()


@pytest.mark.parametrize("graphs", [False, True])
def test_generate_stream_returns_the_models_log_probs(graphs):
    model = build("pscavaetf", seed=11)
    R = 8
    N = 5 * R + 3
    p = make_pool("pscavaetf", torch.randint(1, 15, (N,), generator=torch.Generator().manual_seed(2)).tolist(), 1, 23)
    caps = torch.randint(1, 20, (N,), generator=torch.Generator().manual_seed(5))
    kw = dict(algo="multinomial", seed=9, use_graphs=graphs)
    ys, rec, tl, lp = stream_logp(model, p, R, 20, caps, **kw)
    assert int(rec["start_step"].max()) > 0                                       # refills did happen
    cols = torch.arange(ys.shape[1])[None, :]
    lens, out_len = p["lens"], rec["out_len"]
    span = (cols >= lens[:, None]) & (cols < (lens + out_len)[:, None])
    assert bool((tl[~span] == 0).all())                                           # also what held rows wrote meanwhile
    assert bool((ys[~span & (cols >= lens[:, None])] == PAD).all())
    span &= ys != PAD                                                             # (a draw may be the pad token: not scored)
    assert bool((tl[~span] == 0).all()) and bool((tl[span] < 0).all())
    assert torch.allclose(lp, tl.sum(1), rtol=0, atol=1e-4)
    _, nt, _, ref_tl = score_tokens(model, cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), ys.cuda(),
                                    prefix_lens=lens, pad_id=PAD)
    assert torch.equal(nt.cpu().long(), span.sum(1))
    close_tokens(tl, ref_tl, f"stream graphs={graphs} token_logp vs score_tokens")
    close_sums(lp, ref_tl, f"stream graphs={graphs} logp vs score_tokens")
    # an item does not depend on the schedule: the pool in slices of R items with the ids kept, bit for bit
    width = ys.shape[1]
    for lo in range(0, N, R):
        hi = min(lo + R, N)
        ys_s, rec_s, tl_s, _ = stream_logp(model, p, R, 20, caps, lo=lo, hi=hi, **kw)
        assert int(rec_s["start_step"].max()) == 0 and torch.equal(rec_s["out_len"], out_len[lo:hi])
        w = min(width, ys_s.shape[1])
        assert torch.equal(ys_s[:, :w], ys[lo:hi, :w])
        assert torch.equal(tl_s[:, :w], tl[lo:hi, :w]), (lo, hi)
        assert not tl_s[:, w:].any() and not tl[lo:hi, w:].any()


def test_full_size_generate_with_log_probs():
    """d = 512, N = 6, 64 rows, graph replay: the recorded log-probabilities against score_tokens on the same ids."""
    model = build("pscavaetf", full=True, seed=3)
    p = make_pool("pscavaetf", [3, 30, 7, 12, 4, 21, 16, 9], 8, 17, Le=40, full=True)
    z, m, d = cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"])
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start(z, m, d, max_total_len=80)
    ys, tl, lp = kd.generate(p["ys0"].cuda(), 40, use_graphs=True, prefix_lens=p["lens"], return_logp=True)
    clean, span = first_eos_cut(ys.cpu(), p["lens"], EOS)
    assert bool((tl.cpu()[~span] == 0).all()) and int(span.sum()) > 64
    _, nt, _, ref_tl = score_tokens(model, z, m, d, clean.cuda(), prefix_lens=p["lens"], pad_id=PAD)
    assert torch.equal(nt.cpu().long(), span.sum(1))
    close_tokens(tl, ref_tl, "full-size generate token_logp vs score_tokens")
    close_sums(lp, ref_tl, "full-size generate logp vs score_tokens")


# ------------------------------------------------------------------------------------------------ 5. front end
SCAFFOLD = "c1ccccc1"


def test_sample_smiles_with_logp():
    n = 9
    g = torch.Generator().manual_seed(6)
    z = torch.randn(n, 30, 16, generator=g)
    dconds = torch.rand(n, 3, generator=g).numpy()
    for rows in (None, 4):
        sp = make_sampler("PscavaetfSampling", "pscavaetf", "multinomial", rows, with_logp=True)
        out = sp.sample_smiles(dconds, SCAFFOLD, zs=z, transform=False)
        assert len(out) == 4 and len(out[0]) == n
        logp = out[3]
        assert logp.shape == (n,) and logp.dtype == torch.float32 and not logp.is_cuda
        assert bool((logp <= 0).all()) and bool((logp < 0).any())
        out = sp.sample_multiple_smiles(dconds, [SCAFFOLD, "CC", "C1CCNCC1"] * 3, zs=z, transform=False)
        assert len(out) == 4 and out[3].shape == (n,) and bool((out[3] <= 0).all())
        plain = make_sampler("PscavaetfSampling", "pscavaetf", "multinomial", rows)
        out3 = plain.sample_smiles(dconds, SCAFFOLD, zs=z, transform=False)
        assert len(out3) == 3 and isinstance(out3[0], list)
    sv = make_sampler("VaetfSampling", "vaetf", "greedy", None, with_logp=True)
    out = sv.sample_smiles(n, zs=z[:, :, :16])
    assert len(out) == 4 and out[3].shape == (n,) and bool((out[3] <= 0).all())
    assert len(make_sampler("VaetfSampling", "vaetf", "greedy", None).sample_smiles(n, zs=z)) == 3


def test_score_smiles_reconstruction():
    from gct_plus_amd.data import tokenize
    from tests.test_data_pipeline import SMILES
    smiles = list(SMILES)[:6]
    sv = make_sampler("VaetfSampling", "vaetf", "greedy", None)
    s = sv.score_smiles(smiles)
    want = torch.tensor([len(tokenize(x, sv.add_sep)) + 1 for x in smiles], dtype=torch.int32)
    assert torch.equal(s.tokens, want) and bool((s.hits <= s.tokens).all()) and bool((s.hits >= 0).all())
    assert s.logp.shape == (6,) and bool((s.logp < 0).all()) and not s.logp.is_cuda
    assert s.token_logp.shape == (6, int(want.max()) + 1) and bool((s.token_logp[:, 0] == 0).all())
    sp = make_sampler("PscavaetfSampling", "pscavaetf", "greedy", None)
    conds = torch.rand(6, 3, generator=torch.Generator().manual_seed(1)).numpy()
    s = sp.score_smiles(smiles, [SCAFFOLD] * 6, conds, transform=False)
    assert torch.equal(s.tokens, want) and bool((s.hits <= s.tokens).all()) and bool((s.logp < 0).all())
    t0 = len(tokenize(SCAFFOLD, True)) + 2
    assert not s.token_logp[:, :t0].any() and bool((s.token_logp[:, t0] < 0).all())   # the prefix is not scored


def test_score_smiles_of_sampled_molecules_gives_their_logp():
    """Greedy sample_smiles(zs=zs) with with_logp, then score_smiles(those molecules, zs=zs): the same number, for the
    molecules whose SMILES string tokenises back to the ids that were decoded and that ended with <eos> (the score's
    target ends with <eos>).  The randomly initialised model is steered so that such molecules exist: the special tokens
    are never the top choice, and the output row of the token greedy emits most often is swapped with <eos>'s."""
    n = 16
    sv = make_sampler("VaetfSampling", "vaetf", "greedy", None, with_logp=True)
    z = torch.randn(n, 20, 16, generator=torch.Generator().manual_seed(8))
    out = sv.model.out
    special = [sv.TRG.stoi[t] for t in ("<pad>", "<sos>", "<unk>", "<sep>") if t in sv.TRG.stoi]
    with torch.no_grad():
        out.bias[special] = -30.0
        ids = sv.decode(z, sv.init_y(n), torch.ones(n, 1, 20, dtype=torch.bool))[0][:, 1:].cpu()
        x = int(torch.bincount(ids[(ids != sv.eos_id) & (ids != sv.pad_id)].view(-1)).argmax())
        pair, riap = [x, sv.eos_id], [sv.eos_id, x]
        out.weight[pair], out.bias[pair] = out.weight[riap].clone(), out.bias[riap].clone()
    if hasattr(sv.model, "invalidate_weight_planes"):
        sv.model.invalidate_weight_planes()
    ids, logp = sv.decode(z, sv.init_y(n), torch.ones(n, 1, 20, dtype=torch.bool))
    ids = ids[:, 1:].cpu().tolist()
    smiles, _, _, logp2 = sv.sample_smiles(n, zs=z)
    keep = [i for i in range(n) if sv.eos_id in ids[i]
            and sv.smi_to_id(smiles[i]) == ids[i][:ids[i].index(sv.eos_id)]]
    print(f"{len(keep)} of {n} greedy molecules end with <eos> and tokenise back to their ids")
    assert len(keep) >= 1
    s = sv.score_smiles([smiles[i] for i in keep], zs=z[keep])
    assert torch.equal(s.tokens.long(), torch.tensor([ids[i].index(sv.eos_id) + 1 for i in keep]))
    close_sums(logp2[keep], s.token_logp, "score_smiles of the sampled molecules vs the run's logp")
    close_sums(logp[keep], s.token_logp, "the same through decode")
