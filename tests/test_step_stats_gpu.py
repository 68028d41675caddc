"""Per-step sampling statistics on the device: gct_step_stats against the fp64 reference (tests/step_stats_ref.py, its
bounds), one real step grammar mask -> filtered selection -> statistics, the tables generate / generate_stream
(return_stats=True) return -- their invariances bit for bit and their values against a recomputation from the
teacher-forced logits of the decoded rows -- and the weighted fine-tuning step.

Tolerances.  Kernel against fp64 on the SAME logits and probs: step_stats_bounds (derived in tests/step_stats_ref.py
from the fp32 operation count over V terms).  Device path against the teacher-forced recomputation: the project's logits
tolerance e_v = 1e-4 + 1e-4 |x_v| pushed through each term with its derivative, as test_policy_terms_gpu.py
does, plus 1e-4 for the term's own fp32 arithmetic.  With q = softmax(masked x / T) (temperature and grammar only: no
top-k / nucleus set whose membership could flip between two computations of the logits), p = softmax(x):
  model_entropy      sum_v |p_v (log p_v + H)| e_v
  behaviour_logp     sum_v |[v == tok] - q_v| e_v / T
  behaviour_entropy  sum_v |q_v (log q_v + H_q)| e_v / T
  behaviour_kl       sum_v (|q_v ((log q_v - log p_v) - KL)| / T + |q_v - p_v|) e_v
"""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd.decode import (FILTERED, GRAMMAR, LOGP, MIXED, STATS, KVDecoder, StepStats, _scoring_logits,
                                 generated_tokens, sample_filter_reference)
from tests.step_stats_ref import NAMES, make_case, step_stats_bounds, step_stats_ref
from tests.test_grammar_gpu import GR31, cu, model_of, walk
from tests.test_grammar_host import EOS, PAD, SOS
from tests.test_mixed_scaffold_decode_gpu import TINY, mixed_prefixes

pytestmark = pytest.mark.gpu

GUARD = 64                                               # floats behind each table that nothing may touch
ERR_ARG = -1                                             # GCT_ERR_ARG


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def nan_tables(k, rows, T):
    """k tables [rows, T] of NaN, each a view of a buffer with GUARD more NaNs behind it: (tables, buffers)."""
    bufs = [torch.full((rows * T + GUARD,), float("nan"), device="cuda") for _ in range(k)]
    return [b[:rows * T].view(rows, T) for b in bufs], bufs


# --------------------------------------------------------------------------------------- 1. the kernel, the rule
def layout_case(n, layout, seed, T=9):
    """Where the rows of a step sit: (pos, row_off, item, prefix_len, out_rows, acts [n] bool, p [n], dst [n]).
    uniform: every row at column *pos + 1.  row_off: row r at *pos + 1 - row_off[r].  stream: rows work on the items of a
    permutation; with n >= 2 the second row is parked, with n >= 3 the third is inside its item's prefix."""
    g = np.random.default_rng(seed)
    pos = 5
    if layout == "uniform":
        return pos, None, None, None, n, np.ones(n, bool), np.full(n, pos + 1), np.arange(n)
    row_off = g.integers(0, 4, n).astype(np.int32)
    p = pos + 1 - row_off
    if layout == "row_off":
        return pos, row_off, None, None, n, np.ones(n, bool), p, np.arange(n)
    items = n + 2
    item = g.permutation(items)[:n].astype(np.int32)
    prefix_len = np.ones(items, dtype=np.int32)
    acts = np.ones(n, bool)
    if n >= 2:
        item[1], acts[1] = -1, False
    if n >= 3:
        prefix_len[item[2]], acts[2] = p[2] + 1, False
    return pos, row_off, item, prefix_len, items, acts, p, item.astype(np.int64)


def run_kernel(ops, x, q, ys, lay, greedy, which=NAMES, T=9):
    """One gct_step_stats launch on NaN tables: ({name: table on the CPU}, buffers)."""
    pos, row_off, item, prefix_len, out_rows = lay[:5]
    tabs, bufs = nan_tables(len(which), out_rows, T)
    dev = lambda a, dt=None: None if a is None else torch.as_tensor(a, dtype=dt).cuda()     # noqa: E731
    ops.step_stats(dev(x), dev(q), dev(ys), torch.tensor([pos], dtype=torch.int32).cuda(), PAD, greedy=greedy,
                   row_off=dev(row_off), item=dev(item), prefix_len=dev(prefix_len), **dict(zip(which, tabs)))
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[-GUARD:]).all())                                # nothing behind a table
    return {name: t.cpu() for name, t in zip(which, tabs)}


@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 130, 1024])
def test_kernel_against_the_reference(ops, V):
    T, worst = 9, np.zeros(4)
    for n in (0, 1, 3, 5, 9):
        for layout in ("uniform", "row_off", "stream"):
            for mode in ("none", "probs", "greedy"):
                x, q, _, tok = make_case(max(n, 1), V, 100 * n + V, PAD, "probs" if mode == "probs" else "none")
                x, tok, q = x[:n], tok[:n], None if q is None else q[:n]
                if mode == "greedy":                                              # greedy ignores a probs row it is given
                    q = make_case(max(n, 1), V, 7, PAD, "probs")[1][:n]
                lay = layout_case(n, layout, 31 * n + V, T)
                pos, row_off, item, prefix_len, out_rows, acts, p, dst = lay
                if n >= 4:
                    tok[3] = PAD                                                  # a finished row
                ys = np.full((n, T), 2, dtype=np.int64)                          # (every other column: a live token)
                ys[np.arange(n), p] = tok
                got = run_kernel(ops, x, q, ys, lay, mode == "greedy", T=T)
                kw = dict(greedy=mode == "greedy")
                qref = None if mode != "probs" else q
                ref, bound = step_stats_ref(x, qref, tok, PAD, **kw), step_stats_bounds(x, qref, tok, PAD, **kw)
                written = np.zeros((out_rows, T), bool)
                for k, name in enumerate(NAMES):
                    t = got[name].double().numpy()
                    for r in range(n):
                        if not acts[r]:
                            continue
                        written[dst[r], p[r]] = True
                        err = abs(t[dst[r], p[r]] - ref[k, r])
                        assert err <= bound[k, r], (name, V, n, layout, mode, r, t[dst[r], p[r]], ref[k, r], bound[k, r])
                        if bound[k, r] > 0:
                            worst[k] = max(worst[k], err / bound[k, r])
                    assert np.isnan(t[~written]).all() and not np.isnan(t[written]).any(), (name, V, n, layout, mode)
                if n >= 4 and acts[3]:
                    assert all(float(got[name][dst[3], p[3]]) == 0.0 for name in NAMES)            # the finished row
                if mode == "none" and n:                                          # the three bit identities
                    out = torch.full((out_rows, T), float("nan")).cuda()
                    dev = lambda a: None if a is None else torch.as_tensor(a).cuda()    # noqa: E731
                    ops.chosen_logp(torch.as_tensor(x).cuda(), torch.as_tensor(ys).cuda(),
                                    torch.tensor([pos], dtype=torch.int32).cuda(), out, PAD, row_off=dev(row_off),
                                    item=dev(item), prefix_len=dev(prefix_len))
                    assert same_bits(got["behaviour_logp"], out), (V, n, layout)
                    assert same_bits(got["behaviour_entropy"], got["model_entropy"])
                    kl = got["behaviour_kl"]
                    assert bool((kl[~torch.isnan(kl)] == 0).all())
                if n == 5:                                                        # each output pointer alone
                    for name in NAMES:
                        alone = run_kernel(ops, x, q, ys, lay, mode == "greedy", which=(name,), T=T)
                        assert same_bits(alone[name], got[name]), (name, V, layout, mode)
    print(f"step_stats V={V}: worst error / bound per output {dict(zip(NAMES, np.round(worst, 4)))}")


def test_kernel_leaves_columns_outside_the_table_alone(ops):
    x, q, _, tok = make_case(5, 30, 3, PAD, "probs")
    ys = np.full((5, 9), 2, dtype=np.int64)
    ys[:, 6] = tok
    lay = layout_case(5, "uniform", 0)
    got = run_kernel(ops, x, q, ys, lay, False, T=6)                              # column 6 of a table 6 wide
    assert all(bool(torch.isnan(t).all()) for t in got.values())
    # item 7 of a table of 4 rows: dst >= out_rows
    lay = (5, np.zeros(5, dtype=np.int32), np.array([0, 1, 7, 2, 3], dtype=np.int32), np.ones(8, dtype=np.int32), 4)
    got = run_kernel(ops, x, q, ys, lay, False)
    for t in got.values():
        assert bool(torch.isnan(t[:, :6]).all()) and not bool(torch.isnan(t[:, 6]).any())


def test_refusals_come_before_a_launch(ops):
    from gct_plus_amd._lib import GctError
    n, V, T = 3, 30, 8
    L = ops._L()
    x, ys = torch.zeros(n, V).cuda(), torch.full((n, T), 2, dtype=torch.int64).cuda()
    pos, i32 = torch.tensor([3], dtype=torch.int32).cuda(), torch.zeros(n, dtype=torch.int32).cuda()
    tabs, bufs = nan_tables(4, n, T)
    st = ops._st()

    def call(logits=x, ys_=ys, pos_=pos, row_off=None, item=None, prefix_len=None, outs=tabs, V_=V, n_=n):
        p = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        return L.gct_step_stats(p(logits), None, V_, p(ys_), T, p(pos_), p(row_off), p(item), p(prefix_len), PAD, 0,
                                *[p(t) for t in outs], T, n, n_, st)

    for kw in (dict(logits=None), dict(ys_=None), dict(pos_=None), dict(outs=[None] * 4), dict(V_=0), dict(n_=-1),
               dict(item=i32), dict(item=i32, prefix_len=i32), dict(prefix_len=i32, row_off=i32)):
        assert call(**kw) == ERR_ARG, kw
        assert "step_stats" in L.gct_last_error().decode()
    assert call(n_=0) == 0                                                        # nothing to do: no launch
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs)                          # outputs untouched by all of the above
    # the binding's own checks
    for kw in (dict(), dict(model_entropy=tabs[0], behaviour_kl=tabs[1][:, :4]), dict(model_entropy=tabs[0].double()),
               dict(entropy=tabs[0])):
        with pytest.raises((ValueError, GctError)):
            ops.step_stats(x, None, ys, pos, PAD, **kw)
    with pytest.raises(ValueError):
        ops.step_stats(x, torch.zeros(n, V + 1).cuda(), ys, pos, PAD, model_entropy=tabs[0])
    with pytest.raises(ValueError):
        ops.step_stats(x, None, ys, pos, PAD, model_entropy=tabs[0], item=i32, row_off=i32)
    assert call() == 0                                                            # and the call they all vary is a good one
    torch.cuda.synchronize()
    assert not bool(torch.isnan(tabs[0][:, 4]).any())


# ---------------------------------------------------------------------------------------------- 2. one real step
def test_one_real_step_mask_select_stats(ops):
    """gct_grammar_mask -> gct_select_token(top-k and nucleus on, probs_out) -> gct_step_stats: behaviour_logp is the log
    of the probs_out entry of the token ys received, and all four tables follow the rule on (raw logits, probs_out)."""
    import random
    n, V, T, g_len = 37, len(GR31), 10, 3
    rng, g = random.Random(5), torch.Generator().manual_seed(5)
    x = torch.randn(n, V, generator=g) * 2
    ys = torch.full((n, T), PAD)
    ys[:, 0] = SOS
    for r in range(n):
        h = walk(GR31, 12, rng, g_len)
        while EOS in h or PAD in h:                                               # a history that is still open
            h = walk(GR31, 12, rng, g_len)
        ys[r, 1:1 + g_len] = torch.tensor(h)
    col = 1 + g_len
    pos = torch.tensor([col - 1], dtype=torch.int32).cuda()
    xd, ysd = x.cuda(), ys.cuda()
    masked, probs = torch.empty_like(xd), torch.full((n, V), float("nan")).cuda()
    ops.grammar_mask(xd, masked, GR31.device_table("cuda"), ysd, pos, gram=torch.tensor([12, 1], dtype=torch.int32).cuda())
    ops.select_token(masked, ysd, 0, torch.zeros(n, T, dtype=torch.uint8).cuda(), torch.zeros(n, dtype=torch.uint8).cuda(),
                     1, PAD, EOS, seed=17, probs_out=probs, pos_dev=pos,
                     filt_dev=ops.sample_filter_settings(5, 0.9, 1.0, V).cuda())
    tabs, _ = nan_tables(4, n, T)
    ops.step_stats(xd, probs, ysd, pos, PAD, **dict(zip(NAMES, tabs)))
    torch.cuda.synchronize()
    tok, q = ysd[:, col].cpu().numpy(), probs.cpu().numpy()
    off = torch.isneginf(GR31.mask_reference(x, ys, 1, col, 12)).numpy()
    assert (q[off] == 0).all() and (q[np.arange(n), tok] > 0).all() and (tok != PAD).all()
    assert (q == 0).sum() > off.sum()                                             # the nucleus cut tokens the grammar allows
    ref, bound = step_stats_ref(x.numpy(), q, tok, PAD), step_stats_bounds(x.numpy(), q, tok, PAD)
    got = np.stack([t[:, col].cpu().double().numpy() for t in tabs])
    assert (np.abs(got[1] - np.log(q[np.arange(n), tok].astype(np.float64))) <= bound[1]).all()
    assert (np.abs(got - ref) <= bound).all(), np.abs(got - ref).max(-1)
    for t in tabs:
        rest = t.clone()
        rest[:, col] = float("nan")
        assert bool(torch.isnan(rest).all())


# ------------------------------------------------------------------------------------------------ 3. end to end
def rows6(seed=33):
    """n = 6 rows of the tiny pscavaetf model with scaffold prefixes of 3 and 5 tokens (rows interleaved)."""
    g = torch.Generator().manual_seed(seed)
    ys0, lens = mixed_prefixes([3, 5], 3, g)
    n, Le = 6, 23
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    return dict(z=z, src_mask=src_mask, dconds=torch.randn(n, 3, generator=g), ys0=ys0, lens=lens)


MAXLEN = 12
FILT = dict(algo="multinomial", seed=9, top_k=5, top_p=0.9, temperature=0.8, grammar=GR31)


def gen(model, p, kd=None, lens="own", **kw):
    kd = kd or KVDecoder(model, PAD, SOS, EOS)
    kd.start(cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), max_total_len=p["ys0"].shape[1] + 30)
    return kd.generate(p["ys0"].cuda(), MAXLEN, prefix_lens=p["lens"] if lens == "own" else lens, **kw), kd


def stream(model, p, R, **kw):
    kd = KVDecoder(model, PAD, SOS, EOS)
    kd.start_stream(cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), rows=R, max_total_len=40)
    return kd.generate_stream(p["ys0"].cuda(), MAXLEN, prefix_lens=p["lens"], **kw)


def check_tables(ys, lens, st):
    """The shape of a StepStats: tables like ys, 0 off the generated span, entropies and the KL not negative on it,
    the behaviour's log-probability not positive, and the row sum."""
    assert isinstance(st, StepStats) and all(t.shape == ys.shape and t.dtype == torch.float32 for t in st[:4])
    ys, tabs = ys.cpu(), [t.cpu() for t in st]
    cols = torch.arange(ys.shape[1])[None, :]
    is_eos = (ys == EOS) & (cols >= lens[:, None])
    assert bool(is_eos.any(1).all())                                              # the grammar ends every row
    span = (cols >= lens[:, None]) & (cols <= is_eos.int().argmax(1)[:, None])
    for t in tabs[:4]:
        assert bool((t[~span] == 0).all()) and bool(torch.isfinite(t).all())
    assert bool((tabs[0][span] > 0).all()) and bool((tabs[1][span] <= 0).all()) and bool((tabs[2][span] >= 0).all())
    assert bool((tabs[3][span] > -1e-5).all()) and bool((tabs[3][span] > 1e-3).any())   # a filter is on: KL(q || p) > 0
    assert torch.allclose(tabs[4], tabs[1].sum(1), rtol=0, atol=1e-4)
    return span


def test_tables_do_not_depend_on_how_the_rows_are_run():
    model, p = model_of("pscavaetf"), rows6()
    kw = dict(FILT, return_stats=True, return_logp=True)
    (ys, tl, lp, st), kd = gen(model, p, **kw)
    check_tables(ys, p["lens"], st)
    # eager against graph replay
    (ys_g, tl_g, lp_g, st_g), kd = gen(model, p, kd=kd, use_graphs=True, **kw)
    assert (FILTERED, MIXED, GRAMMAR, LOGP, STATS) in kd.graphs
    assert torch.equal(ys_g, ys) and same_bits(tl_g, tl) and all(same_bits(a, b) for a, b in zip(st_g, st))
    # the rows of the 3-token scaffold in a batch that holds that scaffold everywhere (uniform rows)
    A = (p["lens"] == 3).nonzero().view(-1)
    pu = dict(p, ys0=p["ys0"][A[0], :3].view(1, 3).repeat(6, 1), lens=None)
    (ys_u, tl_u, lp_u, st_u), _ = gen(model, pu, **kw)
    G = MAXLEN - 1
    assert torch.equal(ys_u[A, 3:3 + G], ys[A, 3:3 + G])
    for a, b in zip(st_u[:4], st[:4]):
        assert same_bits(a[A, 3:3 + G], b[A, 3:3 + G])
    # per molecule, between continuous batching through 2 rows and through 6
    ys2, rec2, tl2, lp2, st2 = stream(model, p, 2, **kw)
    ys6, rec6, tl6, lp6, st6 = stream(model, p, 6, **kw)
    assert int(rec2["start_step"].max()) > 0 and int(rec6["start_step"].max()) == 0
    check_tables(ys2, p["lens"], st2)
    w = min(ys2.shape[1], ys6.shape[1])
    assert torch.equal(ys2[:, :w], ys6[:, :w]) and torch.equal(rec2["out_len"], rec6["out_len"])
    for a, b in zip(st2[:4], st6[:4]):
        assert same_bits(a[:, :w], b[:, :w]) and not a[:, w:].any() and not b[:, w:].any()
    assert torch.allclose(st2[4], st6[4], rtol=0, atol=1e-5)


def recomputed(model, p, ys, T):
    """The four terms of every generated token of ys from the teacher-forced logits of the decoded rows, in fp64, with
    the pushed-through tolerance of each: (ref [4, n, L], tol [4, n, L], span [n, L])."""
    lens, n, L = p["lens"], ys.shape[0], ys.shape[1]
    ys = ys.cpu()
    cols = torch.arange(L)[None, :]
    is_eos = (ys == EOS) & (cols >= lens[:, None])
    span = (cols >= lens[:, None]) & (cols <= is_eos.int().argmax(1)[:, None])
    with torch.no_grad():
        logits2d, rows = _scoring_logits(model, cu(p["z"]), cu(p["src_mask"]), cu(p["dconds"]), ys.cuda(),
                                         lens.cuda(), PAD, False)
    logits = logits2d.view(n, rows, -1).cpu()
    ref, tol = torch.zeros(4, n, L, dtype=torch.float64), torch.ones(4, n, L, dtype=torch.float64)
    rr, cc = span.nonzero(as_tuple=True)
    x = logits[rr, cc - 1].double()                                               # row c - 1 predicts token c
    masked = GR31.mask_reference(x, ys[rr], lens[rr].tolist(), cc.tolist(), MAXLEN - 1)
    q = sample_filter_reference(masked, temperature=T).double()                   # (its softmax is fp32: 1e-7, far below tol)
    tok = ys[rr, cc]
    out = step_stats_ref(x.numpy(), q.numpy(), tok.numpy(), PAD)
    lp = torch.log_softmax(x, -1)
    pr, lq = lp.exp(), torch.log(torch.where(q > 0, q, torch.ones_like(q)))
    H, Hq = -(pr * lp).sum(-1, keepdim=True), -(q * lq).sum(-1, keepdim=True)
    KL = (q * (lq - lp)).sum(-1, keepdim=True)
    e = 1e-4 + 1e-4 * x.abs()
    hot = torch.zeros_like(q).scatter_(1, tok.view(-1, 1), 1.0)
    t = [((pr * (lp + H)).abs() * e).sum(-1), ((hot - q).abs() * e).sum(-1) / T,
         ((q * (lq + Hq)).abs() * e).sum(-1) / T, (((q * ((lq - lp) - KL)).abs() / T + (q - pr).abs()) * e).sum(-1)]
    for k in range(4):
        ref[k, rr, cc] = torch.as_tensor(out[k])
        tol[k, rr, cc] = 1e-4 + t[k]
    return ref, tol, span


def test_tables_against_the_teacher_forced_recomputation():
    model, p, T = model_of("pscavaetf"), rows6(41), 0.7
    kw = dict(algo="multinomial", seed=4, temperature=T, grammar=GR31, return_stats=True)
    (ys, st), _ = gen(model, p, **kw)
    ys_s, rec, st_s = stream(model, p, 2, **kw)
    for what, y, s in (("generate", ys, st), ("stream", ys_s, st_s)):
        ref, tol, span = recomputed(model, p, y, T)
        assert int(span.sum()) >= 12                                              # two tokens per row at the least
        for k, name in enumerate(NAMES):
            got = s[k].cpu().double()
            ratio = ((got - ref[k]).abs() / tol[k])[span]
            print(f"{what} {name}: worst error / tolerance {float(ratio.max()):.4f} over {int(span.sum())} tokens")
            assert bool((ratio <= 1).all()), (what, name)                         # every generated token of every row
            assert bool((got[~span] == 0).all())
        assert torch.allclose(s.behaviour_logp_sum.cpu().double(), ref[1].sum(1), rtol=0, atol=float(tol[1][span].sum()))


def test_without_return_stats_nothing_changes():
    model, p = model_of("pscavaetf"), rows6()
    kw = dict(FILT, use_graphs=True)
    (ys_s, tl_s, lp_s, st), kd_s = gen(model, p, return_logp=True, return_stats=True, **kw)
    out, kd = gen(model, p, return_logp=True, **kw)
    assert isinstance(out, tuple) and len(out) == 3 and torch.equal(out[0], ys_s) and same_bits(out[1], tl_s)
    plain, kd = gen(model, p, kd=kd, **kw)
    assert torch.is_tensor(plain) and torch.equal(plain, ys_s)
    assert set(kd.graphs) == {(FILTERED, MIXED, GRAMMAR, LOGP), (FILTERED, MIXED, GRAMMAR)}
    assert "probs" not in kd.buf and kd.stats_tab is None                         # nothing allocated, nothing launched
    assert set(kd_s.graphs) == {(FILTERED, MIXED, GRAMMAR, LOGP, STATS)} and "probs" in kd_s.buf
    only, _ = gen(model, p, return_stats=True, **FILT)                            # stats without the log-probabilities
    assert len(only) == 2 and torch.equal(only[0], ys_s) and all(same_bits(a, b) for a, b in zip(only[1], st))
    ys2, rec = stream(model, p, 2, **FILT)
    assert torch.is_tensor(ys2) and isinstance(rec, dict)
    # greedy and the plain multinomial draw record their own behaviour: the one-hot, and the model itself
    (yg, sg), kg = gen(model, p, algo="greedy", grammar=GR31, return_stats=True)
    span = check_span(yg, p["lens"])
    assert not sg.behaviour_logp.any() and not sg.behaviour_entropy.any() and "probs" not in kg.buf
    assert bool((sg.behaviour_kl.cpu()[span] > 0).all())
    (ym, tlm, lpm, sm), km = gen(model, p, algo="multinomial", seed=3, return_logp=True, return_stats=True)
    assert same_bits(sm.behaviour_logp, tlm) and same_bits(sm.behaviour_entropy, sm.model_entropy)
    assert not sm.behaviour_kl.any() and "probs" not in km.buf and same_bits(sm.behaviour_logp_sum, lpm)


def check_span(ys, lens):
    ys = ys.cpu()
    cols = torch.arange(ys.shape[1])[None, :]
    is_eos = (ys == EOS) & (cols >= lens[:, None])
    first = torch.where(is_eos.any(1), is_eos.int().argmax(1), torch.full((ys.shape[0],), ys.shape[1]))
    return (cols >= lens[:, None]) & (cols <= first[:, None]) & (ys != PAD)


# ------------------------------------------------------------------------------------- 4. samplers, fine-tuning
def make_sampler(**kw):
    """test_sbs_gpu.py's sampler over the SMILES vocabulary, with a dropout-0 model (so that training-mode and eval-mode
    log-probabilities agree) built from one seed."""
    from gct_plus_amd import data
    from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling
    from gct_plus_amd.Model import model_dict
    from tests.test_data_pipeline import SMILES
    strs = ["c1ccccc1<sep>" + s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    torch.manual_seed(4)
    model = model_dict["pscavaetf"](len(SRC), len(TRG), dropout=0.0, nconds=3, use_cond2lat=True, **TINY).cuda().eval()
    return PscavaetfSampling(model, SRC, TRG, latent_dim=16, max_strlen=14, cond_dim=3, decode_algo="multinomial",
                             toklen_data=[12, 14, 15, 18, 20, 16], seed=2, **kw)


def test_sampler_returns_the_stats_and_unit_weights_change_nothing():
    from gct_plus_amd.Inference.sampling_tool import DecodedRows
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import behaviour_weights, ppo_update, reinforce_step
    n = 6
    z = torch.randn(n, 26, 16, generator=torch.Generator().manual_seed(9))
    done = []
    for weight in (None, torch.ones(n)):
        sp = make_sampler(with_logp=True, with_stats=True, well_formed=True, top_p=0.9, temperature=0.8)
        smiles, toklen, gen_len, logp, st, rows = sp.sample_smiles(np.ones((n, 3)) * 0.3, "c1ccccc1", zs=z,
                                                                   transform=False, return_rows=True)
        assert isinstance(st, StepStats) and isinstance(rows, DecodedRows) and not st.behaviour_logp.is_cuda
        assert st.behaviour_logp.shape == rows.ys.shape and logp.shape == st.behaviour_logp_sum.shape == (n,)
        rho = behaviour_weights(logp, st.behaviour_logp_sum, clip=5.0)
        assert bool(((rho > 0) & (rho <= 5.0)).all()) and bool(((rho - 1).abs() > 1e-3).any())   # q is not the policy
        opt = FusedAdam(sp.model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9, model=sp.model)
        reward = torch.tensor([float(len(s)) for s in smiles])
        stats = reinforce_step(sp, opt, rows, reward, weight=weight)
        assert ("weight_mean" in stats) == (weight is not None)
        hist = ppo_update(sp, opt, rows, reward, epochs=2, weight=weight)         # and two clipped epochs behind it
        assert all(("weight_max" in h) == (weight is not None) for h in hist)
        done.append((smiles, stats, [q.detach().clone() for q in sp.model.parameters()], hist))
    (s0, st0, p0, h0), (s1, st1, p1, h1) = done
    assert s0 == s1 and all(st1[k] == v for k, v in st0.items()) and st1["weight_mean"] == st1["weight_max"] == 1.0
    assert len(h0) == len(h1) == 2 and all(b[k] == v for a, b in zip(h0, h1) for k, v in a.items())
    assert all(same_bits(a, b) for a, b in zip(p0, p1))                           # bit for bit
    sp = make_sampler(with_stats=True)                                            # stats alone, no rows: (ids, stats)
    ids, st = sp.decode(z, sp.init_y(n, True, sp.smi_to_id("c1ccccc1"), True), torch.ones(n, 1, 26, dtype=torch.bool),
                        torch.full((n, 3), 0.3))
    assert torch.is_tensor(ids) and isinstance(st, StepStats) and not st.behaviour_kl.any()
    assert math.isfinite(float(st.model_entropy.sum()))
