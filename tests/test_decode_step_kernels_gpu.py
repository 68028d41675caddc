"""The four kernels under every decode step, each against a plain fp64 reference of its own operation
(tests/decode_step_ref.py, tests/rng_ref.py; written from include/gctplus_hip.h and held to themselves in
tests/test_decode_step_ref_host.py):
  gct_attn_decode     fixed cache (masks, klen), device position (append, chained steps with gct_decode_advance), ragged
  gct_decode_embed    clamped ids, positions, row offsets
  gct_select_token    greedy (first maximum, probabilities, side effects) and multinomial, plain and filtered: every draw
                      predicted exactly from the Philox stream, except the rows too close to a cumulative boundary
                      (row offsets, streamed rows: parked, inside the prefix, without room for the valid flag)
Every output buffer starts as NaN (a sentinel for integers); whatever a kernel must not touch is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd import ops
from tests import decode_step_ref as D

pytestmark = pytest.mark.gpu
NAN = float("nan")
RTOL = ATOL = 1e-5            # cached attention against fp64: what test_attn_decode_beam_identity_and_random_map holds
T_ROWS = 256                  # cache rows (the kernel's limit)
YS_FILL, VALID_FILL = -7, 9   # sentinels of the integer outputs


def same_bits(a, b):
    """fp32 tensors equal bit for bit (NaN payloads included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close(got, want, what):
    """got (fp32) within RTOL / ATOL of want (fp64); prints the worst error over the tolerance."""
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    ratio = float(((got - want).abs() / (ATOL + RTOL * want.abs())).max())
    print(f"{what}: worst error / tolerance = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


# ================================================================================================ gct_attn_decode
def attn_inputs(dk, n, H, seed, rows=T_ROWS + 2):
    """A fused q | k | v step row wider than 3 d, caches whose key rows are wider than d (kv_row > H dk) with slack rows
    behind the T_ROWS cache rows of every sample."""
    d = H * dk
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * d + 4, generator=g)
    kc, vc = torch.randn(n, rows, d + 8, generator=g), torch.randn(n, rows, d + 8, generator=g)
    return qkv, kc, vc


def heads(t, H, dk):
    """[n, L, >= H dk] cache rows (or [n, >= H dk] step rows) -> fp64 [n, L, H, dk] ([n, H, dk])."""
    return t[..., :H * dk].double().reshape(*t.shape[:-1], H, dk)


def run_attn(qkv, kc, vc, valid, Lc, H, dk, **kw):
    """One launch on device tensors; the output is a strided view into a NaN buffer.  Returns it on the host."""
    n, d = qkv.shape[0], H * dk
    obuf = torch.full((n, d + 4), NAN, device="cuda")
    ops.attn_decode(qkv, qkv.stride(0), kc, vc, kc.stride(1), kc.stride(0), valid, 0 if valid is None else valid.stride(0),
                    obuf[:, :d], n, H, Lc, dk, **kw)
    torch.cuda.synchronize()
    assert bool(obuf[:, d:].isnan().all())                       # nothing behind the d columns of a row
    return obuf[:, :d].cpu()


@pytest.mark.parametrize("dk", [16, 32, 64])
def test_attn_decode_fixed_cache(dk):
    n, H = 3, 2                                                  # n H = 6 pairs: the second workgroup is half empty
    kpp = 64 // (dk // 4)                                        # keys per pass
    scale = 1.0 / math.sqrt(dk)
    qkv, kc, vc = attn_inputs(dk, n, H, seed=dk)
    q = heads(qkv, H, dk)
    qkv_d, kc_d, vc_d = qkv.cuda(), kc.cuda(), vc.cuda()
    g = torch.Generator().manual_seed(7 * dk)
    for Lc in sorted({1, kpp - 1, kpp, kpp + 1, 63, 64, 65, 255, 256}):
        keys, vals = heads(kc[:, :Lc], H, dk), heads(vc[:, :Lc], H, dk)
        got = run_attn(qkv_d, kc_d, vc_d, None, Lc, H, dk)
        close(got.view(n, H, dk), D.cached_attention(q, keys, vals, None, scale), f"dk {dk} Lc {Lc} no mask")
        # sample 0 sees everything, sample 1 has holes, sample 2 sees nothing (uniform weights)
        valid = torch.ones(n, T_ROWS + 8, dtype=torch.uint8)
        valid[1, :Lc] = (torch.rand(Lc, generator=g) < 0.6).to(torch.uint8)
        valid[2] = 0
        got = run_attn(qkv_d, kc_d, vc_d, valid.cuda(), Lc, H, dk)
        close(got.view(n, H, dk), D.cached_attention(q, keys, vals, valid[:, :Lc], scale), f"dk {dk} Lc {Lc} masks")
        mean = vals[2].mean(0)
        assert float((got.view(n, H, dk)[2].double() - mean).abs().max()) <= ATOL + RTOL * float(mean.abs().max())
        # klen: a visible prefix per sample; the rows at and behind klen[b] are NaN and must not be read
        klen = torch.tensor([Lc, 1, max(1, (Lc + 1) // 2)], dtype=torch.int32)
        valid = (torch.arange(T_ROWS + 8)[None, :] < klen[:, None]).to(torch.uint8)
        kn, vn = kc.clone(), vc.clone()
        for b in range(n):
            kn[b, int(klen[b]):], vn[b, int(klen[b]):] = NAN, NAN
        got = run_attn(qkv_d, kn.cuda(), vn.cuda(), valid.cuda(), Lc, H, dk, klen=klen.cuda())
        close(got.view(n, H, dk), D.cached_attention(q, keys, vals, valid[:, :Lc], scale), f"dk {dk} Lc {Lc} klen")
        for b in range(n):                                       # == a call with Lc = klen[b] on that sample alone
            one = run_attn(qkv_d[b:b + 1], kc_d[b:b + 1], vc_d[b:b + 1], None, int(klen[b]), H, dk)
            assert same_bits(got[b], one[0]), (dk, Lc, b)


def test_attn_decode_klen_is_clamped_to_the_cache_length():
    """klen[b] above Lc looks at Lc keys (the header's min(klen[b], Lc)).  All 256 cache rows are allocated and finite,
    so nothing outside the allocation is touched either way; without the clamp sample 0 attends to 48 keys."""
    n, H, dk, Lc = 3, 2, 32, 40
    qkv, kc, vc = attn_inputs(dk, n, H, seed=5)
    klen = torch.tensor([48, 40, 7], dtype=torch.int32)
    valid = torch.ones(n, T_ROWS, dtype=torch.uint8)
    got = run_attn(qkv.cuda(), kc.cuda(), vc.cuda(), valid.cuda(), Lc, H, dk, klen=klen.cuda())
    seen = (torch.arange(Lc)[None, :] < klen.clamp(max=Lc)[:, None]).to(torch.uint8)
    want = D.cached_attention(heads(qkv, H, dk), heads(kc[:, :Lc], H, dk), heads(vc[:, :Lc], H, dk), seen,
                              1.0 / math.sqrt(dk))
    close(got.view(n, H, dk), want, "klen 48 / 40 / 7 at Lc 40")


def step(qkv, kc, vc, valid, pos, cache_off, H, dk, row_off=None):
    """The device-position form: this step's key / value are columns d .. 3 d of the fused row."""
    d = H * dk
    return run_attn(qkv, kc, vc, valid, 0, H, dk, pos=pos, cache_off=cache_off, knew=qkv[:, d:], vnew=qkv[:, 2 * d:],
                    ldn=qkv.stride(0), row_off=row_off)


def cache_with(base, L, new, H, dk):
    """fp64 keys [n, L + 1, H, dk]: the first L cache rows, then this step's row."""
    return torch.cat([heads(base[:, :L], H, dk), heads(new, H, dk)[:, None]], 1)


@pytest.mark.parametrize("cache_off", [0, 3])
@pytest.mark.parametrize("dk", [16, 32, 64])
def test_attn_decode_device_position(dk, cache_off):
    """Lold = cache_off + *pos cached keys (every count of the list that cache_off allows, and *pos = 0), the rows
    behind them NaN: the output is attention over the Lold keys and this step's key, cache row Lold becomes this step's
    key / value bit for bit and nothing else in the caches changes."""
    n, H = 3, 2
    d, scale = H * dk, 1.0 / math.sqrt(dk)
    g = torch.Generator().manual_seed(100 + dk + cache_off)
    for Lold in sorted({cache_off} | {L for L in (0, 1, 63, 64, 254, 255) if L >= cache_off}):
        qkv, kc, vc = attn_inputs(dk, n, H, seed=1000 * dk + Lold, rows=T_ROWS)
        kc[:, Lold:], vc[:, Lold:] = NAN, NAN
        valid = (torch.rand(n, T_ROWS, generator=g) < 0.8).to(torch.uint8)
        valid[0] = 1
        valid[1, Lold], valid[2, Lold] = 0, 1                    # sample 1 masks the step's own key
        kc_d, vc_d, qkv_d = kc.cuda(), vc.cuda(), qkv.cuda()
        pos = torch.tensor([Lold - cache_off], dtype=torch.int32, device="cuda")
        got = step(qkv_d, kc_d, vc_d, valid.cuda(), pos, cache_off, H, dk)
        want = D.cached_attention(heads(qkv, H, dk), cache_with(kc, Lold, qkv[:, d:2 * d], H, dk),
                                  cache_with(vc, Lold, qkv[:, 2 * d:3 * d], H, dk), valid[:, :Lold + 1], scale)
        close(got.view(n, H, dk), want, f"dk {dk} cache_off {cache_off} Lold {Lold}")
        kc[:, Lold, :d], vc[:, Lold, :d] = qkv[:, d:2 * d], qkv[:, 2 * d:3 * d]
        assert same_bits(kc_d.cpu(), kc) and same_bits(vc_d.cpu(), vc), (dk, cache_off, Lold)
        assert int(pos) == Lold - cache_off


def test_attn_decode_chained_steps_with_advance():
    """Three steps on one counter: *pos goes 0, 1, 2, 3 and the caches accumulate one row per step."""
    n, H, dk, cache_off = 3, 2, 32, 3
    d, scale = H * dk, 1.0 / math.sqrt(dk)
    _, kc, vc = attn_inputs(dk, n, H, seed=9, rows=T_ROWS)
    kc[:, cache_off:], vc[:, cache_off:] = NAN, NAN
    valid = torch.ones(n, T_ROWS, dtype=torch.uint8)
    valid[1, 1], valid[2, cache_off + 1] = 0, 0
    kc_d, vc_d, valid_d = kc.cuda(), vc.cuda(), valid.cuda()
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in range(3):
        assert int(pos) == s
        qkv = torch.randn(n, 3 * d + 4, generator=torch.Generator().manual_seed(50 + s))
        got = step(qkv.cuda(), kc_d, vc_d, valid_d, pos, cache_off, H, dk)
        L = cache_off + s
        want = D.cached_attention(heads(qkv, H, dk), cache_with(kc, L, qkv[:, d:2 * d], H, dk),
                                  cache_with(vc, L, qkv[:, 2 * d:3 * d], H, dk), valid[:, :L + 1], scale)
        close(got.view(n, H, dk), want, f"chained step {s}")
        kc[:, L, :d], vc[:, L, :d] = qkv[:, d:2 * d], qkv[:, 2 * d:3 * d]
        assert same_bits(kc_d.cpu(), kc) and same_bits(vc_d.cpu(), vc), s
        ops.check(ops._L().gct_decode_advance(pos.data_ptr(), ops._st()), "gct_decode_advance")
    assert int(pos) == 3


@pytest.mark.parametrize("dk", [16, 32, 64])
def test_attn_decode_ragged_rows_equal_one_row_calls(dk):
    """row_off per row (0 and *pos among them): output and appended cache row of every row equal, bit for bit, a
    one-row call without row_off at that row's own position."""
    n, H, cache_off, P = 5, 2, 3, 70
    row_off = torch.tensor([0, P, 5, 64, 7], dtype=torch.int32)
    qkv, kc, vc = attn_inputs(dk, n, H, seed=3 * dk, rows=T_ROWS)
    for b in range(n):
        L = cache_off + P - int(row_off[b])
        kc[b, L:], vc[b, L:] = NAN, NAN
    valid = (torch.rand(n, T_ROWS, generator=torch.Generator().manual_seed(dk)) < 0.8).to(torch.uint8)
    qkv_d, valid_d = qkv.cuda(), valid.cuda()
    kr, vr = kc.cuda(), vc.cuda()
    got = step(qkv_d, kr, vr, valid_d, torch.tensor([P], dtype=torch.int32, device="cuda"), cache_off, H, dk,
               row_off=row_off.cuda())
    assert bool(torch.isfinite(got).all())
    for b in range(n):
        k1, v1 = kc[b:b + 1].cuda(), vc[b:b + 1].cuda()
        pos = torch.tensor([P - int(row_off[b])], dtype=torch.int32, device="cuda")
        one = step(qkv_d[b:b + 1], k1, v1, valid_d[b:b + 1], pos, cache_off, H, dk)
        assert same_bits(got[b], one[0]), (dk, b)
        assert same_bits(kr[b], k1[0]) and same_bits(vr[b], v1[0]), (dk, b)
        assert not same_bits(k1[0].cpu(), kc[b])                 # the one-row call did append


# ================================================================================================ gct_decode_embed
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("pe_off", [0, 3])
@pytest.mark.parametrize("d,n", [(4, 301), (512, 3)])              # n d / 4 = 301 and 384: a partial last workgroup
def test_decode_embed(d, n, pe_off, ragged):
    vocab, W, p0 = 11, 8, 5
    g = torch.Generator().manual_seed(d + pe_off)
    table, pe = torch.randn(vocab, d, generator=g), torch.randn(16, d, generator=g)
    ys = torch.randint(0, vocab, (n, W), generator=g)
    row_off = (torch.arange(n) % 6).to(torch.int32) if ragged else None
    p = torch.full((n,), p0) - (row_off.long() if ragged else 0)
    ys[0, p[0]], ys[1, p[1]], ys[2, p[2]] = -1, vocab, 1 << 40     # clamped to rows 0, vocab - 1, vocab - 1
    scale = float(np.float32(math.sqrt(d)))                        # the argument is an fp32
    ys_d, table_d, pe_d = ys.cuda(), table.cuda(), pe.cuda()
    out = torch.full((n, d), NAN, device="cuda")
    pos = torch.tensor([p0], dtype=torch.int32, device="cuda")
    ops.decode_embed(ys_d, pos, pe_off, table_d, pe_d, out, scale, row_off=None if row_off is None else row_off.cuda())
    torch.cuda.synchronize()
    want, bound = D.decode_embed(ys, p, table, pe, pe_off, scale)
    err = (out.double().cpu() - want).abs()
    assert bool(torch.isfinite(err).all())
    print(f"decode_embed d {d} pe_off {pe_off} ragged {ragged}: worst error / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(ys_d.cpu(), ys) and same_bits(table_d.cpu(), table) and same_bits(pe_d.cpu(), pe)
    assert int(pos) == p0


# ================================================================================================ gct_select_token
def run_select(x, mode, pos, W, pad, eos, done0=None, valid_sb=16, valid_off=0, probs=True, spare_rows=0, **kw):
    """One launch on fresh sentinel buffers -> (ys, valid, done, probs) on the host; valid_sb = 0 / done0 = None pass
    NULL for valid / done.  spare_rows: rows of valid allocated (and returned) behind the n of the launch."""
    n, V = x.shape
    ys = torch.full((n, W), YS_FILL, dtype=torch.int64, device="cuda")
    valid = torch.full((n + spare_rows, valid_sb), VALID_FILL, dtype=torch.uint8, device="cuda") if valid_sb else None
    done = None if done0 is None else done0.cuda()
    pr = torch.full((n, V), NAN, device="cuda") if probs else None
    ops.select_token(x, ys, pos, valid, done, mode, pad, eos, probs_out=pr, valid_off=valid_off, **kw)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu()              # noqa: E731
    return ys.cpu(), host(valid), host(done), host(pr)


def side_effects(ys, valid, done, cols, pad, eos, done0, valid_off, written=None):
    """The tokens of the written rows (column cols[r] of row r) after checking that ys holds nothing else, that valid
    holds only (token != pad) at valid_off + cols[r] and that done = done0 | (token == eos); rows that are not `written`
    keep every sentinel."""
    n = ys.shape[0]
    rows = torch.arange(n)
    cols = torch.as_tensor(cols).expand(n).long() if not isinstance(cols, torch.Tensor) else cols.long()
    written = torch.ones(n, dtype=torch.bool) if written is None else written
    tok = ys[rows, cols]
    want = torch.full_like(ys, YS_FILL)
    want[rows[written], cols[written]] = tok[written]
    assert torch.equal(ys, want), "ys written outside the step's column"
    assert bool((tok[~written] == YS_FILL).all())
    if valid is not None:
        want = torch.full_like(valid, VALID_FILL)
        want[rows[written], valid_off + cols[written]] = (tok[written] != pad).to(torch.uint8)
        assert torch.equal(valid, want), "valid flags"
    if done is not None:
        want = done0.clone()
        want[written] |= (tok[written] == eos).to(torch.uint8)
        assert torch.equal(done, want), "done flags"
    return tok


def greedy_rows(V):
    """9 logit rows: the exact maximum 5.0 twice, at (5, 70), (63, 64), (67, 3), (0, V - 1) where V has those tokens
    ((0, V - 1) otherwise); -inf on every even token; all logits equal; the maximum on the last token; one finite
    logit; maxima in the middle and at the end.  Every other logit is below 3."""
    g = torch.Generator().manual_seed(V)
    x = torch.randn(9, V, generator=g).clamp(max=3.0)
    for r, (a, b) in enumerate([(5, 70), (63, 64), (67, 3), (0, V - 1)]):
        x[r, [a, b] if max(a, b) < V else [0, V - 1]] = 5.0
    if V >= 2:
        x[4, ::2] = -math.inf
        x[4, [1, V - 1 - V % 2]] = 5.0                  # the first and the last odd token
    x[5] = 0.7
    x[6, V - 1] = 5.0
    x[7] = -math.inf
    x[7, V // 2] = 1.5
    x[8, [V // 2, V - 1]] = 5.0
    top = x.max(-1, keepdim=True).values
    assert bool(((x == top) | (x <= top - 1e-2)).all())          # the fp64 argmax is unambiguous but for the exact ties
    return x


@pytest.mark.parametrize("n", [1, 5, 9])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 130, 4099])
def test_select_token_greedy(V, n):
    x = greedy_rows(V)
    first, p64 = D.greedy(x)
    if V > 70:
        assert first[:4].tolist() == [5, 63, 3, 0]               # the lower index of each stated pair
    x_d, worst = x.cuda(), 0.0
    for lo in (range(9) if n == 1 else [9 - n]):                 # n = 1: every row on its own
        rows = slice(lo, lo + n)
        want = first[rows]
        pad, eos = int(want[0]), int(want[n // 2])               # both occur among the picks
        done0 = (torch.arange(n) % 2).to(torch.uint8)            # done is sticky: a prefilled 1 stays
        ys, valid, done, pr = run_select(x_d[rows].contiguous(), 0, 2, 6, pad, eos, done0=done0, valid_off=3)
        tok = side_effects(ys, valid, done, 2, pad, eos, done0, 3)
        assert torch.equal(tok, want), (V, n, lo, tok.tolist(), want.tolist())
        err = float((pr.double() - p64[rows]).abs().max())
        assert err < 1e-6, (V, n, lo, err)
        worst = max(worst, err)
    print(f"greedy V {V} n {n}: worst probability error / 1e-6 = {worst / 1e-6:.3f}")


def test_select_token_greedy_optional_outputs_and_positions():
    """valid = NULL and done = NULL are accepted; pos_dev with valid_off; row_off."""
    V, n = 130, 9
    x = greedy_rows(V)
    want = D.greedy(x)[0]
    x_d = x.cuda()
    pad, eos = int(want[0]), int(want[1])
    ys, valid, done, pr = run_select(x_d, 0, 4, 6, pad, eos, valid_sb=0, probs=False)
    assert valid is None and done is None and pr is None
    assert torch.equal(side_effects(ys, None, None, 4, pad, eos, None, 0), want)
    done0 = torch.zeros(n, dtype=torch.uint8)
    pos_dev = torch.tensor([2], dtype=torch.int32, device="cuda")                  # the token goes to column 3
    ys, valid, done, _ = run_select(x_d, 0, 0, 6, pad, eos, done0=done0, valid_off=4, pos_dev=pos_dev)
    assert torch.equal(side_effects(ys, valid, done, 3, pad, eos, done0, 4), want)
    row_off = (torch.arange(n) % 5).to(torch.int32)                                # columns 5 - row_off
    pos_dev = torch.tensor([4], dtype=torch.int32, device="cuda")
    ys, valid, done, _ = run_select(x_d, 0, 0, 6, pad, eos, done0=done0, valid_off=2, pos_dev=pos_dev,
                                    row_off=row_off.cuda())
    assert torch.equal(side_effects(ys, valid, done, 5 - row_off.long(), pad, eos, done0, 2), want)
    assert int(pos_dev) == 4


def test_select_token_greedy_stream_rows():
    """Mode 0 over streamed rows: the rows that act write the first maximum at column *pos_dev + 1 - row_off[r] with the
    valid / done side effects; parked rows (item < 0) and rows inside their item's prefix keep every sentinel."""
    V, n = 130, 9
    x = greedy_rows(V)
    want, p64 = D.greedy(x)
    row_off = (torch.arange(n) % 8).to(torch.int32)
    cols = 10 - row_off.long()                                                     # 10, 9, .., 3, 10
    item = torch.randperm(n, generator=torch.Generator().manual_seed(9)).to(torch.int32)
    item[::3] = -1
    prefix_len = (2 + 3 * (torch.arange(n) % 4)).to(torch.int32)                   # per item: 2, 5, 8, 11
    behind = cols >= prefix_len[item.clamp(min=0).long()]
    live = (item >= 0) & behind
    assert 0.2 * n < int(live.sum()) < 0.8 * n and int(((item >= 0) & ~behind).sum()) > 0
    pad, eos = int(want[live][0]), int(want[live][-1])                             # both occur among the picks
    done0 = (torch.arange(n) % 2).to(torch.uint8)
    ys, valid, done, pr = run_select(x.cuda(), 0, 0, 12, pad, eos, done0=done0, valid_off=2,
                                     pos_dev=torch.tensor([9], dtype=torch.int32, device="cuda"), row_off=row_off.cuda(),
                                     item=item.cuda(), prefix_len=prefix_len.cuda(), item_base=1000)
    tok = side_effects(ys, valid, done, cols, pad, eos, done0, 2, written=live)
    assert torch.equal(tok[live], want[live]), (tok.tolist(), want.tolist(), live.tolist())
    assert bool(pr[~live].isnan().all()) and float((pr[live].double() - p64[live]).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ exact draws
PAD, EOS = 0, 2


def filt_dev(name):
    filt = D.CASE[name][3]
    return None if filt is None else ops.sample_filter_settings(*filt, D.CASE[name][1]).cuda()


@pytest.mark.parametrize("name", [c[0] for c in D.DRAW_CASES])
def test_multinomial_draws_are_the_predicted_ones(name):
    """Every row of every case, at each (seed, position) pair of the case: the pick is the reference's wherever the uniform is
    further than delta(V) from a cumulative boundary, one of the two tokens at the boundary elsewhere, never a token of
    weight 0 (the ninf cases have those on both sides of every hit)."""
    V = D.CASE[name][1]
    x, w = D.draw_inputs(name)
    x_d, fd, n = x.cuda(), filt_dev(name), D.DRAW_ROWS
    done0 = torch.zeros(n, dtype=torch.uint8)
    for seed, pos in D.combos(V):
        ys, valid, done, _ = run_select(x_d, 1, pos, 8, PAD, EOS, done0=done0, probs=False, seed=seed, filt_dev=fd)
        tok = side_effects(ys, valid, done, pos, PAD, EOS, done0, 0)
        und = D.check_draws(tok.numpy(), w, seed, np.arange(n), np.full(n, pos), V)
        print(f"{name} seed {seed:#x} pos {pos}: all decidable rows exact, {und} of {n} rows undecidable")


@pytest.mark.parametrize("name", ["plain-65", "filt-65", "filt-30"])
def test_multinomial_seed_from_device_memory(name):
    """seed_dev gives the picks of the same seed passed by value (and overrides the by-value one); the other two
    (seed, position) pairs than the diagonal."""
    V = D.CASE[name][1]
    x, w = D.draw_inputs(name)
    x_d, fd, n = x.cuda(), filt_dev(name), D.DRAW_ROWS
    for seed, pos in zip(D.SEEDS, reversed(D.POSITIONS)):
        by_value = run_select(x_d, 1, pos, 8, PAD, EOS, probs=False, seed=seed, filt_dev=fd)[0]
        by_dev = run_select(x_d, 1, pos, 8, PAD, EOS, probs=False, seed=999, filt_dev=fd,
                            seed_dev=D.seed_tensor(seed).cuda())[0]
        assert torch.equal(by_value, by_dev), (name, hex(seed))
        D.check_draws(by_dev[:, pos].numpy(), w, seed, np.arange(n), np.full(n, pos), V)


@pytest.mark.parametrize("name", ["plain-65", "filt-65", "filt-30"])
def test_multinomial_row_offsets_key_each_row_by_its_own_position(name):
    V = D.CASE[name][1]
    x, w = D.draw_inputs(name)
    n = D.DRAW_ROWS
    row_off = (torch.arange(n) % 8).to(torch.int32)
    cols = 10 - row_off.long()                                                     # *pos_dev + 1 - row_off
    done0 = torch.zeros(n, dtype=torch.uint8)
    ys, valid, done, _ = run_select(x.cuda(), 1, 0, 12, PAD, EOS, done0=done0, valid_off=2, probs=False, seed=D.SEEDS[1],
                                    pos_dev=torch.tensor([9], dtype=torch.int32, device="cuda"), row_off=row_off.cuda(),
                                    filt_dev=filt_dev(name))
    tok = side_effects(ys, valid, done, cols, PAD, EOS, done0, 2)
    D.check_draws(tok.numpy(), w, D.SEEDS[1], np.arange(n), cols.numpy(), V)


@pytest.mark.parametrize("item_base", [0, 1000])
@pytest.mark.parametrize("name", ["plain-65", "filt-65", "filt-30"])
def test_multinomial_stream_rows_are_keyed_by_their_item(name, item_base):
    """Continuous batching: the key is (item_base + item, pos); parked rows (item < 0) and rows inside their prefix
    (pos < prefix_len[item]) write nothing at all."""
    V = D.CASE[name][1]
    x, w = D.draw_inputs(name)
    n = D.DRAW_ROWS
    g = torch.Generator().manual_seed(4)
    item = torch.randperm(n, generator=g).to(torch.int32)
    item[::5] = -1
    prefix_len = (1 + torch.arange(n) % 12).to(torch.int32)                        # per item
    row_off = (torch.arange(n) % 8).to(torch.int32)
    cols = 10 - row_off.long()                                                     # 3 .. 10
    live = (item >= 0) & (cols >= prefix_len[item.clamp(min=0).long()])
    assert 0.2 * n < int(live.sum()) < 0.8 * n and int((item < 0).sum()) > 0
    done0 = (torch.arange(n) % 3 == 0).to(torch.uint8)
    ys, valid, done, _ = run_select(x.cuda(), 1, 0, 12, PAD, EOS, done0=done0, valid_off=2, probs=False, seed=D.SEEDS[0],
                                    pos_dev=torch.tensor([9], dtype=torch.int32, device="cuda"), row_off=row_off.cuda(),
                                    filt_dev=filt_dev(name), item=item.cuda(), prefix_len=prefix_len.cuda(),
                                    item_base=item_base)
    tok = side_effects(ys, valid, done, cols, PAD, EOS, done0, 2, written=live)
    keys = (item_base + item.long())[live].numpy()
    D.check_draws(tok[live].numpy(), w[live.numpy()], D.SEEDS[0], keys, cols[live].numpy(), V)


@pytest.mark.parametrize("name", ["plain-65", "filt-30"])
def test_multinomial_stream_rows_without_room_write_nothing(name):
    """A streamed row whose flag slot valid_off + pos lies at or behind valid_sb writes nothing -- ys (wide enough to
    hold the column), valid, done -- and the rows with room draw as ever.  A write past the row's flags would land in
    the next row of valid: the over-long rows are not the last one, and a spare row lies behind the n of the launch."""
    V = D.CASE[name][1]
    x, w = D.draw_inputs(name)
    n, valid_sb, valid_off = D.DRAW_ROWS, 9, 2
    item = torch.randperm(n, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    prefix_len = torch.ones(n, dtype=torch.int32)
    row_off = (torch.arange(n) % 8).to(torch.int32)
    row_off[-1] = 7                                                                # the last row has room
    cols = 10 - row_off.long()                                                     # 3 .. 10; flag slots 5 .. 12
    live = valid_off + cols < valid_sb
    assert 0.2 * n < int(live.sum()) < 0.8 * n and bool(live[-1]) and int((valid_off + cols).max()) < 2 * valid_sb
    done0 = (torch.arange(n) % 3 == 0).to(torch.uint8)
    ys, valid, done, _ = run_select(x.cuda(), 1, 0, 12, PAD, EOS, done0=done0, valid_sb=valid_sb, valid_off=valid_off,
                                    probs=False, spare_rows=1, seed=D.SEEDS[0],
                                    pos_dev=torch.tensor([9], dtype=torch.int32, device="cuda"), row_off=row_off.cuda(),
                                    filt_dev=filt_dev(name), item=item.cuda(), prefix_len=prefix_len.cuda())
    tok = side_effects(ys, valid, done, cols, PAD, EOS, done0, valid_off, written=live)
    D.check_draws(tok[live].numpy(), w[live.numpy()], D.SEEDS[0], item.long()[live].numpy(), cols[live].numpy(), V)
