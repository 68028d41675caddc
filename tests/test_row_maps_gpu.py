"""csrc/liverows.hip against the host reference (tests/rowmap_ref.py): the maps of gct_live_rows / gct_key_rows, the
quad gather / scatter / scatter-add, gct_zero_gap_rows, gct_dead_rows_nonzero and the device guard of gct_adam_step.
Every comparison is integer or bit equality; every input is tiny."""
import pytest
import torch

from tests.rowmap_ref import (causal_pad_mask, compact_rows, gap_rows, prefix_live, random_plans,
                              row_plan_reference)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.25                  # finite sentinel of the destination buffers


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def _lens(B, T, salt=3):
    """Deterministic prefix lengths with 0 and T among them."""
    return [(0, T, (7 * b + salt) % (T + 1), 1)[(b + salt) % 4] for b in range(B)]


def _dev(t):
    return None if t is None else t.to(DEV)


def _live_rows(ops, live, mask):
    B, T = live.shape
    L = ops.LiveRows.from_rows(live.to(torch.uint8).to(DEV), B, T, _dev(mask))
    L.host()
    return L


def _check(L, ref, what, tiles=True):
    B, M, padded = ref["B"], ref["M"], ref["Mc"] // 4
    assert L.info.cpu().tolist() == ref["info"], f"{what}: info {L.info.cpu().tolist()} != {ref['info']}"
    assert L.Mc == ref["Mc"]
    assert torch.equal(L.live[:M].cpu().bool(), ref["live"].reshape(-1)), f"{what}: live"
    assert L.n_b[:B].cpu().tolist() == ref["n_b"].tolist(), f"{what}: n_b"
    assert L.cstart[:B].cpu().tolist() == ref["cstart"].tolist(), \
        f"{what}: cstart {L.cstart[:B].cpu().tolist()} != {ref['cstart'].tolist()} (n_b {ref['n_b'].tolist()})"
    assert L.quad_list[:padded].cpu().tolist() == ref["quad_list"].tolist(), f"{what}: quad_list"
    if tiles:
        n = int(L.tile_count.item())
        assert n == ref["info"][3]
        assert L.tile_list[:n].cpu().tolist() == ref["tile_list"].tolist(), f"{what}: tile_list"


# ------------------------------------------------------------------------------------------ gct_live_rows
def test_live_rows_random_plans(ops):
    for name, live, mask in random_plans():
        _check(_live_rows(ops, live, mask), row_plan_reference(live, mask), name)


def _hand_plans():
    out = []
    for B, T in [(1, 1), (3, 5), (2, 7), (3, 6), (5, 33), (4, 64), (2, 81)]:
        for salt in (1, 2, 3):
            n = _lens(B, T, salt)
            out.append((f"B{B}T{T}n{n}", prefix_live(B, T, n), causal_pad_mask(B, T, n)))
    out.append(("issue example", prefix_live(3, 6, (0, 0, 2)), causal_pad_mask(3, 6, (0, 0, 2))))
    out.append(("32 live quads", prefix_live(1, 128, (128,)), None))                 # no -1 padding
    out.append(("33 live quads", prefix_live(1, 132, (132,)), None))                 # a full extra block of padding
    out.append(("32 live quads, shared", prefix_live(2, 66, (66, 59)), causal_pad_mask(2, 66, (66, 59))))
    out.append(("all dead", prefix_live(3, 10, (0, 0, 0)), causal_pad_mask(3, 10, (0, 0, 0))))
    out.append(("all live", prefix_live(3, 10, (10, 10, 10)), None))
    out.append(("tail of 28 rows", prefix_live(1, 100, (100,)), None))
    out.append(("empty tail", prefix_live(1, 128, (128,)), causal_pad_mask(1, 128, (128,))))
    return out


def test_live_rows_hand_plans(ops):
    for name, live, mask in _hand_plans():
        ref = row_plan_reference(live, mask)
        _check(_live_rows(ops, live, mask), ref, name)
    ref = row_plan_reference(prefix_live(1, 128, (128,)))
    assert ref["info"][5] == 32 and ref["Mc"] == 128 and (ref["quad_list"] >= 0).all()
    assert row_plan_reference(prefix_live(2, 66, (66, 59)))["info"][5] == 32
    ref = row_plan_reference(prefix_live(1, 132, (132,)))
    assert ref["info"][5] == 33 and ref["Mc"] == 256
    ref = row_plan_reference(prefix_live(3, 10, (0, 0, 0)))
    assert ref["Mc"] == 0 and ref["info"][4] == ref["info"][5] == 0


def test_live_rows_second_pass_of_the_quad_scan(ops):
    """(B, T) = (70, 61): 1068 quads, the single-workgroup scan of 1024 runs a second pass; live quads on both sides."""
    B, T = 70, 61
    n = _lens(B, T, 2)
    live, mask = prefix_live(B, T, n), prefix_live(B, T, n).to(torch.uint8)
    ref = row_plan_reference(live, mask)
    assert (B * T + 3) // 4 == 1068
    ql = ref["quad_list"][:ref["info"][5]]
    assert (ql < 1024).any() and (ql >= 1024).any()
    _check(_live_rows(ops, live, mask), ref, "70 x 61")


def test_live_rows_second_pass_of_the_tile_scan(ops):
    """(B, T) = (330, 100), 4 gradient columns: 1032 tiles of 32 rows, the tile-list scan runs a second pass."""
    B, T = 330, 100
    n = _lens(B, T, 1)
    live, mask = prefix_live(B, T, n), prefix_live(B, T, n).to(torch.uint8)
    ref = row_plan_reference(live, mask)
    assert (B * T + 31) // 32 == 1032 and (ref["tile_list"] >= 1024).any() and (ref["tile_list"] < 1024).any()
    g = torch.zeros(B * T, 4)
    g[live.reshape(-1), 2] = -3.0
    L = ops.LiveRows(g.to(DEV), B, T, mask.to(DEV))
    L.host()
    _check(L, ref, "330 x 100")


@pytest.mark.parametrize("layout", ["c512", "c30", "c1", "strided"])
def test_live_rows_gradient_layouts(ops, layout):
    """live = the row holds a non-zero element: -0.0 is zero, NaN is not; the last column counts; a strided view and
    the scalar flag path (cols % 4 != 0, the vocabulary head's shape) read their own columns only."""
    B, T = 3, 7
    n = (7, 3, 0)
    cols = {"c512": 512, "c30": 30, "c1": 1, "strided": 64}[layout]
    live = prefix_live(B, T, n)
    g = torch.zeros(B * T, cols)
    gen = torch.Generator().manual_seed(5)
    g[live.reshape(-1)] = torch.randn(int(live.sum()), cols, generator=gen)
    g[1] = 0.0
    g[1, cols - 1] = 1e-30                           # live through its last column alone
    g[2] = 0.0
    g[2, 0] = float("nan")                           # NaN != 0: live
    g[T + 3] = -0.0                                  # a dead row of negative zeros stays dead
    g[T + 4] = 0.0
    if layout == "strided":
        wide = torch.full((B * T, 192), 5.0)         # non-zero everywhere outside the view: must not be read
        wide[:, 64:128] = g
        gd = wide.to(DEV)[:, 64:128]
        assert gd.stride(0) == 192
    else:
        gd = g.to(DEV)
    mask = causal_pad_mask(B, T, n)
    L = ops.LiveRows(gd, B, T, mask.to(DEV))
    L.host()
    _check(L, row_plan_reference(live, mask), layout)


def test_live_rows_masks(ops):
    B, T = 4, 9
    n = (9, 4, 0, 6)
    live = prefix_live(B, T, n)
    cases = [("none, mixed", live, None),
             ("none, all or nothing", prefix_live(B, T, (9, 0, 9, 0)), None),
             ("key padding", live, prefix_live(B, T, n).to(torch.uint8)),
             ("key padding, one key too many", live, prefix_live(B, T, (9, 5, 0, 6)).to(torch.uint8))]
    # causal-and-padding mask from the token ids (pad = 1: the reference's `* pad_idx` keeps the mask)
    tok = torch.where(live, torch.full((B, T), 5), torch.full((B, T), 1))
    dm = ops.trg_mask_u8(tok.to(DEV), 1)
    assert torch.equal(dm.cpu(), causal_pad_mask(B, T, n))
    cases.append(("trg_mask_u8", live, dm.cpu()))
    # left-padded: the live rows are a suffix (non-prefix), visible keys = live keys up to the query
    left = torch.arange(T)[None, :] >= (T - torch.tensor(n))[:, None]
    lm = (left[:, None, :] & torch.tril(torch.ones(T, T, dtype=torch.bool))[None]).to(torch.uint8)
    cases.append(("left padded", left, lm))
    blind = causal_pad_mask(B, T, n)
    blind[1, 2, :] = 0                                # live row (1, 2) sees no key; sample 1 has dead rows
    cases.append(("a live row without a key", live, blind))
    blind_full = causal_pad_mask(B, T, n)
    blind_full[0, 2, :] = 0                           # ... in a sample without dead rows: no violation
    cases.append(("a live row without a key, no dead row", live, blind_full))
    want = {"none, mixed": (2, 0), "none, all or nothing": (0, 0), "key padding": (0, 0),
            "key padding, one key too many": (1, 0), "trg_mask_u8": (0, 0), "left padded": (0, 2),
            "a live row without a key": (1, 0), "a live row without a key, no dead row": (0, 0)}
    for name, lv, mask in cases:
        ref = row_plan_reference(lv, mask)
        assert tuple(ref["info"][1:3]) == want[name], (name, ref["info"])
        _check(_live_rows(ops, lv, mask), ref, name)


# ------------------------------------------------------------------------------------------- gct_key_rows
def test_key_rows(ops):
    gen = torch.Generator().manual_seed(9)
    cases = []
    for B, Lk in [(1, 1), (3, 5), (2, 7), (5, 33), (4, 64), (2, 81), (3, 100), (70, 61)]:
        n = [max(1, x) for x in _lens(B, Lk, 2)]
        cases.append((f"prefix {B}x{Lk}", prefix_live(B, Lk, n)))
        cases.append((f"holes {B}x{Lk}", torch.rand(B, Lk, generator=gen) < 0.6))
        cases.append((f"a sample without a key {B}x{Lk}", prefix_live(B, Lk, _lens(B, Lk, 0))))
    for name, vis in cases:
        B, Lk = vis.shape
        ref = row_plan_reference(vis, key_side=True)
        K = ops.KeyRows(vis.to(torch.uint8).to(DEV), B, Lk)
        K.host()
        _check(K, ref, name, tiles=False)
    assert row_plan_reference(prefix_live(3, 5, _lens(3, 5, 0)), key_side=True)["info"][6] > 0


# ------------------------------------------------------------------------- gather / scatter / scatter_add
def _move_plans():
    plans = [p for p in random_plans()[:18]]
    plans += [("M % 4 != 0, last quad live", prefix_live(3, 7, (2, 0, 7)), None),
              ("M % 4 != 0, shared quads", prefix_live(5, 33, (33, 1, 0, 17, 33)), None),
              ("no padding quads", prefix_live(1, 128, (128,)), None)]
    return plans


@pytest.mark.parametrize("cols,ld", [(4, 4), (64, 64), (512, 512), (30, 30), (64, 96), (30, 33)])
def test_gather_scatter(ops, cols, ld):
    """gather: compact row i = source row orig[i], zeros for the -1 quads and for rows >= M, nothing behind row Mc;
    scatter: row orig[i] = compact row i, every other row and the guard rows behind M keep the sentinel."""
    gen = torch.Generator().manual_seed(cols)
    for name, live, mask in _move_plans():
        B, T = live.shape
        M = B * T
        ref = row_plan_reference(live, mask)
        if ref["Mc"] == 0:
            continue
        L = _live_rows(ops, live, mask)
        orig, _ = compact_rows(ref)
        ok = orig >= 0
        if name == "M % 4 != 0, last quad live":      # the last quad reaches past M: its rows >= M are padding
            assert (~ok[:4 * ref["info"][5]]).any()
        src = torch.randn(M, ld, generator=gen)
        srcd = src.to(DEV)[:, :cols]
        exp = torch.zeros(L.Mc, cols)
        exp[ok] = src[orig[ok], :cols]
        out = torch.full((L.Mc + 4, ld), SENT, device=DEV)
        got = L.gather(srcd, out=out[:L.Mc, :cols])
        assert torch.equal(got.cpu(), exp), f"gather {name}"
        assert (out[L.Mc:] == SENT).all() and (out[:, cols:] == SENT).all(), f"gather wrote outside {name}"
        # scatter the compact rows (fresh values in EVERY compact row, padding included) back into a guarded buffer
        comp = torch.randn(L.Mc, ld, generator=gen)
        dst = torch.full((M + 8, ld), SENT, device=DEV)
        L.scatter(comp.to(DEV)[:, :cols], out=dst[:M, :cols])
        exp = torch.full((M + 8, ld), SENT)
        exp[orig[ok], :cols] = comp[ok, :cols]
        assert torch.equal(dst.cpu(), exp), f"scatter {name}"


@pytest.mark.parametrize("cols,ld", [(4, 4), (64, 64), (512, 512), (64, 96)])
def test_scatter_add(ops, cols, ld):
    """dst row orig[i] += compact row i: one fp32 add per element, so bit equality with the host's add."""
    gen = torch.Generator().manual_seed(100 + cols)
    for name, live, mask in _move_plans():
        B, T = live.shape
        M = B * T
        ref = row_plan_reference(live, mask)
        if ref["Mc"] == 0:
            continue
        L = _live_rows(ops, live, mask)
        orig, _ = compact_rows(ref)
        ok = orig >= 0
        comp = torch.randn(L.Mc, ld, generator=gen)
        base = torch.randn(M + 8, ld, generator=gen)
        base[M:] = SENT
        untouched = torch.ones(M + 8, dtype=torch.bool)
        untouched[orig[ok]] = False
        base[untouched] = SENT
        dst = base.to(DEV)
        L.scatter_add(comp.to(DEV)[:, :cols], dst[:M, :cols])
        exp = base.clone()
        exp[orig[ok], :cols] = base[orig[ok], :cols] + comp[ok, :cols]
        assert torch.equal(dst.cpu(), exp), f"scatter_add {name}"


# -------------------------------------------------------------------------------------- gct_zero_gap_rows
def _usable_plans():
    out = []
    for name, live, mask in random_plans() + _hand_plans():
        ref = row_plan_reference(live, mask)
        if ref["usable"]:
            out.append((name, live, mask, ref))
    return out


def test_zero_gap_rows(ops):
    """Through the C ABI on a sentinel-filled buffer of Mc + SLACK rows, once with nrows = Mc and once with
    nrows = Mc + SLACK: every row of [0, nrows) outside the live prefixes is zero, every live-prefix row and every row
    >= nrows keeps the sentinel.  Every usable plan, samples without a live row included -- (T, B) = (6, 3) with
    lengths (0, 0, 2) zeroed the two live rows of sample 2 while cstart carried the offset of row 0 inside its quad
    for samples whose first quad is dead."""
    from gct_plus_amd import _lib
    lib = _lib.load()
    SLACK = ops.LiveRows.SLACK
    plans = _usable_plans()
    assert len(plans) >= 40 and any((r["n_b"] == 0).any() and r["Mc"] for *_, r in plans)
    tails = set()
    bad = []
    for name, live, mask, ref in plans:
        B = ref["B"]
        L = _live_rows(ops, live, mask)
        _, prefix = compact_rows(ref)
        for nrows, cols, ld in [(L.Mc, 8, 8), (L.Mc + SLACK, 8, 8), (L.Mc + SLACK, 64, 96)]:
            tails.add((B, nrows - int(ref["cstart"][-1] + ref["n_b"][-1])))
            buf = torch.full((L.Mc + SLACK, ld), SENT, device=DEV)
            _lib.check(lib.gct_zero_gap_rows(buf.data_ptr(), ld, cols, L.cstart.data_ptr(), L.n_b.data_ptr(), B, nrows,
                                             torch.cuda.current_stream().cuda_stream), "gct_zero_gap_rows")
            got = buf.cpu()
            zero = torch.zeros(L.Mc + SLACK, dtype=torch.bool)
            zero[:nrows] = gap_rows(ref, nrows)
            exp = torch.full((L.Mc + SLACK, ld), SENT)
            exp[zero, :cols] = 0.0
            if not torch.equal(got, exp):
                rows = torch.nonzero((got != exp).any(1)).flatten().tolist()
                bad.append((name, ref["n_b"].tolist(), L.cstart[:B].cpu().tolist(), nrows, rows[:8]))
    assert not bad, f"{len(bad)} calls left a wrong row; (plan, n_b, cstart, nrows, rows): {bad[:4]}"
    lens = {t for _, t in tails}
    assert any(b == 1 for b, _ in tails)
    assert any(0 < t < 49 for t in lens) and any(t > 49 and t % 49 for t in lens) and 0 in lens


# ------------------------------------------------------------- gct_dead_rows_nonzero and the Adam guard
def test_dead_rows_nonzero_counts_exactly(ops):
    B, T, cols, ld = 4, 9, 30, 40
    live = prefix_live(B, T, (9, 4, 0, 6))
    L = _live_rows(ops, live, causal_pad_mask(B, T, (9, 4, 0, 6)))
    g = torch.zeros(B * T, ld)
    g[:, cols:] = 1.0                                 # behind the view: never read
    g[live.reshape(-1), :cols] = 1.0                  # live rows may hold anything
    dead = torch.nonzero(~live.reshape(-1)).flatten()
    hit = dead[[0, 3, 7, len(dead) - 1]]
    g[hit[0], 0] = 1.0
    g[hit[1], cols - 1] = -2.0                        # the last column alone
    g[hit[2], 7] = float("nan")
    g[hit[3], :cols] = 3.0
    g[dead[1], :cols] = -0.0                          # negative zeros are zeros
    counter = ops.skipped_row_gradients()
    try:
        before = int(counter.item())
        L.check_grad(g.to(DEV)[:, :cols])
        assert int(counter.item()) - before == 4
        L.check_grad(torch.zeros(B * T, cols, device=DEV))
        assert int(counter.item()) - before == 4
    finally:
        counter.zero_()


def test_adam_guard(ops):
    """guard=True: with the skipped-row counter non-zero p, m and v stay as they are, bit for bit; with it zero the
    step is torch.optim.Adam's (the bounds of test_adam_matches_torch)."""
    from tests.test_kernels_gpu import close, rnd
    n = 10007
    p0, g = rnd(n, seed=1), rnd(n, seed=2)
    counter = ops.skipped_row_gradients()
    try:
        counter.zero_()
        ref = p0.clone().requires_grad_()
        opt = torch.optim.Adam([ref], lr=1e-4, betas=(0.9, 0.98), eps=1e-9)
        pg, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        for step in range(1, 4):
            gi = g * (1 + 0.1 * step)
            ref.grad = gi.clone()
            opt.step()
            ops.adam_step(pg, gi.to(DEV), m, v, 1e-4, 0.9, 0.98, 1e-9, step, guard=True)
        close(pg, ref, 1e-7, 1e-6, "adam params")
        close(m, opt.state[ref]["exp_avg"], 1e-7, 1e-5)
        close(v, opt.state[ref]["exp_avg_sq"], 1e-9, 1e-5)
        keep = [t.clone() for t in (pg, m, v)]
        counter.fill_(2)
        ops.adam_step(pg, g.to(DEV), m, v, 1e-4, 0.9, 0.98, 1e-9, 4, guard=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(keep, (pg, m, v))), "a guarded step changed p / m / v"
        ops.adam_step(pg, g.to(DEV), m, v, 1e-4, 0.9, 0.98, 1e-9, 4, guard=False)
        assert not torch.equal(keep[0], pg)           # the same call without the guard does step
    finally:
        counter.zero_()
