"""tests/kv_fold_ref.py held to independent restatements (fp32 on the CPU, summed in the opposite order), the case tables
of tests/test_kv_fold_edges_gpu.py shown to reach every branch of the kv_fold kernels and to tell each likely kernel
mistake apart on a named case, the fold's algebra (folded = unfolded formulas in fp64) and the truth table of
ops.KvFold.usable.  No GPU."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests import gemm_ref as G
from tests import kv_fold_ref as R

F32_ROUTE = (G.F32_FAST, 1, 0, 0, 1, 1, 0, 0)                  # an fp32 route without slabs
X6_ROUTE = (G.X6S, 1, 0, 0, 1, 1, 0, 0)                        # a bf16 route without slabs


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_fwd_reference_against_fp32_in_the_opposite_order(c, bias):
    inp = R.inputs(c)
    ref = R.reference_fwd(inp, bias)
    rows = 2 * c.layers * c.d
    assert ref.wstack.shape == (rows, c.dm) and ref.wstack.dtype == torch.float32
    for i, w in enumerate(inp.w):                              # the stack, row by row
        for r in (0, c.d - 1):
            assert torch.equal(ref.wstack[i * c.d + r], w[r])
    assert ref.c.dtype == ref.a.dtype == torch.float64 and ref.c.shape == (rows,) and ref.a.shape == (rows, c.lat)
    w32 = ref.wstack
    got_c = w32.flip(1) @ inp.bz.flip(0)
    if bias:
        got_c = got_c + torch.cat(inp.b)
    assert R.ratio(got_c, ref.c, R.bound_c(ref, c)) <= 1.0
    got_a = w32.flip(1) @ inp.wz.flip(0)
    assert R.ratio(got_a, ref.a, R.bound_a(ref, R.F32, F32_ROUTE)) <= 1.0
    # the bound formulas, spelled out once
    Sc = w32.double().abs() @ inp.bz.double().abs() + (torch.cat(inp.b).double().abs() if bias else 0)
    assert torch.equal(R.bound_c(ref, c), (c.dm + 1) * 2.0 ** -24 * 1.01 * Sc)
    Sa = w32.double().abs() @ inp.wz.double().abs()
    assert torch.equal(ref.gemm.S, Sa) and ref.gemm.terms == c.dm
    for mode, route, drop in ((R.F32, F32_ROUTE, 0.0), (R.BF16X6, X6_ROUTE, 2.0 ** -23), (R.BF16X3, X6_ROUTE, 3.02 * 2.0 ** -16),
                              (R.BF16X6, F32_ROUTE, 0.0)):      # an fp32 route drops nothing, whatever the mode
        assert torch.equal(R.bound_a(ref, mode, route), (drop + c.dm * 2.0 ** -24 * 1.01) * Sa + ref.gemm.floor)
    # two bf16 pieces per operand (bf16x3 arithmetic, exact accumulation) stay inside the bf16x3 bound
    from tests.wgrad_ref import _pieces2
    wh, wm = _pieces2(w32)
    zh, zm = _pieces2(inp.wz)
    assert R.ratio(wh @ zh + wh @ zm + wm @ zh, ref.a, R.bound_a(ref, R.BF16X3, X6_ROUTE)) <= 1.0


@pytest.mark.parametrize("c", R.WGRAD_CASES, ids=R.case_id)
def test_wgrad_reference_against_fp32_in_the_opposite_order(c):
    inp = R.inputs(c)
    ref = R.reference_wgrad(inp)
    assert ref.dw.shape == ref.S.shape == (2 * c.d, c.dm) and ref.dw.dtype == torch.float64
    got = inp.p.flip(1) @ inp.wz.flip(1).t() + inp.s[:, None] * inp.bz[None, :]
    assert R.ratio(got, ref.dw, R.bound_w(ref, c)) <= 1.0
    S = inp.p.double().abs() @ inp.wz.double().abs().t() + inp.s.double().abs()[:, None] * inp.bz.double().abs()[None, :]
    assert torch.equal(R.bound_w(ref, c), (c.lat + 1) * 2.0 ** -24 * 1.01 * S)
    assert torch.equal(ref.db, inp.s)
    m, n = 2 * c.d - 1, c.dm - 1                               # one element by hand
    want = sum(float(inp.p[m, k]) * float(inp.wz[n, k]) for k in range(c.lat)) + float(inp.s[m]) * float(inp.bz[n])
    assert abs(float(ref.dw[m, n]) - want) <= 1e-13 * float(ref.S[m, n])


@pytest.mark.parametrize("c", R.DBZ_CASES, ids=R.case_id)
def test_dbz_reference_against_fp32_in_the_opposite_order(c):
    inp = R.inputs(c)
    ref = R.reference_dbz(inp)
    assert ref.dbz.shape == (c.dm,) and ref.dbz.dtype == torch.float64
    got = inp.wstack.flip(0).t() @ inp.s.flip(0)
    assert R.ratio(got, ref.dbz, R.bound_dbz(ref, c)) <= 1.0
    assert torch.equal(R.bound_dbz(ref, c), c.rows * 2.0 ** -24 * 1.01 * (inp.wstack.double().abs().t() @ inp.s.double().abs()))
    want = sum(float(inp.wstack[r, c.dm - 1]) * float(inp.s[r]) for r in range(c.rows))
    assert abs(float(ref.dbz[-1]) - want) <= 1e-13 * float(ref.S[-1])


def test_planes_sum_is_the_exact_inverse_of_a_three_piece_split():
    x = R.rnd(64, seed=3)
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = (x - hi - mid).bfloat16().float()
    assert torch.equal(hi + mid + lo, x)
    planes = torch.stack([(t.view(torch.int32) >> 16).to(torch.int16) for t in (hi, mid, lo)])
    wide = torch.cat([planes, torch.full((3, 8), 0x5A5A, dtype=torch.int16)], 1)
    assert torch.equal(R.planes_sum(wide, 64), x)


# ------------------------------------------------------------------------------------------------ the tables reach every branch
def test_the_tables_cover_every_branch_of_the_kernels():
    ids = [R.case_id(c) for c in R.FWD_CASES + R.WGRAD_CASES + R.DBZ_CASES]
    assert len(ids) == len(set(ids))
    T, K, ROWS = R.KVF_T, R.KVF_K, R.KVF_ROWS
    wg, fw, dz = R.WGRAD_CASES, R.FWD_CASES, R.DBZ_CASES
    # wgrad, K chunks: one chunk; several full chunks (the prefetch alone); a ragged last chunk behind a full one
    assert any(c.lat <= K for c in wg) and any(c.lat > K and c.lat % K == 0 for c in wg)
    assert any(c.lat > K and c.lat % K != 0 for c in wg) and any(c.lat > 2 * K and c.lat % K != 0 for c in wg)
    # wgrad, tile edges: ragged row and column tiles, more than one tile each way, the k | v boundary inside a tile and
    # inside one thread's four rows
    assert any(2 * c.d % T != 0 for c in wg) and any(c.dm % T != 0 for c in wg)
    assert any(2 * c.d > T for c in wg) and any(c.dm > T for c in wg)
    assert any(2 * c.d % T == 0 and c.dm % T == 0 for c in wg)
    assert any(c.d % T != 0 for c in wg) and any(c.d % 4 != 0 for c in wg)
    assert any(2 * c.d % 4 != 0 for c in wg)                   # the last row inside one thread's four
    assert any(c.d < 4 for c in wg)                            # dw0 and dw1 rows in the first thread's four
    # stack: d != dm both ways round is not needed, one way is; copy loop passes 1, 2 and 3, ragged last passes; the
    # smallest call; the table's limit
    assert any(c.d != c.dm for c in fw) and any(c.d == c.dm for c in fw)
    assert any(c.dm > 256 and c.dm % 256 != 0 for c in fw) and any(c.dm > 512 for c in fw) and any(c.dm < 256 for c in fw)
    assert any(c.layers == R.MAX_LAYERS for c in fw) and any(c.layers == 1 for c in fw)
    assert any(c.lat % 32 != 0 and c.lat > 32 for c in fw)
    assert all(c.d % 4 == 0 and c.dm % 4 == 0 and c.lat % 4 == 0 for c in fw)         # what gct_kv_fold_fwd accepts
    assert all(c.dm % 4 == 0 and c.lat % 4 == 0 for c in wg)                          # what gct_kv_fold_wgrad accepts
    # dbz: a ragged last part, fewer than 8 parts, a part count above 8 that is no multiple of 8, one that is, more than
    # one column block, a width that is no multiple of the sum kernel's 32 columns
    parts = [R.dbz_parts(c) for c in dz]
    assert any(c.rows % ROWS != 0 for c in dz) and any(c.rows % ROWS == 0 for c in dz)
    assert any(p < 8 for p in parts) and any(p > 8 and p % 8 != 0 for p in parts) and any(p > 8 and p % 8 == 0 for p in parts)
    assert any(p == 1 for p in parts)
    assert any(c.dm > 256 for c in dz) and any(c.dm % 32 != 0 for c in dz) and any(c.dm > 256 and c.dm % 256 != 0 for c in dz)


# ------------------------------------------------------------------------------------------------ the cases discriminate
def _fwd_c(wrong_of):
    def run(c):
        inp = R.inputs(c)
        ref = R.reference_fwd(inp)
        return R.ratio(wrong_of(inp, ref), ref.c, R.bound_c(ref, c))
    return run


def _stride_d(inp, ref):
    w = R.mistake_stack_row_stride_d(inp)
    assert torch.equal(w, ref.wstack) == (inp.c.d == inp.c.dm)
    return R.reference_fwd(inp, w=w).c


def _one_off(inp, ref):
    w, b = R.mistake_segment_one_off(inp)
    return w.double() @ inp.bz.double() + b.double()


def _wgrad(wrong_of):
    def run(c):
        inp = R.inputs(c)
        ref = R.reference_wgrad(inp)
        return R.ratio(wrong_of(inp, ref), ref.dw, R.bound_w(ref, c))
    return run


def _dbz(wrong_of):
    def run(c):
        inp = R.inputs(c)
        ref = R.reference_dbz(inp)
        return R.ratio(wrong_of(inp, ref), ref.dbz, R.bound_dbz(ref, c))
    return run


FW, WG, DZ = ({R.case_id(c): c for c in t} for t in (R.FWD_CASES, R.WGRAD_CASES, R.DBZ_CASES))
# mistake -> (table, error / bound of a case under it, the case named to catch it, every case that must catch it)
MISTAKES = {
    "first K chunk only": (WG, _wgrad(lambda i, r: R.mistake_first_k_chunk_only(i)), "wgrad-40x72x36",
                           {"wgrad-40x72x36", "wgrad-37x68x68", "wgrad-64x64x128"}),
    "ragged chunk reads on": (WG, _wgrad(lambda i, r: R.mistake_ragged_chunk_reads_on(i)), "wgrad-40x72x36",
                              {"wgrad-2x4x4", "wgrad-40x72x36", "wgrad-37x68x68"}),
    "d for dm in the stack's row stride": (FW, _fwd_c(_stride_d), "fwd-2x40x72x36",
                                           {"fwd-2x40x72x36", "fwd-3x64x260x128", "fwd-16x8x516x20"}),
    "segment one off at a boundary": (FW, _fwd_c(_one_off), "fwd-1x4x4x4", set(FW)),
    "s (x) b_z left out": (WG, _wgrad(lambda i, r: R.mistake_no_s_bz(i)), "wgrad-2x4x4", set(WG)),
    "rows >= d behind dw0": (WG, _wgrad(R.mistake_dw1_rows_into_dw0), "wgrad-37x68x68", set(WG)),
    "last ragged part dropped": (DZ, _dbz(lambda i, r: R.mistake_last_ragged_part_dropped(i)), "dbz-33x257",
                                 {"dbz-1x1", "dbz-31x7", "dbz-33x257", "dbz-257x260"}),
    "parts 0..7 only": (DZ, _dbz(lambda i, r: R.mistake_first_8_parts_only(i)), "dbz-257x260", {"dbz-257x260", "dbz-2048x36"}),
    "columns >= 256 unwritten": (DZ, _dbz(lambda i, r: R.mistake_cols_from_256_unwritten(r)), "dbz-33x257",
                                 {"dbz-33x257", "dbz-257x260"}),
    "b_kv left out of c": (FW, _fwd_c(R.mistake_no_b_kv), "fwd-16x8x516x20", set(FW)),
}


@pytest.mark.parametrize("name", list(MISTAKES))
def test_every_mistake_is_caught_by_a_named_case(name):
    table, moved_of, named, catchers = MISTAKES[name]
    moved = {cid: moved_of(c) for cid, c in table.items()}
    print(f"`{name}`: error / bound", {k: (v if math.isinf(v) else round(v, 1)) for k, v in moved.items()})
    assert named in catchers and moved[named] > 1.0, f"`{name}` moves {named} by only {moved[named]:.2f} x the bound"
    for cid, v in moved.items():
        if cid in catchers:
            assert v > 1.0, f"`{name}` moves {cid} by only {v:.2f} x the bound"
        else:
            assert v == 0.0, f"`{name}` should not change {cid} at all"


def test_the_reference_itself_passes_its_own_judge():
    for table, run in ((FW, _fwd_c(lambda i, r: r.c)), (WG, _wgrad(lambda i, r: r.dw)), (DZ, _dbz(lambda i, r: r.dbz))):
        assert all(run(c) == 0.0 for c in table.values())


# ------------------------------------------------------------------------------------------------ the algebra
@pytest.mark.parametrize("c", [R.FWD_CASES[1], R.FWD_CASES[3]], ids=R.case_id)
def test_folded_formulas_equal_the_unfolded_ones_in_fp64(c):
    inp = R.inputs(c)
    Mv = 5
    g = torch.Generator().manual_seed(9)
    z = torch.randn(Mv, c.lat, generator=g, dtype=torch.float64)
    wkv = [torch.cat([inp.w[2 * l], inp.w[2 * l + 1]]).double() for l in range(c.layers)]
    bkv = [torch.cat([inp.b[2 * l], inp.b[2 * l + 1]]).double() for l in range(c.layers)]
    dkv = [torch.randn(Mv, 2 * c.d, generator=g, dtype=torch.float64) for _ in range(c.layers)]
    un = R.unfolded(z, inp.wz.double(), inp.bz.double(), wkv, bkv, dkv)
    fo = R.folded(z, inp.wz.double(), inp.bz.double(), wkv, bkv, dkv)
    assert set(un) == set(fo) == {"kvb", "dW_kv", "db_kv", "dW_z", "db_z", "dz"}
    for name in un:
        u, f = un[name], fo[name]
        u, f = (torch.stack(u), torch.stack(f)) if isinstance(u, list) else (u, f)
        assert u.shape == f.shape
        assert float((u - f).abs().max()) <= 1e-12 * float(u.abs().max()), name


# ------------------------------------------------------------------------------------------------ KvFold.usable
def _modules(layers=2, d=8, dm=12, lat=4):
    lin = lambda o, i: SimpleNamespace(weight=torch.zeros(o, i), bias=torch.zeros(o))           # noqa: E731
    return [(lin(d, dm), lin(d, dm)) for _ in range(layers)], lin(dm, lat)


def test_kv_fold_usable_truth_table():
    from gct_plus_amd import ops
    usable = ops.KvFold.usable
    kv, fc_z = _modules()
    assert all(m.weight.data_ptr() % 16 == 0 for pair in kv for m in pair) and fc_z.weight.data_ptr() % 16 == 0
    assert usable(kv, fc_z) is True
    assert usable(*_modules(layers=ops.KV_FOLD_MAX_LAYERS)) is True and ops.KV_FOLD_MAX_LAYERS == R.MAX_LAYERS
    assert not usable([], fc_z)                                                # no layers
    assert not usable(*_modules(layers=ops.KV_FOLD_MAX_LAYERS + 1))            # 17 layers
    kv, fc_z = _modules()
    fc_z.bias = None
    assert not usable(kv, fc_z)
    for which in (0, 1):                                                       # a k bias, a v bias
        kv, fc_z = _modules()
        kv[1][which].bias = None
        assert not usable(kv, fc_z)
    assert not usable(*_modules(d=6)) and not usable(*_modules(dm=6)) and not usable(*_modules(lat=6))
    kv, fc_z = _modules()
    fc_z.weight = torch.zeros(16, 4)                                           # fc_z.weight.shape[0] != dm
    assert not usable(kv, fc_z)
    kv, fc_z = _modules()
    kv[1][1].weight = torch.zeros(12, 12)                                      # a layer with another weight shape
    assert not usable(kv, fc_z)
    kv, fc_z = _modules()
    kv[0][1].weight = torch.zeros(12, 8).t()                                   # the right shape, not contiguous
    assert kv[0][1].weight.shape == (8, 12) and not usable(kv, fc_z)
    kv, fc_z = _modules()
    fc_z.weight = torch.zeros(4, 12).t()
    assert fc_z.weight.shape == (12, 4) and not usable(kv, fc_z)
    for target in ("kv", "fc_z"):                                              # 4 bytes off a 16-byte boundary
        kv, fc_z = _modules()
        flat = torch.zeros(8 * 12 + 4)
        assert flat.data_ptr() % 16 == 0
        if target == "kv":
            kv[1][0].weight = flat[1:1 + 8 * 12].view(8, 12)
            assert kv[1][0].weight.data_ptr() % 16 == 4 and kv[1][0].weight.is_contiguous()
        else:
            fc_z.weight = flat[1:1 + 12 * 4].view(12, 4)
            assert fc_z.weight.data_ptr() % 16 == 4
        assert not usable(kv, fc_z)
