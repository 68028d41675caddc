"""gct_kv_fold_fwd, gct_kv_fold_wgrad and gct_kv_fold_dbz against tests/kv_fold_ref.py (fp64 on the CPU, derived bounds)
through raw library calls, one entry point at a time with exact inputs, at the shapes where the kernels take other
branches than at d = d_model = 64, latent 32 (tests/test_kv_fold_ref_host.py lists the branches and shows that the tables
tell the likely mistakes apart):

  fwd    every case with and without b_addrs, without a_planes / with them at stride numel / at stride numel + 8, with and
         without the planes of W_z, in the fp32, bf16x6 and bf16x3 GEMM modes; 2 * layers separately allocated weights.
         wstack bit-exact, c and a inside their bounds (a under the route gct_gemm_last_route reports, which must be the
         one gct_linear_dgrad_route plans), hi + mid + lo of a_planes = a bit for bit, nothing written beyond numel.
  wgrad  dw0, dw1, db0, db1 separately allocated between NaN guard rows; db0 | db1 = s bit for bit.
  dbz    a workspace of exactly the parts' size; two calls bit-identical; one byte less is refused.
Every output starts as NaN (an unwritten element fails), every buffer ends in a guard that must stay as it was.
Argument errors return before any launch: non-zero, a message, the outputs untouched.  ops.KvFold itself at d = d_model
= 72, latent 36, 3 layers through the compound comparison of tests/test_kv_fold_gpu.py (its helpers, its FACTOR).

Of the five fwd geometries only 2 x 64 x 64 x 32 is planned onto a bf16 kernel once W_z has planes (X6); the others stay
on the fp32 vector kernel in every mode (their d_model or latent width is no multiple of 32), and so does A at d = 72.

Measured on MI355X, worst error / bound per entry point (printed at the end of the module with -s):
  c 0.164 (1 x 4 x 4 x 4 without biases)     dW 0.151 (d 2; 0.02 - 0.11 at the others)     db_z 0.336 (1 row; 0.055 at 33, 1e-4 at 2 048)
  a: F32_VEC 0.328 (1 x 4 x 4 x 4, the same in every mode)   F32_FAST 0.044   X6 bf16x6 0.036, bf16x3 0.064 (2 x 64 x 64 x 32)
  KvFold at 72 / 36 / 3: 1.53 x the floor of tests/test_kv_fold_gpu.py (dW_kv at 4 rows), against its FACTOR 4.
The 36 tests take under 3 s together."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import gemm_ref as G
from tests import kv_fold_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
NAN = float("nan")
SENTINEL = 0x5A5A                # int16 fill of a_planes
WORST = {}                       # worst error / bound per entry point


@pytest.fixture(scope="module")
def lib():
    from gct_plus_amd import _lib, ops
    keep = ops.gemm_get_mode()
    yield _lib.load()
    ops.gemm_set_mode(keep)
    for key in sorted(WORST):
        print(f"[kv fold edges] worst err / bound  {key}: {WORST[key][0]:.4f}  ({WORST[key][1]})")


def _st():
    return torch.cuda.current_stream().cuda_stream


def note(key, r, where):
    if r > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (r, where)


def nan_rows(rows, cols):
    """(allocation, view): [rows][cols] of NaN between one NaN guard row before and one after"""
    buf = torch.full((rows + 2, cols), NAN, device=DEV)
    return buf, buf[1:rows + 1]


def nan_vec(n):
    """(allocation, view): n NaN floats between guards of 4 floats (the view stays 16-byte aligned)"""
    buf = torch.full((n + 8,), NAN, device=DEV)
    return buf, buf[4:4 + n]


def guards_are_nan(buf):
    edge = (buf[0], buf[-1]) if buf.dim() == 2 else (buf[:4], buf[-4:])
    return all(bool(torch.isnan(e).all()) for e in edge)


class Ws:
    """a workspace of exactly `nbytes` (floats of `fill`) and a guard behind it"""

    def __init__(self, nbytes, fill=NAN):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
        self.buf[:nbytes // 4 * 4].view(torch.float32).fill_(fill)
        self.buf[nbytes // 4 * 4:] = 0xA5

    def ptr(self):
        return self.buf.data_ptr()

    def guard_intact(self):
        return bool((self.buf[(self.nbytes + 3) // 4 * 4:] == 0xA5).all())


def last_route(lib):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    assert lib.gct_gemm_last_route(ctypes.addressof(out)) == 0
    return tuple(out)


def planned_route(lib, c, mode, have_planes, ws_bytes):
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    rows = 2 * c.layers * c.d
    assert lib.gct_linear_dgrad_route(rows, 1, c.dm, c.lat, c.dm, c.lat, c.lat, G.DEPI_STORE, 1, int(have_planes), mode,
                                      ws_bytes, ctypes.addressof(out)) == 0
    return tuple(out)


# ------------------------------------------------------------------------------------------------ fwd
@functools.lru_cache(maxsize=None)
def fwd_setup(c):
    """inputs, the references with and without biases (computed once), the operands on the device"""
    from gct_plus_amd import ops
    inp = R.inputs(c)
    dev = dict(w=[t.to(DEV) for t in inp.w], b=[t.to(DEV) for t in inp.b], wz=inp.wz.to(DEV), bz=inp.bz.to(DEV))
    dev["wzp"] = ops.split_planes(dev["wz"].view(-1))
    ptrs = {t.data_ptr() for t in dev["w"]}
    assert len(ptrs) == 2 * c.layers and all(p % 16 == 0 for p in ptrs)
    torch.cuda.synchronize()
    return inp, {True: R.reference_fwd(inp, True), False: R.reference_fwd(inp, False)}, dev


def call_fwd(lib, c, dev, bias, a_stride, wz_planes, w_addrs=None, args=None):
    """one gct_kv_fold_fwd call into fresh NaN outputs; a_stride: None (no a_planes) or the plane stride; args: overrides
    of (layers, d, dm, lat) for the argument-error calls -> (rc, outputs)"""
    rows, n = 2 * c.layers * c.d, 2 * c.layers
    wa =(ctypes.c_int64 * len(w_addrs or dev["w"]))(*(w_addrs or [t.data_ptr() for t in dev["w"]]))
    ba = (ctypes.c_int64 * n)(*[t.data_ptr() for t in dev["b"]])
    o = dict(zip(("wstack_buf", "wstack"), nan_rows(rows, c.dm)))
    o.update(zip(("a_buf", "a"), nan_rows(rows, c.lat)))
    o.update(zip(("c_buf", "c"), nan_vec(rows)))
    o["planes"] = None if a_stride is None else torch.full((3 * a_stride,), SENTINEL, dtype=torch.int16, device=DEV)
    o["ws"] = Ws(int(lib.gct_kv_fold_ws_bytes(c.layers, c.d, c.dm, c.lat)))
    layers, d, dm, lat = args or c
    rc = lib.gct_kv_fold_fwd(layers, ctypes.addressof(wa), ctypes.addressof(ba) if bias else None, d, dm,
                             dev["wz"].data_ptr(), dev["wzp"].data_ptr() if wz_planes else None,
                             dev["wzp"].stride(0) if wz_planes else 0, dev["bz"].data_ptr(), lat, o["wstack"].data_ptr(),
                             o["a"].data_ptr(), o["c"].data_ptr(), None if a_stride is None else o["planes"].data_ptr(),
                             0 if a_stride is None else a_stride, o["ws"].ptr(), o["ws"].nbytes, _st())
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
def test_fwd_against_the_reference(lib, c, mode):
    from gct_plus_amd import ops
    inp, refs, dev = fwd_setup(c)
    rows, numel = 2 * c.layers * c.d, 2 * c.layers * c.d * c.lat
    keep = ops.gemm_get_mode()
    try:
        ops.gemm_set_mode(mode)
        first = {}
        for wz_planes in (False, True):
            for bias in (True, False):
                for a_stride in (None, numel, numel + 8):
                    rc, o = call_fwd(lib, c, dev, bias, a_stride, wz_planes)
                    what = f"{R.case_id(c)} {R.MODE_NAMES[mode]} wz planes {wz_planes} bias {bias} a_planes {a_stride}"
                    assert rc == 0, (what, lib.gct_last_error())
                    out8 = last_route(lib)
                    assert out8 == planned_route(lib, c, mode, wz_planes, o["ws"].nbytes), (what, out8)
                    if not wz_planes or mode == R.F32:
                        assert out8[0] not in G.BF16_KINDS, (what, out8)
                    ref = refs[bias]
                    assert all(guards_are_nan(o[k]) for k in ("wstack_buf", "a_buf", "c_buf")), what
                    assert o["ws"].guard_intact(), what
                    wstack, a, cc = o["wstack"].cpu(), o["a"].cpu(), o["c"].cpu()
                    assert torch.equal(wstack.view(torch.int32), ref.wstack.view(torch.int32)), what
                    rc_ = R.ratio(cc, ref.c, R.bound_c(ref, c))
                    ra = R.ratio(a, ref.a, R.bound_a(ref, mode, out8))
                    kind = G.KIND_NAMES[out8[0]]
                    note("fwd c", rc_, what)
                    note(f"fwd a [{R.MODE_NAMES[mode]}, {kind}]", ra, what)
                    assert rc_ <= 1.0, f"{what}: c is {rc_:.3f} x its bound"
                    assert ra <= 1.0, f"{what}: a ({kind}) is {ra:.3f} x its bound"
                    if a_stride is not None:
                        pl = o["planes"].cpu().view(3, a_stride)
                        assert torch.equal(R.planes_sum(pl, numel).view(torch.int32), a.reshape(-1).view(torch.int32)), what
                        assert bool((pl[:, numel:] == SENTINEL).all()), f"{what}: written beyond numel of a plane"
                    # the same operands give the same bits, whatever else the call was asked for
                    key = wz_planes
                    if key in first:
                        assert torch.equal(first[key].view(torch.int32), a.view(torch.int32)), what
                    first.setdefault(key, a)
        print(f"  {R.case_id(c)} [{R.MODE_NAMES[mode]}]: routes without / with W_z planes "
              f"{G.KIND_NAMES[planned_route(lib, c, mode, False, 0)[0]]} / {G.KIND_NAMES[planned_route(lib, c, mode, True, 0)[0]]}")
    finally:
        ops.gemm_set_mode(keep)


def test_the_planes_of_w_z_put_one_case_on_a_bf16_kernel(lib):
    """the bf16 product through wzp is held to its own bound by fwd-2x64x64x32, in both bf16 modes"""
    c = R.FwdCase(2, 64, 64, 32)
    assert c in R.FWD_CASES
    ws = int(lib.gct_kv_fold_ws_bytes(*c))
    for mode in (R.BF16X6, R.BF16X3):
        assert planned_route(lib, c, mode, True, ws)[0] in G.BF16_KINDS
        assert planned_route(lib, c, mode, False, ws)[0] not in G.BF16_KINDS
    assert planned_route(lib, c, R.F32, True, ws)[0] not in G.BF16_KINDS


# ------------------------------------------------------------------------------------------------ wgrad
def call_wgrad(lib, c, dev, lat=None):
    o = dict(zip(("dw0_buf", "dw0"), nan_rows(c.d, c.dm)))
    o.update(zip(("dw1_buf", "dw1"), nan_rows(c.d, c.dm)))
    o.update(zip(("db0_buf", "db0"), nan_vec(c.d)))
    o.update(zip(("db1_buf", "db1"), nan_vec(c.d)))
    rc = lib.gct_kv_fold_wgrad(dev["p"].data_ptr(), dev["s"].data_ptr(), c.d, c.lat if lat is None else lat,
                               dev["wz"].data_ptr(), dev["bz"].data_ptr(), c.dm, o["dw0"].data_ptr(), o["dw1"].data_ptr(),
                               o["db0"].data_ptr(), o["db1"].data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("c", R.WGRAD_CASES, ids=R.case_id)
def test_wgrad_against_the_reference(lib, c):
    inp = R.inputs(c)
    ref = R.reference_wgrad(inp)
    dev = {k: getattr(inp, k).to(DEV) for k in ("p", "s", "wz", "bz")}
    rc, o = call_wgrad(lib, c, dev)
    assert rc == 0, lib.gct_last_error()
    assert all(guards_are_nan(o[k]) for k in ("dw0_buf", "dw1_buf", "db0_buf", "db1_buf")), "a guard row was written"
    dw = torch.cat([o["dw0"].cpu(), o["dw1"].cpu()])
    db = torch.cat([o["db0"].cpu(), o["db1"].cpu()])
    assert torch.equal(db.view(torch.int32), ref.db.view(torch.int32))
    r = R.ratio(dw, ref.dw, R.bound_w(ref, c))
    print(f"  {R.case_id(c)}: err / bound {r:.4f}")
    note("wgrad dW", r, R.case_id(c))
    assert r <= 1.0, f"{R.case_id(c)}: dW is {r:.3f} x its bound"
    rc, o2 = call_wgrad(lib, c, dev)
    assert rc == 0 and all(torch.equal(o[k].view(torch.int32), o2[k].view(torch.int32)) for k in ("dw0", "dw1", "db0", "db1"))


# ------------------------------------------------------------------------------------------------ dbz
def call_dbz(lib, rows, dm, wstack, s, ws):
    buf, dbz = nan_vec(dm)
    rc = lib.gct_kv_fold_dbz(wstack.data_ptr(), s.data_ptr(), rows, dm, dbz.data_ptr(), ws.ptr(), ws.nbytes, _st())
    torch.cuda.synchronize()
    return rc, buf, dbz


@pytest.mark.parametrize("c", R.DBZ_CASES, ids=R.case_id)
def test_dbz_against_the_reference(lib, c):
    inp = R.inputs(c)
    ref = R.reference_dbz(inp)
    wstack, s = inp.wstack.to(DEV), inp.s.to(DEV)
    need = R.dbz_parts(c) * c.dm * 4
    ws = Ws(need)
    rc, buf, dbz = call_dbz(lib, c.rows, c.dm, wstack, s, ws)
    assert rc == 0, lib.gct_last_error()
    assert guards_are_nan(buf) and ws.guard_intact()
    r = R.ratio(dbz.cpu(), ref.dbz, R.bound_dbz(ref, c))
    print(f"  {R.case_id(c)}: err / bound {r:.4f}")
    note("dbz", r, R.case_id(c))
    assert r <= 1.0, f"{R.case_id(c)}: db_z is {r:.3f} x its bound"
    ws0 = Ws(need, fill=0.0)                                   # deterministic, whatever the workspace held
    rc, buf2, dbz2 = call_dbz(lib, c.rows, c.dm, wstack, s, ws0)
    assert rc == 0 and torch.equal(dbz.view(torch.int32), dbz2.view(torch.int32)) and ws0.guard_intact()
    short = Ws(need - 1)                                       # one byte less: refused, nothing written
    rc, buf3, dbz3 = call_dbz(lib, c.rows, c.dm, wstack, s, short)
    assert rc != 0 and b"kv_fold_dbz" in lib.gct_last_error()
    assert bool(torch.isnan(buf3).all()) and short.guard_intact()
    assert bool(torch.isnan(short.buf[:(need - 1) // 4 * 4].view(torch.float32)).all())


@pytest.mark.parametrize("c", R.FWD_CASES, ids=R.case_id)
def test_the_workspace_query_covers_fwd_and_dbz(lib, c):
    """gct_kv_fold_ws_bytes >= what gct_linear_dgrad and gct_kv_fold_dbz ask for at this geometry; a workspace of exactly
    that size serves both (test_fwd_against_the_reference checks the guard behind it for fwd)"""
    inp, refs, dev = fwd_setup(c)
    rows = 2 * c.layers * c.d
    have = int(lib.gct_kv_fold_ws_bytes(c.layers, c.d, c.dm, c.lat))
    assert have >= int(lib.gct_linear_dgrad_ws_bytes(rows, c.dm, c.lat))
    assert have >= (rows + R.KVF_ROWS - 1) // R.KVF_ROWS * c.dm * 4
    dc = R.DbzCase(rows, c.dm)
    wstack = refs[True].wstack
    s = R.rnd(rows, seed=77)
    ref = R.reference_dbz(SimpleNamespace(wstack=wstack, s=s))
    ws = Ws(have)
    rc, buf, dbz = call_dbz(lib, rows, c.dm, wstack.to(DEV), s.to(DEV), ws)
    assert rc == 0 and guards_are_nan(buf) and ws.guard_intact()
    r = R.ratio(dbz.cpu(), ref.dbz, R.bound_dbz(ref, dc))
    note("dbz", r, f"rows of {R.case_id(c)}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_return_before_any_launch(lib):
    """Host-side checks: every call below is refused with a message, launches nothing and leaves its outputs NaN."""
    c = R.FwdCase(2, 8, 8, 8)
    big = R.FwdCase(R.MAX_LAYERS + 1, 8, 8, 8)                 # operands and outputs large enough for every call below
    inp = R.inputs(big)
    dev = dict(w=[t.to(DEV) for t in inp.w], b=[t.to(DEV) for t in inp.b], wz=inp.wz.to(DEV), bz=inp.bz.to(DEV))
    dev["wzp"] = None
    addrs = [t.data_ptr() for t in dev["w"]]
    rc, o = call_fwd(lib, c, dict(dev, w=dev["w"][:4], b=dev["b"][:4]), True, None, False)
    assert rc == 0 and bool(torch.isfinite(o["a"]).all())      # the conforming call
    off4 = list(addrs)
    off4[3] += 4
    null = list(addrs)
    null[1] = 0
    bad = {"layers 0": dict(args=(0, 8, 8, 8)), "layers 17": dict(args=(R.MAX_LAYERS + 1, 8, 8, 8)),
           "d 6": dict(args=(2, 6, 8, 8)), "dm 6": dict(args=(2, 8, 6, 8)), "lat 6": dict(args=(2, 8, 8, 6)),
           "weight 4 bytes off": dict(args=tuple(c), w_addrs=off4), "null weight": dict(args=tuple(c), w_addrs=null)}
    for name, kw in bad.items():
        rc, o = call_fwd(lib, big, dev, True, 2 * big.layers * big.d * big.lat, False, **dict(dict(w_addrs=addrs), **kw))
        assert rc != 0, name
        msg = lib.gct_last_error()
        assert b"kv_fold_fwd" in msg, (name, msg)
        for k in ("wstack_buf", "a_buf", "c_buf"):
            assert bool(torch.isnan(o[k]).all()), f"{name}: {k} was written"
        assert bool((o["planes"] == SENTINEL).all()) and o["ws"].guard_intact(), name
    wc = R.WgradCase(8, 8, 8)
    winp = R.inputs(wc)
    wdev = {k: getattr(winp, k).to(DEV) for k in ("p", "s", "wz", "bz")}
    rc, o = call_wgrad(lib, wc, wdev)
    assert rc == 0 and bool(torch.isfinite(o["dw1"]).all())
    rc, o = call_wgrad(lib, wc, wdev, lat=6)
    assert rc != 0 and b"kv_fold_wgrad" in lib.gct_last_error()
    assert all(bool(torch.isnan(o[k]).all()) for k in ("dw0_buf", "dw1_buf", "db0_buf", "db1_buf"))


# ------------------------------------------------------------------------------------------------ ops.KvFold off the 64s
@pytest.mark.parametrize("D,LAT,LAYERS,Mv,planes", [(72, 36, 3, 4, False), (72, 36, 3, 132, False), (72, 36, 3, 132, True),
                                                   (64, 32, 2, 132, True)])
def test_kv_fold_object_against_fp64_and_the_unfolded_path(lib, D, LAT, LAYERS, Mv, planes, monkeypatch):
    """The compound comparison of tests/test_kv_fold_gpu.py (its helpers, its FACTOR) at d = d_model = 72, latent 36, 3
    layers: ragged tiles in gct_kv_fold_wgrad, a ragged K chunk, 14 dbz parts.  planes: the folded path finds planes
    registered for W_z -- at 64 / 32 / 2 that puts A = wstack W_z on the bf16x6 kernel, at 72 / 36 / 3 the planner keeps it
    on the fp32 vector kernel all the same (72 and 36 are no multiples of 32)."""
    from gct_plus_amd import ops
    from tests import test_kv_fold_gpu as K
    for name, v in (("D", D), ("LAT", LAT), ("LAYERS", LAYERS)):
        monkeypatch.setattr(K, name, v)
    x = K._inputs(Mv, 300 + Mv)
    ref = K._fp64(x)
    un = K._unfolded(x)
    if planes:
        plain = K._modules

        def with_planes(x):
            kv, fc_z = plain(x)
            ops.register_planes(fc_z.weight, ops.split_planes(fc_z.weight.view(-1)))
            return kv, fc_z
        monkeypatch.setattr(K, "_modules", with_planes)
        kind = ops.linear_dgrad_route(2 * LAYERS * D, 1, D, LAT, have_planes=True)[0]
        assert (kind in G.BF16_KINDS) == (D == 64), G.KIND_NAMES[kind]
    fo, fold = K._folded(x)
    torch.cuda.synchronize()
    assert (fold.L, fold.d, fold.dm, fold.lat) == (LAYERS, D, D, LAT)
    wst = torch.cat(x["wkv"])
    assert torch.equal(fold.wstack.cpu(), wst)
    pl = R.planes_sum(fold.a_planes.cpu(), fold.a.numel())
    assert torch.equal(pl.view(torch.int32), fold.a.cpu().view(-1).view(torch.int32))
    worst = 0.0
    for name in K.NAMES:
        r = ref[name]
        eu = float((un[name].cpu().double() - r).abs().max())
        ef = float((fo[name].cpu().double() - r).abs().max())
        floor = max(eu, 2.0 ** -24 * float(r.abs().max()))
        print(f"kv_fold D={D} LAT={LAT} Mv={Mv} planes={planes} {name}: unfolded err {eu:.3e} folded err {ef:.3e} "
              f"ratio to floor {ef / floor:.2f}")
        worst = max(worst, ef / floor)
        assert ef == ef and ef <= K.FACTOR * floor, (name, Mv, ef, eu, floor)
    note(f"KvFold compound D={D} planes={planes} (x floor, FACTOR {K.FACTOR})", worst, f"Mv={Mv}")
