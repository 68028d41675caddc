"""The three decode-step kernels tests/test_decode_step_kernels_gpu.py leaves out, each against a plain host reference
of its own operation (tests/decode_aux_ref.py, written from include/gctplus_hip.h and held to itself in
tests/test_decode_aux_ref_host.py):
  gct_attn_decode_z     latent widths, head counts, every residue of the padded score rows, masks, klen, condition
                        rows, the large-LDS path, strides with NaN gaps, refusals
  gct_attn_decode_beam  maps (random ancestry, entries to clamp, identity against gct_attn_decode), guard rows, the
                        step's own flag, the appended cache row, no room
  gct_stream_refill     every field of GctStreamState after one call for every kind of row, and a whole scripted stream
Every output buffer starts as NaN (a sentinel for integers); whatever a kernel must not touch is compared bit for bit."""
import ctypes

import pytest
import torch

from gct_plus_amd import ops
from tests import decode_aux_ref as A
from tests.test_decode_step_kernels_gpu import ATOL, RTOL, same_bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
assert RTOL == ATOL == A.Z_TOL == 1e-5


def ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================ gct_attn_decode_z
class ZCall:
    """The operands of a tests/decode_aux_ref.ZCase on the device, with `gap` floats of NaN between everything the
    strides can separate (gap = 0: the tight layout): qoff > H dk, ldq > qoff + H lat, z_batch > Le lat,
    ld_ckv > 2 H dk, ckv_batch > nc ld_ckv, valid_sb > Lk (flags 1 behind the row), ooff > H dk, ldo > ooff + H lat."""

    def __init__(self, c, gap):
        n, H, dk, lat, Le, nc = A.Z_N, c.H, c.dk, c.lat, c.Le, c.nc
        d, Lk = H * dk, nc + Le
        self.c, self.d = c, d
        self.qoff = self.ooff = d + gap
        self.ldq = self.ldo = d + gap + H * lat + gap
        self.z_batch = Le * lat + gap
        self.ld_ckv = 2 * d + gap
        self.ckv_batch = nc * self.ld_ckv + gap
        self.valid_sb = Lk + (3 if gap else 0)
        q = torch.full((n, self.ldq), NAN)
        q[:, :d], q[:, self.qoff:self.qoff + H * lat] = c.q.reshape(n, d), c.qf.reshape(n, H * lat)
        z = torch.full((n, self.z_batch), NAN)
        z[:, :Le * lat] = c.z.reshape(n, Le * lat)
        ckv = None
        if nc:
            ckv = torch.full((n, self.ckv_batch), NAN)
            rows = ckv[:, :nc * self.ld_ckv].view(n, nc, self.ld_ckv)
            rows[:, :, :d], rows[:, :, d:2 * d] = c.ck.reshape(n, nc, d), c.cv.reshape(n, nc, d)
        valid = torch.ones(n, self.valid_sb, dtype=torch.uint8)
        valid[:, :Lk] = c.valid
        self.q, self.z, self.valid, self.klen = q.cuda(), z.cuda(), valid.cuda(), c.klen.cuda()
        self.ckv = None if ckv is None else ckv.cuda()

    def run(self, b0=0, n=A.Z_N, Le=None, klen=True):
        """Samples b0 .. b0 + n - 1 into rows 1 .. n of a NaN buffer of n + 2 rows -> that buffer on the host."""
        c = self.c
        out = torch.full((n + 2, self.ldo), NAN, device="cuda")
        rc = ops._L().gct_attn_decode_z(
            ptr(self.q[b0:]), self.ldq, self.qoff, ptr(self.z[b0:]), self.z_batch, c.lat, c.Le if Le is None else Le,
            None if self.ckv is None else ptr(self.ckv[b0:]), self.ckv_batch, self.ld_ckv, c.nc, ptr(self.valid[b0:]),
            self.valid_sb, ptr(self.klen[b0:]) if klen else None, ptr(out[1:]), self.ldo, self.ooff, n, c.H, c.dk, c.scale,
            ops._st())
        ops.check(rc, "gct_attn_decode_z")
        torch.cuda.synchronize()
        return out.cpu()

    def split(self, out_all):
        """(ctx [n, H, lat], cond [n, H dk]) of a buffer `run` returned, after checking that nothing else was written:
        the guard rows, the gaps and, without condition rows, the columns [0, H dk) still hold NaN bit for bit."""
        c, d = self.c, self.d
        n = out_all.shape[0] - 2
        lo, hi = self.ooff, self.ooff + c.H * c.lat
        want = torch.full_like(out_all, NAN)
        want[1:n + 1, lo:hi] = out_all[1:n + 1, lo:hi]
        if c.nc:
            want[1:n + 1, :d] = out_all[1:n + 1, :d]
        assert same_bits(out_all, want), "written outside the two output column ranges"
        return out_all[1:n + 1, lo:hi].reshape(n, c.H, c.lat), out_all[1:n + 1, :d]


def check_z(c, gap, bitwise):
    """One case: both outputs within the tolerance of the fp64 reference, nothing else written; bitwise: every sample
    equals a one-sample call, and the sample with a visible prefix a call without klen on klen - nc latent rows.
    Returns the worst error / tolerance."""
    call = ZCall(c, gap)
    out_all = call.run()
    ctx, cond = call.split(out_all)
    want_ctx, want_cond = c.reference()
    worst = A.worst_ratio(ctx, want_ctx)
    if c.nc:
        worst = max(worst, A.worst_ratio(cond.reshape(A.Z_N, c.H, c.dk), want_cond))
    what = (c.lat, c.H, c.dk, c.Le, c.nc, gap)
    assert worst <= 1.0, (what, worst)
    Lk = c.nc + c.Le
    if int(c.valid[3].sum()) == 0 and int(c.klen[3]) == Lk:              # no visible key: the mean of the z rows
        mean = c.z[3].double().mean(0) * c.Le / Lk
        assert A.worst_ratio(ctx[3], mean.expand(c.H, c.lat)) <= 1.0, what
    if bitwise:
        for b in range(A.Z_N):
            one = call.run(b0=b, n=1)
            call.split(one)
            assert same_bits(one[1], out_all[1 + b]), (what, b)
        one = call.run(b0=2, n=1, Le=int(c.klen[2]) - c.nc, klen=False)
        assert same_bits(one[1], out_all[3]), what
    return worst


def test_attn_decode_z_large_lds_case_then_a_small_one():
    """Le = 256 at lat = 128 with 8 heads needs 147 KB of dynamic LDS (the attribute is raised once); the small case
    behind it runs under the raised attribute."""
    big = check_z(A.z_case(128, 8, 64, 256, 3), 4, False)
    small = check_z(A.z_case(4, 2, 16, 1, 0), 4, False)
    print(f"attn_decode_z 147 KB of LDS, then 20 B: worst error / tolerance = {big:.3f}, {small:.3f}")


@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("H,dk", A.Z_HEADS)
@pytest.mark.parametrize("lat", A.Z_LAT)
def test_attn_decode_z_grid(lat, H, dk, gap):
    worst = 0.0
    for Le in A.Z_LE:
        for nc in A.Z_NC:
            worst = max(worst, check_z(A.z_case(lat, H, dk, Le, nc), gap, bitwise=gap == 0))
    print(f"attn_decode_z lat {lat} H {H} dk {dk} gap {gap}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("klen", [2, 3])
def test_attn_decode_z_klen_inside_the_condition_rows(klen, gap):
    """nc = 3 and klen = 2 or 3: no latent row is visible, ctx is exactly 0 and cond the attention over the klen
    condition rows; every z row and the condition rows behind klen are NaN."""
    c = A.z_case(16, 3, 32, 5, 3, klen=klen)
    call = ZCall(c, gap)
    ctx, cond = call.split(call.run())
    assert bool((ctx == 0).all())
    worst = A.worst_ratio(cond.reshape(A.Z_N, c.H, c.dk), c.reference()[1])
    print(f"attn_decode_z klen {klen} of nc 3, gap {gap}: worst error / tolerance = {worst:.3f}")
    assert worst <= 1.0


def test_attn_decode_z_refusals_and_empty_batch():
    """Every refused call returns an error and writes nothing; n = 0 returns OK and writes nothing.  The buffers are
    large enough for every variant, so a call that was not refused would still stay inside them."""
    n, H, dk = 2, 2, 16
    q = torch.randn(n, 4096, device="cuda")
    z = torch.randn(n, 300 * 136, device="cuda")
    ckv = torch.randn(n, 8 * 600, device="cuda")
    valid = torch.ones(n, 300, dtype=torch.uint8, device="cuda")
    out = torch.full((n, 4096), NAN, device="cuda")
    nan = out.cpu()
    base = dict(ldq=4096, qoff=32, z_batch=300 * 136, lat=16, Le=8, ckv=ckv, ckv_batch=8 * 600, ld_ckv=600, nc=3, ldo=4096,
                ooff=32, n=n, H=H, dk=dk)

    def call(**kw):
        a = dict(base, **kw)
        rc = ops._L().gct_attn_decode_z(ptr(q), a["ldq"], a["qoff"], ptr(z), a["z_batch"], a["lat"], a["Le"], ptr(a["ckv"]),
                                        a["ckv_batch"], a["ld_ckv"], a["nc"], ptr(valid), 300, None, ptr(out), a["ldo"],
                                        a["ooff"], a["n"], a["H"], a["dk"], 0.25, ops._st())
        torch.cuda.synchronize()
        return rc

    refused = [dict(lat=6), dict(lat=132), dict(Le=257, nc=0), dict(Le=257), dict(nc=4, Le=256), dict(ckv=None),
               dict(ld_ckv=2 * H * dk - 4), dict(qoff=34), dict(ooff=34), dict(ldq=4098), dict(ldo=4098),
               dict(z_batch=300 * 136 + 2), dict(H=0)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert same_bits(out.cpu(), nan), kw
    assert call(n=0) == 0 and same_bits(out.cpu(), nan)
    assert call() == 0 and bool(torch.isfinite(out[:, :32]).all()) and bool(torch.isfinite(out[:, 32:64]).all())


# ================================================================================================ gct_attn_decode_beam
def run_beam(c, cache_off, plain=False):
    """One launch on device copies of the case; o is rows 1 .. n, columns [0, d) of a NaN buffer.  plain: gct_attn_decode
    (the case's map is the identity).  -> (o buffer, kc_all, vc_all) on the host, after checking that the flags, the map,
    the step row and *pos did not change."""
    n, d, H, dk = c.n, c.d, c.H, c.dk
    qkv, kc_all, vc_all, valid_all, kv_src = (t.cuda() for t in (c.qkv, c.kc_all, c.vc_all, c.valid_all, c.kv_src))
    kc, vc, valid = c.rows(kc_all), c.rows(vc_all), c.rows(valid_all)
    obuf = torch.full((n + 2, d + 4), NAN, device="cuda")
    pos = torch.tensor([c.Lold - cache_off], dtype=torch.int32, device="cuda")
    step = dict(knew=qkv[:, d:], vnew=qkv[:, 2 * d:], ldn=qkv.stride(0))
    if plain:
        ops.attn_decode(qkv, qkv.stride(0), kc, vc, kc.stride(1), kc.stride(0), valid, valid.stride(0), obuf[1:n + 1, :d],
                        n, H, 0, dk, pos=pos, cache_off=cache_off, **step)
    else:
        ops.attn_decode_beam(qkv, qkv.stride(0), kc, vc, kc.stride(1), kc.stride(0), valid, valid.stride(0),
                             obuf[1:n + 1, :d], n, H, c.T, dk, pos, cache_off, step["knew"], step["vnew"], step["ldn"],
                             kv_src)
    torch.cuda.synchronize()
    assert int(pos) == c.Lold - cache_off
    assert torch.equal(valid_all.cpu(), c.valid_all) and torch.equal(kv_src.cpu(), c.kv_src) and same_bits(qkv.cpu(), c.qkv)
    return obuf.cpu(), kc_all.cpu(), vc_all.cpu()


def appended(c):
    """The caches after the step: cache row Lold of physical row b holds the step's key / value."""
    kc, vc, d = c.kc_all.clone(), c.vc_all.clone(), c.d
    kc[1:c.n + 1, c.Lold, :d], vc[1:c.n + 1, c.Lold, :d] = c.qkv[:, d:2 * d], c.qkv[:, 2 * d:3 * d]
    return kc, vc


@pytest.mark.parametrize("cache_off", [0, 3])
@pytest.mark.parametrize("dk", [16, 32, 64])
def test_attn_decode_beam_maps(dk, cache_off):
    """Lold = cache_off + *pos at every count of the list: o is the attention over the Lold mapped keys (flags through
    the map) and the step's own key (flag of row b); cache row Lold of row b becomes the step's key / value bit for bit;
    no other byte of the allocations, guard rows included, changes.  With the identity map: gct_attn_decode's bits."""
    worst = 0.0
    for i, (T, Lold) in enumerate(A.BEAM_LOLD):
        for kind in ("random", "clamp", "identity"):
            c = A.beam_case(dk, Lold, T, kind, seed=1000 * dk + 10 * i + (kind == "clamp"))
            obuf, kc, vc = run_beam(c, cache_off)
            o = obuf[1:c.n + 1, :c.d]
            want = torch.full_like(obuf, NAN)
            want[1:c.n + 1, :c.d] = o
            assert same_bits(obuf, want), "o written outside its rows and columns"
            ratio = A.worst_ratio(o.reshape(c.n, c.H, dk), A.beam_reference(c))
            assert ratio <= 1.0, (dk, cache_off, T, Lold, kind, ratio)
            worst = max(worst, ratio)
            kw, vw = appended(c)
            assert same_bits(kc, kw) and same_bits(vc, vw), (dk, cache_off, T, Lold, kind)
            if kind == "identity":
                obuf1, kc1, vc1 = run_beam(c, cache_off, plain=True)
                assert same_bits(obuf1, obuf) and same_bits(kc1, kc) and same_bits(vc1, vc), (dk, cache_off, T, Lold)
    print(f"attn_decode_beam dk {dk} cache_off {cache_off}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("dk", [16, 32, 64])
def test_attn_decode_beam_without_room_writes_nothing(dk):
    """Lold = T = 208 in a 256-row allocation: no room for this step's key, o stays NaN and the caches as they were."""
    c = A.beam_case(dk, 208, 208, "random", seed=dk)
    obuf, kc, vc = run_beam(c, 3)
    assert bool(obuf.isnan().all()) and same_bits(kc, c.kc_all) and same_bits(vc, c.vc_all)


# ================================================================================================ gct_stream_refill
def on_device(allocs):
    return {name: (t.cuda(), shape) for name, (t, shape) in allocs.items()}


def bound(state, **over):
    """An ops.StreamState pointing at the tensors of tests/decode_aux_ref.stream_state (fields of `over` replaced).  The
    addresses are taken from the storage: a pool of no items still lies inside its allocation, it is not NULL."""
    def addr(x):
        if isinstance(x, (list, tuple)):
            return [addr(y) for y in x]
        if isinstance(x, torch.Tensor):
            return x.untyped_storage().data_ptr() + x.storage_offset() * x.element_size()
        return x

    st = ops.StreamState()
    st.set(**{name: addr(over.get(name, state[name])) for name, _ in st.fields})
    return st


def raw_refill(st):
    rc = ops._L().gct_stream_refill(ctypes.addressof(st.words), ops._st())
    torch.cuda.synchronize()
    return rc


def assert_state(dev, host, what):
    """Every allocation, margins included, equal bit for bit."""
    for name, (t, _) in host.items():
        got = dev[name][0].cpu()
        if not A.same(got, t):
            at = int((got.view(torch.int32 if t.dtype == torch.float32 else t.dtype) !=
                      t.view(torch.int32 if t.dtype == torch.float32 else t.dtype)).nonzero()[0]) - A.MARGIN
            raise AssertionError(f"{what}: {name} differs at flat index {at} (negative / beyond the tensor: a margin): "
                                 f"got {got[at + A.MARGIN]}, want {t[at + A.MARGIN]}")


def one_call(geom, allocs, what):
    """The call on a device copy against the reference on the host copy."""
    dev = on_device(allocs)
    assert raw_refill(bound(A.stream_state(geom, dev))) == 0, what
    A.stream_refill_reference(A.stream_state(geom, allocs))
    assert_state(dev, allocs, what)


STREAM_SHAPES = [(R, lay) for R in (1, 5, 255, 256, 257, 600) for lay in ("small", "mid")] + [(1, "wide"), (5, "wide")]


@pytest.mark.parametrize("R,layout", STREAM_SHAPES + [(257, "wide")])
def test_stream_refill_first_call(R, layout):
    """item = -1 everywhere and *pos = -1: the first min(R, N) items enter rows 0, 1, ... and the other rows park."""
    Ns = [R] if (layout == "wide" and R > 5) else sorted({N for N in (0, R - 2, R, 3 * R + 3) if N >= 0})
    for N in Ns:
        geom, allocs = A.stream_alloc(R, N, layout, seed=R + N)
        one_call(geom, allocs, f"first call R {R} N {N} {layout}")
        s = A.stream_state(geom, allocs)
        assert int(s["next_item"][0]) == min(R, N) and s["item"].tolist() == [r if r < N else -1 for r in range(R)]
    print(f"stream_refill first call R {R} {layout}: every field equal for N in {Ns}")


@pytest.mark.parametrize("R,layout", STREAM_SHAPES)
def test_stream_refill_mid_stream(R, layout):
    """*pos = 9 over rows of every kind, the pool nearly empty; for more than 256 rows also with items left for the first
    wanting rows of the second scan pass only; then the same state with *enable = 0: nothing changes, scratch included."""
    wanting256 = sum(A.STREAM_KINDS[r % 7] not in ("one short", "in the prefix, done set") for r in range(min(R, 256)))
    for spare in [3] + ([wanting256 + 2] if R > 256 else []):
        geom, allocs = A.stream_midstream(R, layout, spare, seed=7 * R + spare)
        one_call(geom, allocs, f"mid-stream R {R} spare {spare} {layout}")
        s = A.stream_state(geom, allocs)
        taken = min(spare, int(s["fresh"].sum()))
        assert int(s["next_item"][0]) == geom["items"] - spare + taken and int(s["n_harvested"][0]) >= 8
        assert sum(i >= geom["items"] - spare for i in s["item"].tolist()) == taken
    geom, allocs = A.stream_midstream(R, layout, 3, seed=7 * R + 3)
    A.stream_state(geom, allocs)["enable"][0] = 0
    before = {name: t.clone() for name, (t, _) in allocs.items()}
    one_call(geom, allocs, f"mid-stream R {R} {layout} enable 0")
    assert all(A.same(allocs[name][0], t) for name, t in before.items())
    print(f"stream_refill mid-stream R {R} {layout}: every field equal")


@pytest.mark.parametrize("R,layout", [(8, "mid"), (300, "small")])
def test_stream_refill_chained_scripted_stream(R, layout):
    """A whole stream of N = 5 R + 3 items without a model, *pos advanced by gct_decode_advance, the step's tokens and
    done flags written by the test: the whole state equals the reference's after every call."""
    geom, allocs, raises_done = A.stream_script(R, layout, seed=20 + R)
    dev = on_device(allocs)
    s, sd = A.stream_state(geom, allocs), A.stream_state(geom, dev)
    st = bound(sd)
    st.refill()
    A.stream_refill_reference(s)
    assert_state(dev, allocs, "first call")
    step = 0
    while int(s["n_harvested"][0]) < geom["items"]:
        assert step < 2000
        ops.check(ops._L().gct_decode_advance(sd["pos"].data_ptr(), ops._st()), "gct_decode_advance")
        s["pos"][0] = step
        writes = A.script_step(s, raises_done)
        A.apply_step(s, writes)
        A.apply_step(sd, writes)
        st.refill()
        torch.cuda.synchronize()
        A.stream_refill_reference(s)
        assert_state(dev, allocs, f"step {step}")
        step += 1
    assert torch.equal(s["out_len"], s["limit"]) and int(s["next_item"][0]) == geom["items"]
    print(f"stream_refill chained R {R} {layout}: every field equal after each of {step + 1} calls")


def test_stream_refill_refusals():
    """Every refused state returns an error and nothing is launched: the whole state stays as it was."""
    geom, allocs = A.stream_midstream(5, "mid", 3, seed=1)
    dev = on_device(allocs)
    s = A.stream_state(geom, dev)
    bad = [dict(rows=0), dict(rows=8193), dict(width=geom["T"] + 1), dict(ld_ys=geom["T"] - 1),
           dict(valid_sb=geom["valid_off"] + geom["T"] - 1), dict(t0_max=geom["width"] + 1), dict(z_row=6),
           dict(layers=17), dict(ckv=[None]), dict(ckv_pool=[None])]
    bad += [{name: None} for name, count in ops.StreamState().fields
            if count == 1 and name not in A.STREAM_GEOM_FIELDS]
    assert len(bad) == 10 + 24
    for over in bad:
        assert raw_refill(bound(s, **over)) != 0, over
        assert_state(dev, allocs, f"refused {over}")
    assert raw_refill(bound(s)) == 0
    A.stream_refill_reference(A.stream_state(geom, allocs))
    assert_state(dev, allocs, "the state that is not refused")
