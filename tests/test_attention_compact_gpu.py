"""The compact address modes of gct_attn_fwd / gct_attn_bwd (kstart / klen, qstart / qlen, cstart / nlive, kv_compact
bits 0 and 1) against fp64 dense attention over the full row space, in the combinations engine.mha_fwd / mha_bwd use:

  F1  attn_fwd(keys=KeyRows)                       k, v compact                       Lk <= 96 and > 96
  F2  attn_fwd(live=L, keys=L), L.fwd, self        q, o, k, v compact                 <= 96
  F3  attn_fwd(live=L, keys=KeyRows), cross        q, o; k, v compact                 Lk <= 96
  B1  attn_bwd(live=L, kv_compact=True), self      dout, dq, dk, dv compact           T <= 96 and > 96
  B2  attn_bwd(live=L, keys=L), L.fwd, self        everything compact                 <= 96
  B3  attn_bwd(live=L, keys=KeyRows), cross        dout, dq (L.fwd: q, o too); k, v, dk, dv compact
  B4  attn_bwd(keys=KeyRows)                       k, v, dk, dv compact               both

The maps come from the real ops.LiveRows.from_rows / ops.KeyRows; every compact buffer has LiveRows.SLACK rows behind
it.  Tolerances are test_attention's (o 1e-5 / 1e-5; dq, dk, dv 2e-5 / 1e-4); compact-against-dense comparisons under
dropout and of lse use the two-builds bound of tools/attn_fuzz.py --compare (1e-5 + 1e-4 * scale); everything else is
exact: rows that do not exist may hold anything finite without changing a bit of the result, and rows outside every
sample's [start, start + len) -- the slack rows too -- are never written."""
import math

import pytest
import torch

from tests.rowmap_ref import causal_pad_mask, prefix_live
from tests.test_kernels_gpu import close, ref_attention, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -123.5
SEED, SITE = 77, 5
O_TOL, G_TOL = (1e-5, 1e-5), (2e-5, 1e-4)
WORST = {}                   # worst error / tolerance per mode of the running test


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def _ratio(mode, what, got, ref, atol, rtol):
    """Assert |got - ref| <= atol + rtol |ref| (close) and keep the worst error / tolerance per mode."""
    err = (got.double() - ref.double()).abs()
    r = float((err / (atol + rtol * ref.double().abs())).max()) if err.numel() else 0.0
    WORST[mode] = max(WORST.get(mode, 0.0), r)
    close(got, ref, atol, rtol, f"{mode} {what}")
    return r


def _two_builds(mode, what, got, ref):
    """tools/attn_fuzz.py --compare: max |got - ref| <= 1e-5 + 1e-4 * max |ref|."""
    if not got.numel():
        return
    err = float((got.double() - ref.double()).abs().max())
    tol = 1e-5 + 1e-4 * (float(ref.abs().max()) + 1e-6)
    key = mode + " vs dense"
    WORST[key] = max(WORST.get(key, 0.0), err / tol)
    assert err <= tol, f"{mode} {what}: compact and dense calls differ by {err:.3e} > {tol:.3e}"


class Rows:
    """The rows of one operand: dense (plan None) or compact under a LiveRows / KeyRows plan read back from the device."""

    def __init__(self, plan, B, L):
        self.plan, self.B, self.L = plan, B, L
        if plan is None:
            self.n = [L] * B
            self.c = self.dn = torch.arange(B * L)
            self.rows, self.alloc = B * L, B * L + 8                  # 8 guard rows behind a dense output
        else:
            cs, self.n = plan.cstart[:B].cpu().tolist(), plan.n_b[:B].cpu().tolist()
            self.c = torch.tensor([cs[b] + t for b in range(B) for t in range(self.n[b])], dtype=torch.long)
            self.dn = torch.tensor([b * L + t for b in range(B) for t in range(self.n[b])], dtype=torch.long)
            self.rows, self.alloc = plan.Mc, plan.Mc + plan.SLACK
            assert len(set(self.c.tolist())) == self.c.numel() and (self.c.numel() == 0 or int(self.c.max()) < plan.Mc)

    def place(self, dense, fill):
        """dense [B*L, cols] on the host -> device buffer holding the existing rows; every other row is `fill`ed."""
        if self.plan is None:
            return dense.to(DEV)
        buf = fill((self.alloc, dense.shape[1]))
        buf[self.c] = dense[self.dn]
        return buf.to(DEV)

    def out(self, cols):
        return torch.full((self.alloc, cols), SENT, device=DEV)

    def split(self, buf):
        """device output buffer -> (existing rows on the host in dense order, `every other row kept the sentinel`)."""
        h = buf.cpu()
        other = torch.ones(h.shape[0], dtype=torch.bool)
        other[self.c] = False
        return h[self.c], bool((h[other] == SENT).all())


def _zeros(shape):
    return torch.zeros(shape)


def _garbage():
    g = torch.Generator().manual_seed(31)
    return lambda shape: (torch.rand(shape, generator=g) * 2 - 1) * 1e3


class Case:
    def __init__(self, ops, B, H, dk, Lq, Lk, qn, kn, self_attn):
        self.ops, self.B, self.H, self.dk, self.Lq, self.Lk, self.self_attn = ops, B, H, dk, Lq, Lk, self_attn
        d = self.d = H * dk
        self.Q, self.K, self.V = rnd(B * Lq, d, seed=2), rnd(B * Lk, d, seed=3), rnd(B * Lk, d, seed=4)
        self.DO = rnd(B * Lq, d, seed=5)
        self.qn, self.kn = qn, kn
        self.live = self.keys = None
        if qn is not None:
            qlive = prefix_live(B, Lq, qn)
            self.DO[~qlive.reshape(-1)] = 0.0                          # the premise of the plan: dead rows carry no gradient
            self.live = ops.LiveRows.from_rows(qlive.to(torch.uint8).to(DEV), B, Lq, causal_pad_mask(B, Lq, qn).to(DEV))
        if self_attn:
            self.mask = causal_pad_mask(B, Lq, qn)                     # [B,T,T]
            mfull = self.mask[:, None]
        else:
            assert min(kn) >= 1                                        # never a sample without a visible key
            self.mask = prefix_live(B, Lk, kn).to(torch.uint8)         # [B,Lk]
            mfull = self.mask[:, None, None, :]
            self.keys = ops.KeyRows(self.mask.to(DEV), B, Lk)
        for p_ in (self.live, self.keys):
            if p_ is not None:
                h = p_.host()
                assert h["violations"] == 0 and h["nonprefix"] == 0 and h["empty"] == 0
        self.maskd = self.mask.to(DEV)
        # fp64 reference over the full row space, dropout off
        sp = lambda t, L: t.double().view(B, L, H, dk).transpose(1, 2).requires_grad_()              # noqa: E731
        qd, kd, vd = sp(self.Q, Lq), sp(self.K, Lk), sp(self.V, Lk)
        oref, _ = ref_attention(qd, kd, vd, mfull, 1 / math.sqrt(dk))
        oref.backward(sp(self.DO, Lq).detach())
        un = lambda t, L: t.detach().transpose(1, 2).reshape(B * L, d)                               # noqa: E731
        self.ref = dict(o=un(oref, Lq), dq=un(qd.grad, Lq), dk=un(kd.grad, Lk), dv=un(vd.grad, Lk))
        self.dense = {}

    # ---- layouts: self-attention reads one fused [q|k|v] buffer, cross-attention q and [k|v]
    def _inputs(self, rq, rkv, fill):
        d = self.d
        if self.self_attn:
            assert rq.plan is rkv.plan
            qkv = rq.place(torch.cat([self.Q, self.K, self.V], 1), fill)
            return (qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, 3 * d, 3 * d), None
        q, kv = rq.place(self.Q, fill), rkv.place(torch.cat([self.K, self.V], 1), fill)
        return (q, kv, kv[:, d:], d, 2 * d, 2 * d), None

    def _grads(self, rd, rdkv):
        d = self.d
        if self.self_attn:
            assert rd.plan is rdkv.plan
            g = rd.out(3 * d)
            n = rd.rows
            return g, g, (g[:n], g[:n, d:], g[:n, 2 * d:], 3 * d, 3 * d, 3 * d), (slice(0, d), slice(d, 2 * d), slice(2 * d, 3 * d))
        dq, dkv = rd.out(d), rdkv.out(2 * d)
        return dq, dkv, (dq[:rd.rows], dkv[:rdkv.rows], dkv[:rdkv.rows, d:], d, 2 * d, 2 * d), \
            (slice(0, d), slice(0, d), slice(d, 2 * d))

    def fwd(self, p, live, keys, fill=_zeros):
        """-> (o rows in dense order, lse [B,H,Lq], untouched rows kept the sentinel)"""
        B, H, Lq, Lk, dk = self.B, self.H, self.Lq, self.Lk, self.dk
        rq, rkv = Rows(live, B, Lq), Rows(keys, B, Lk)
        (q, k, v, ldq, ldk, ldv), _ = self._inputs(rq, rkv, fill)
        ob = rq.out(self.d)
        _, lse, _ = self.ops.attn_fwd(q, k, v, ldq, ldk, ldv, self.maskd, B, H, Lq, Lk, dk, p, SEED, SITE,
                                      out=ob[:rq.rows], keys=keys, live=live)
        o, kept = rq.split(ob)
        return o, lse.cpu().view(B, H, Lq), kept

    def dense_run(self, p):
        """The dense GPU call with the same mask, seed and site: o, lse and the three gradients (host, dense rows)."""
        if p not in self.dense:
            B, H, Lq, Lk, dk, d = self.B, self.H, self.Lq, self.Lk, self.dk, self.d
            o, lse, kept = self.fwd(p, None, None)
            assert kept
            r = Rows(None, B, Lq)
            rk = Rows(None, B, Lk)
            (q, k, v, ldq, ldk, ldv), _ = self._inputs(r, rk, _zeros)
            gq, gkv, (dq, dk_, dv, a, b_, c), sl = self._grads(r, rk)
            od = o.to(DEV)
            self.ops.attn_bwd(q, k, v, ldq, ldk, ldv, self.maskd, od, self.DO.to(DEV), lse.reshape(-1).to(DEV), dq, dk_, dv,
                              a, b_, c, B, H, Lq, Lk, dk, p, SEED, SITE)
            self.dense[p] = dict(o=o, lse=lse, dq=r.split(gq)[0][:, sl[0]], dk=rk.split(gkv)[0][:, sl[1]],
                                 dv=rk.split(gkv)[0][:, sl[2]])
        return self.dense[p]

    def bwd(self, p, live, keys, kv_compact, fill=_zeros, poison_lse=False):
        """-> dict(dq, dk, dv: existing rows in dense order; kept: untouched rows kept the sentinel; the Rows used)"""
        B, H, Lq, Lk, dk = self.B, self.H, self.Lq, self.Lk, self.dk
        dn = self.dense_run(p)
        fwdc = live is not None and live.fwd
        rq = Rows(live if fwdc else None, B, Lq)                       # q, o
        rd = Rows(live, B, Lq)                                         # dout, dq
        rkv = Rows(keys, B, Lk)                                        # k, v
        rdkv = Rows(keys if keys is not None else (live if kv_compact else None), B, Lk)     # dk, dv
        (q, k, v, ldq, ldk, ldv), _ = self._inputs(rq, rkv, fill)
        o_in, dout = rq.place(dn["o"], fill), rd.place(self.DO, fill)
        if rq.plan is None and rd.plan is not None:                    # o and dout share one leading dimension: d
            assert o_in.stride(0) == dout.stride(0)
        lse = dn["lse"].clone()
        if poison_lse:     # a forward over compact query rows does not write the entries of rows that do not exist
            for b in range(B):
                lse[b, :, rd.n[b]:] = fill((H, Lq - rd.n[b]))
        gq, gkv, (dq, dk_, dv, a, b_, c), sl = self._grads(rd, rdkv)
        self.ops.attn_bwd(q, k, v, ldq, ldk, ldv, self.maskd, o_in, dout, lse.reshape(-1).to(DEV), dq, dk_, dv, a, b_, c,
                          B, H, Lq, Lk, dk, p, SEED, SITE, live=live, kv_compact=kv_compact, keys=keys)
        xq, kq = rd.split(gq)
        xkv, kkv = rdkv.split(gkv)
        return dict(dq=xq[:, sl[0]], dk=xkv[:, sl[1]], dv=xkv[:, sl[2]], kept=kq and kkv, rd=rd, rdkv=rdkv)


def _check_fwd(c, mode, live, keys):
    rq = Rows(live, c.B, c.Lq)
    exist = torch.zeros(c.B, c.H, c.Lq, dtype=torch.bool)
    for b in range(c.B):
        exist[b, :, :rq.n[b]] = True
    o0, lse0, kept = c.fwd(0.0, live, keys)
    assert kept, f"{mode}: a row outside every sample's rows was written"
    _ratio(mode, "o", o0, c.ref["o"][rq.dn], *O_TOL)
    for p in (0.0, 0.1):
        dn = c.dense_run(p)
        oz, lz, kz = (o0, lse0, kept) if p == 0.0 else c.fwd(p, live, keys)
        og, lg, kg = c.fwd(p, live, keys, fill=_garbage())
        assert kz and kg, f"{mode}: a row outside every sample's rows was written (p = {p})"
        assert torch.equal(oz, og) and torch.equal(lz[exist], lg[exist]), \
            f"{mode}: rows that do not exist changed the result (p = {p})"
        _two_builds(mode, f"o (p = {p})", oz, dn["o"][rq.dn])
        _two_builds(mode, f"lse (p = {p})", lz[exist], dn["lse"][exist])
    print(f"{mode} B={c.B} H={c.H} dk={c.dk} Lq={c.Lq} Lk={c.Lk}: worst error / tolerance {WORST[mode]:.3f} (fp64), "
          f"{WORST.get(mode + ' vs dense', 0.0):.3f} (dense call)")


def _check_bwd(c, mode, live, keys, kv_compact):
    fwdc = live is not None and live.fwd
    for p in (0.0, 0.1):
        z = c.bwd(p, live, keys, kv_compact)
        g = c.bwd(p, live, keys, kv_compact, fill=_garbage(), poison_lse=fwdc)
        assert z["kept"] and g["kept"], f"{mode}: a row outside every sample's rows was written (p = {p})"
        for w in ("dq", "dk", "dv"):
            assert torch.equal(z[w], g[w]), f"{mode}: rows that do not exist changed {w} (p = {p})"
        rd, rdkv = z["rd"], z["rdkv"]
        dn = c.dense_run(p)
        if p == 0.0:
            if kv_compact or (live is not None and keys is live):      # dk / dv of dead rows have no row: they must be zero
                dead = torch.ones(c.B * c.Lk, dtype=torch.bool)
                dead[rdkv.dn] = False
                assert not c.ref["dk"][dead].any() and not c.ref["dv"][dead].any()
            dead = torch.ones(c.B * c.Lq, dtype=torch.bool)
            dead[rd.dn] = False
            assert not c.ref["dq"][dead].any()                         # (and dq of the rows without a gradient)
            _ratio(mode, "dq", z["dq"], c.ref["dq"][rd.dn], *G_TOL)
            _ratio(mode, "dk", z["dk"], c.ref["dk"][rdkv.dn], *G_TOL)
            _ratio(mode, "dv", z["dv"], c.ref["dv"][rdkv.dn], *G_TOL)
        _two_builds(mode, f"dq (p = {p})", z["dq"], dn["dq"][rd.dn])
        _two_builds(mode, f"dk (p = {p})", z["dk"], dn["dk"][rdkv.dn])
        _two_builds(mode, f"dv (p = {p})", z["dv"], dn["dv"][rdkv.dn])
    print(f"{mode} B={c.B} H={c.H} dk={c.dk} Lq={c.Lq} Lk={c.Lk}: worst error / tolerance {WORST[mode]:.3f} (fp64), "
          f"{WORST.get(mode + ' vs dense', 0.0):.3f} (dense call)")


# (B, H, dk, Lq, Lk, visible keys per sample): 80, 70 and 17 keys run the direct kernels, 203, 97 and 100 the LDS ones;
# the last case has 528 (batch, head) pairs, more than the persistent workgroups of the LDS route
KEY_CASES = [(3, 4, 16, 33, 80, (80, 17, 1)), (1, 1, 32, 130, 70, (15,)), (5, 4, 64, 60, 203, (203, 97, 16, 1, 100)),
             (3, 1, 32, 5, 97, (97, 96, 17)), (3, 4, 64, 17, 17, (17, 16, 15)),
             (66, 8, 16, 20, 100, tuple(100 - (7 * b) % 60 for b in range(66)))]


@pytest.mark.parametrize("B,H,dk,Lq,Lk,kn", KEY_CASES)
def test_compact_keys(ops, B, H, dk, Lq, Lk, kn):
    """F1 and B4: k, v (and dk, dv) hold the visible keys only."""
    WORST.clear()
    c = Case(ops, B, H, dk, Lq, Lk, None, kn, False)
    _check_fwd(c, "F1", None, c.keys)
    _check_bwd(c, "B4", None, c.keys, False)


# (B, H, dk, T, live prefix per sample): T not a multiple of 4 except 96, so that samples share quads; lengths 1, T, 15,
# 16, 17 and an empty sample; T = 97 and 130 run the LDS backward (B1 only: compact q / o need the direct kernels)
SELF_CASES = [(3, 4, 16, 5, (1, 5, 0)), (5, 1, 32, 17, (17, 16, 15, 0, 1)), (3, 4, 64, 33, (17, 33, 15)),
              (1, 4, 16, 96, (95,)), (3, 1, 64, 97, (97, 16, 0)), (5, 4, 32, 130, (130, 17, 0, 1, 113))]


@pytest.mark.parametrize("B,H,dk,T,qn", SELF_CASES)
def test_compact_self_attention(ops, B, H, dk, T, qn):
    """F2, B1 and B2: the decoder's self-attention over its live rows (causal-and-padding mask)."""
    WORST.clear()
    c = Case(ops, B, H, dk, T, T, qn, None, True)
    c.live.fwd = False
    _check_bwd(c, "B1", c.live, None, True)
    if T <= ops.ATTN_DIRECT_MAX_KEYS:
        c.live.fwd = True
        _check_fwd(c, "F2", c.live, c.live)
        _check_bwd(c, "B2", c.live, c.live, False)


# (B, H, dk, Lq, Lk, live query prefix, visible keys)
CROSS_CASES = [(3, 4, 16, 33, 80, (17, 0, 33), (80, 17, 1)), (5, 1, 32, 130, 70, (130, 16, 0, 1, 15), (70, 16, 15, 1, 33)),
               (3, 4, 64, 60, 203, (60, 0, 17), (203, 97, 100)), (1, 4, 32, 5, 97, (3,), (96,)),
               (5, 4, 64, 33, 80, (1, 33, 15, 0, 16), (17, 80, 1, 16, 15))]


@pytest.mark.parametrize("B,H,dk,Lq,Lk,qn,kn", CROSS_CASES)
def test_compact_cross_attention(ops, B, H, dk, Lq, Lk, qn, kn):
    """F3 and B3 (forward dense and forward compact): live query rows over the visible keys of the memory."""
    WORST.clear()
    c = Case(ops, B, H, dk, Lq, Lk, qn, kn, False)
    c.live.fwd = False
    _check_bwd(c, "B3 (dense forward)", c.live, c.keys, False)
    if Lk <= ops.ATTN_DIRECT_MAX_KEYS:
        c.live.fwd = True
        _check_fwd(c, "F3", c.live, c.keys)
        _check_bwd(c, "B3 (compact forward)", c.live, c.keys, False)


def test_compact_argument_errors(ops):
    """Combinations the kernels do not have are refused before anything is launched."""
    from gct_plus_amd import _lib
    B, H, dk = 2, 2, 16
    d = H * dk

    def plans(T, Lk):
        L = ops.LiveRows.from_rows(prefix_live(B, T, (T, 3)).to(torch.uint8).to(DEV), B, T, causal_pad_mask(B, T, (T, 3)).to(DEV))
        K = ops.KeyRows(prefix_live(B, Lk, (Lk, 2)).to(torch.uint8).to(DEV), B, Lk)
        L.host()
        K.host()
        return L, K

    def bufs(L, K, T, Lk):
        rows = max(B * max(T, Lk), L.Mc, K.Mc) + L.SLACK
        return (torch.zeros(rows, 3 * d, device=DEV), torch.full((rows, 3 * d), SENT, device=DEV),
                torch.zeros(B * H * T, device=DEV))

    # qstart / qlen with more keys than the direct kernels take, and with a probs output
    for T, probs in ((97, False), (17, True)):
        L, K = plans(T, T)
        L.fwd = True
        x, out, _ = bufs(L, K, T, T)
        with pytest.raises(_lib.GctError):
            ops.attn_fwd(x, x[:, d:], x[:, 2 * d:], 3 * d, 3 * d, 3 * d, None, B, H, T, T, dk, 0.0, 0, 0, out=out[:, :d],
                         want_probs=probs, keys=L, live=L)
        torch.cuda.synchronize()
        assert (out == SENT).all()
    # kv_compact with Lq != Lk; kstart / klen together with kv_compact
    for T, Lk, with_keys in ((17, 20, False), (17, 17, True)):
        L, K = plans(T, Lk)
        x, out, lse = bufs(L, K, T, Lk)
        with pytest.raises(_lib.GctError):
            ops.attn_bwd(x, x[:, d:], x[:, 2 * d:], 3 * d, 3 * d, 3 * d, None, x[:, :d], x[:, d:2 * d], lse, out, out[:, d:],
                         out[:, 2 * d:], 3 * d, 3 * d, 3 * d, B, H, T, Lk, dk, 0.0, 0, 0, live=L, kv_compact=True,
                         keys=K if with_keys else None)
        torch.cuda.synchronize()
        assert (out == SENT).all()
