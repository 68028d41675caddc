"""Host references of the three decode-step kernels tests/decode_step_ref.py leaves out -- gct_attn_decode_z,
gct_attn_decode_beam, gct_stream_refill -- written from the statements in include/gctplus_hip.h, in plain torch on the
CPU, plus the inputs of their tests: tests/test_decode_aux_ref_host.py holds the references to themselves and shows
that the inputs tell a wrong kernel from a right one, tests/test_decode_aux_kernels_gpu.py holds the kernels to them."""
import math

import numpy as np
import torch

from tests.decode_step_ref import cached_attention

NAN = float("nan")


# ================================================================================================ gct_attn_decode_z
def latent_cross_attention(qf, q, z, ck, cv, valid, klen, scale, dtype=torch.float64):
    """The operation of gct_attn_decode_z, without folding matrices.  qf [n, H, lat] (the folded queries), q [n, H, dk]
    (the plain ones; unused without condition rows), z [n, Le, lat], ck / cv [n, nc, H, dk] (None: nc = 0), valid
    [n, >= nc + Le] uint8 or None (condition rows first), klen [n] or None -> (ctx [n, H, lat], cond [n, H, dk] or None).
    Per sample and head: scores q_h . ck_{j,h} for the nc condition rows, then qf_h . z_j for the latent rows, times
    scale, masked_fill(valid == 0, -1e9); ONE softmax over the first min(klen, nc + Le) keys -- the keys behind weigh 0
    and are not looked at (they may hold anything); ctx = sum_{j >= nc} p_j z_j, cond = sum_{j < nc} p_j cv_{j,h}.
    dtype = torch.float32 gives the plain fp32 restatement of the same sums."""
    n, H, lat = qf.shape
    Le = z.shape[1]
    nc = 0 if ck is None else ck.shape[1]
    ctx = torch.zeros(n, H, lat, dtype=dtype)
    cond = None if nc == 0 else torch.zeros(n, H, ck.shape[-1], dtype=dtype)
    for b in range(n):
        L = nc + Le if klen is None else min(int(klen[b]), nc + Le)
        c = min(nc, L)
        e = L - c
        zb = z[b, :e].to(dtype)
        s = torch.empty(H, L, dtype=dtype)
        if c:
            s[:, :c] = torch.einsum("hd,jhd->hj", q[b].to(dtype), ck[b, :c].to(dtype))
        s[:, c:] = qf[b].to(dtype) @ zb.T
        s = s * scale
        if valid is not None:
            s = s.masked_fill(valid[b, :L][None, :] == 0, -1e9)
        p = torch.softmax(s, -1)
        ctx[b] = p[:, c:] @ zb
        if nc:
            cond[b] = torch.einsum("hj,jhd->hd", p[:, :c], cv[b, :c].to(dtype))
    return ctx, cond


Z_TOL = 1e-5                                        # per element: Z_TOL + Z_TOL |ref|, on ctx and on cond
Z_LAT = (4, 16, 128)
Z_HEADS = ((2, 16), (3, 32), (8, 64))               # three heads leave the fourth wave idle, eight give two per wave
Z_LE = (1, 3, 4, 5, 63, 64, 65, 255, 256)
Z_NC = (0, 3)                                       # nc + Le takes every residue mod 4 and reaches 259
Z_N = 5


def z_grid():
    return [(lat, H, dk, Le, nc) for lat in Z_LAT for H, dk in Z_HEADS for Le in Z_LE for nc in Z_NC]


class ZCase:
    """The logical operands of one gct_attn_decode_z call (fp32 / uint8 / int32 CPU tensors, laid out tightly)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def reference(self, dtype=torch.float64):
        return latent_cross_attention(self.qf, self.q, self.z, self.ck, self.cv, self.valid, self.klen, self.scale, dtype)


def z_case(lat, H, dk, Le, nc, klen=None):
    """N(0,1) operands for Z_N = 5 samples.  klen = None, the masks of the grid: sample 0 sees every key, 1 has holes,
    2 a visible prefix of klen[2] keys (at least one latent row among them), 3 sees no key at klen = Lk (uniform
    weights), 4 has klen = Lk + 7 (clamped) -- klen is given for all five.  klen = an int: every sample sees that prefix.
    What the kernel must not read is NaN: the z rows at and behind klen - nc, the condition rows at and behind
    min(klen, nc), and without condition rows the plain queries."""
    Lk = nc + Le
    g = torch.Generator().manual_seed(((lat * 131 + H) * 263 + Le) * 2 + (nc > 0) + (0 if klen is None else 7919 * klen))
    qf, q = torch.randn(Z_N, H, lat, generator=g), torch.randn(Z_N, H, dk, generator=g)
    z = torch.randn(Z_N, Le, lat, generator=g)
    ck = torch.randn(Z_N, nc, H, dk, generator=g) if nc else None
    cv = torch.randn(Z_N, nc, H, dk, generator=g) if nc else None
    if klen is None:
        k2 = nc + 1 + int(torch.randint(0, Le, (1,), generator=g))
        kl = torch.tensor([Lk, Lk, k2, Lk, Lk + 7], dtype=torch.int32)
        valid = torch.ones(Z_N, Lk, dtype=torch.uint8)
        valid[1] = (torch.rand(Lk, generator=g) < 0.6).to(torch.uint8)
        valid[2, k2:] = 0
        valid[3] = 0
    else:
        kl = torch.full((Z_N,), klen, dtype=torch.int32)
        valid = (torch.arange(Lk)[None, :] < kl[:, None]).to(torch.uint8)
    for b in range(Z_N):
        L = min(int(kl[b]), Lk)
        z[b, max(L - nc, 0):] = NAN
        if nc:
            ck[b, min(L, nc):], cv[b, min(L, nc):] = NAN, NAN
    if not nc:
        q[:] = NAN
    return ZCase(lat=lat, H=H, dk=dk, Le=Le, nc=nc, qf=qf, q=q, z=z, ck=ck, cv=cv, valid=valid, klen=kl,
                 scale=float(np.float32(1.0 / math.sqrt(dk))))            # the argument is an fp32


def worst_ratio(got, want, tol=Z_TOL):
    """max |got - want| / (tol + tol |want|) over the elements; inf when got is not finite somewhere."""
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    if got.numel() == 0:
        return 0.0
    return float(((got - want).abs() / (tol + tol * want.abs())).max())


# ================================================================================================ gct_attn_decode_beam
def mapped_cache(kc, vc, valid, kv_src, Lold, knew, vnew, H, dk):
    """Keys, values and flags row b of gct_attn_decode_beam attends to: kc / vc [n, rows, >= H dk] and valid [n, > Lold]
    are the n physical rows, kv_src [n, >= Lold] the map, knew / vnew [n, >= H dk] this step's key / value.  Position
    j < Lold of row b comes from physical row kv_src[b, j] clamped to [0, n); position Lold is the step's own key and
    value with the flag valid[b, Lold] of row b ITSELF.  -> (keys, values fp64 [n, Lold + 1, H, dk], flags [n, Lold + 1]),
    the operands of decode_step_ref.cached_attention."""
    n, d = kc.shape[0], H * dk
    src = kv_src[:, :Lold].long().clamp(0, n - 1)
    j = torch.arange(Lold)[None, :]
    b = torch.arange(n)
    keys = torch.cat([kc[src, j, :d], knew[:, None, :d]], 1).double().reshape(n, Lold + 1, H, dk)
    vals = torch.cat([vc[src, j, :d], vnew[:, None, :d]], 1).double().reshape(n, Lold + 1, H, dk)
    flags = torch.cat([valid[src, j], valid[b, Lold][:, None]], 1)
    return keys, vals, flags


def mapped_attention(q, kc, vc, valid, kv_src, Lold, knew, vnew, H, dk, scale):
    keys, vals, flags = mapped_cache(kc, vc, valid, kv_src, Lold, knew, vnew, H, dk)
    return cached_attention(q[:, :H * dk].double().reshape(-1, H, dk), keys, vals, flags, scale)


BEAM_N, BEAM_H, BEAM_ROWS = 6, 2, 256
BEAM_LOLD = ((256, 0), (256, 1), (256, 63), (256, 64), (256, 65), (256, 254), (256, 255), (208, 207))   # (T, Lold)


class BeamCase:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def rows(self, t):
        """The n physical rows of an allocation with one guard row in front and one behind."""
        return t[1:BEAM_N + 1]


def beam_case(dk, Lold, T, kind, seed):
    """Operands of one gct_attn_decode_beam call for n = 6 rows of H = 2 heads.  qkv [n, 3 d + 4] is the fused step row;
    kc_all / vc_all [n + 2, 256, d + 8] and valid_all [n + 2, 264] are allocations whose rows 1 .. n are the physical
    rows: the guard rows 0 and n + 1 are NaN (flags: 0), and so is every cache position >= Lold of every row.  The
    flags are random per row (row 0: all set), row 1 masks its own new key and row 2 does not.  kv_src [n, T + 5]:
    kind "random": any ancestry, positions >= Lold included; "clamp": some positions < Lold hold -1 and n (the only
    out-of-range values: a missing clamp reads a guard row, not unallocated memory); "identity": kv_src[b, j] = b."""
    n, H = BEAM_N, BEAM_H
    d = H * dk
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * d + 4, generator=g)
    kc_all, vc_all = torch.randn(n + 2, BEAM_ROWS, d + 8, generator=g), torch.randn(n + 2, BEAM_ROWS, d + 8, generator=g)
    for t in (kc_all, vc_all):
        t[0], t[n + 1] = NAN, NAN
        t[:, Lold:] = NAN
    valid_all = (torch.rand(n + 2, BEAM_ROWS + 8, generator=g) < 0.7).to(torch.uint8)
    valid_all[0], valid_all[n + 1] = 0, 0
    valid_all[1] = 1
    if Lold < BEAM_ROWS:
        valid_all[2, Lold], valid_all[3, Lold] = 0, 1
    kv_src = torch.randint(0, n, (n, T + 5), generator=g).to(torch.int32)
    if kind == "identity":
        kv_src[:] = torch.arange(n, dtype=torch.int32)[:, None]
    elif kind == "clamp" and Lold > 0:
        out = torch.rand(n, Lold, generator=g)
        kv_src[:, :Lold][out < 0.2] = -1
        kv_src[:, :Lold][out > 0.8] = n
        kv_src[0, 0], kv_src[n - 1, Lold - 1] = n, -1
    return BeamCase(dk=dk, H=H, n=n, d=d, Lold=Lold, T=T, qkv=qkv, kc_all=kc_all, vc_all=vc_all, valid_all=valid_all,
                    kv_src=kv_src, scale=float(np.float32(1.0 / math.sqrt(dk))))


def beam_reference(c):
    d = c.d
    return mapped_attention(c.qkv, c.rows(c.kc_all), c.rows(c.vc_all), c.rows(c.valid_all), c.kv_src, c.Lold,
                            c.qkv[:, d:2 * d], c.qkv[:, 2 * d:3 * d], c.H, c.dk, c.scale)


# ================================================================================================ gct_stream_refill
def stream_refill_reference(s):
    """One gct_stream_refill call on a dict of CPU tensors (and ints for the geometry) under GctStreamState's field
    names (ckv / ckv_pool: lists of `layers` tensors), advanced in place; points 1-3 of the header comment.
    *enable == 0: nothing changes.  A row whose id lies outside [0, items) counts as empty.  next_item saturates at
    items; n_harvested accumulates; harvest / fresh (the scratch) hold every row's verdict of this call."""
    if int(s["enable"][0]) == 0:
        return
    R, N, W, T, off = s["rows"], s["items"], s["width"], s["T"], s["valid_off"]
    p = int(s["pos"][0])
    nxt, harvested = int(s["next_item"][0]), 0
    items, offs, done = s["item"].tolist(), s["row_off"].tolist(), s["done"].tolist()
    plen, limit = s["prefix_len"].tolist(), s["limit"].tolist()
    for r in range(R):
        it, finished = items[r], False
        empty = it < 0 or it >= N
        if not empty:
            gen = p - offs[r] + 2 - plen[it]                           # <= 0: still inside the prefix, never finished
            finished = gen > 0 and (done[r] != 0 or gen >= limit[it])
            if finished:                                               # 1. harvest
                s["out_ys"][it, :W] = s["ys"][r, :W]
                s["out_len"][it] = gen
                harvested += 1
        s["harvest"][r] = it if finished else -1
        s["fresh"][r] = 1 if (finished or empty) else 0
        if not (finished or empty):
            continue
        ni = -1                                                        # 2. the next item, in ascending row order
        if nxt < N:
            ni, nxt = nxt, nxt + 1
            s["row_of"][ni], s["start_step"][ni] = r, p + 1
        s["item"][r] = ni
        s["row_off"][r] = p + 1                                        # 3. lay the row out (a parked row: the offset only)
        if ni < 0:
            continue
        s["done"][r] = 0
        s["src_klen"][r] = s["klen_pool"][ni]
        s["ys"][r, :T] = s["pad_id"]
        s["ys"][r, :plen[ni]] = s["prefix_pool"][ni, :plen[ni]]
        s["valid"][r, off:off + T] = (s["ys"][r, :T] != s["pad_id"]).to(torch.uint8)
        s["src_valid"][r] = s["valid_pool"][ni]
        s["z3"][r] = s["z_pool"][ni]
        if s["ckv_row"] > 0:
            for l in range(s["layers"]):
                s["ckv"][l][r] = s["ckv_pool"][l][ni]
    s["next_item"][0] = min(nxt, N)
    s["n_harvested"][0] += harvested


MARGIN = 64                                          # sentinel elements in front of and behind every tensor
STREAM_GEOM = dict(ld_ys=18, valid_sb=21, valid_off=3, T=16, width=13, t0_max=5, pad_id=0)   # ld_ys > T > width > t0_max
STREAM_LAYOUTS = {                                   # z_row = Le lat: one thread / several trips of the 256-thread loop
    "small": dict(z_row=4, Lk=1, layers=0, ckv_row=0),
    "mid": dict(z_row=1040, Lk=259, layers=1, ckv_row=8),
    "wide": dict(z_row=4, Lk=259, layers=16, ckv_row=2048),
}
STREAM_GEOM_FIELDS = ("rows", "items", "ld_ys", "valid_sb", "valid_off", "T", "width", "t0_max", "z_row", "Lk", "ckv_row",
                      "layers", "pad_id")


def _pattern(shape, salt):
    """Distinct small integers as fp32 (cheap to make at any size, exact to compare)."""
    numel = int(np.prod(shape))
    return ((torch.arange(numel, dtype=torch.int64) * 7 + salt) % 8191).to(torch.float32).view(shape)


def same(a, b):
    """Tensors equal bit for bit (fp32: NaN payloads included)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def view_of(flat, shape):
    return flat[MARGIN:MARGIN + int(np.prod(shape))].view(shape)


def stream_alloc(R, N, layout, seed):
    """(geom, allocs): allocs[name] = (flat tensor, shape) -- every tensor of a GctStreamState (ckv<l> / ckv_pool<l> per
    layer) in the middle of an allocation filled with the tensor's sentinel, MARGIN elements on each side.  The row-side
    tensors and the results hold sentinels throughout (NaN for floats); the pools are filled: prefixes of random length
    1 .. t0_max over tokens 1 .. 49 with a <pad> inside some, right-padded; limit in [1, width - prefix_len]."""
    geom = dict(STREAM_GEOM, rows=R, items=N, **STREAM_LAYOUTS[layout])
    g = torch.Generator().manual_seed(seed)
    i32, i64, u8, f32 = torch.int32, torch.int64, torch.uint8, torch.float32
    spec = {
        "ys": ((R, geom["ld_ys"]), i64, -7), "valid": ((R, geom["valid_sb"]), u8, 9), "done": ((R,), u8, 5),
        "row_off": ((R,), i32, -77), "pos": ((1,), i32, -1), "z3": ((R, geom["z_row"]), f32, NAN),
        "src_valid": ((R, geom["Lk"]), u8, 9), "src_klen": ((R,), i32, -3), "item": ((R,), i32, -1),
        "harvest": ((R,), i32, -9), "fresh": ((R,), u8, 7),
        "z_pool": ((N, geom["z_row"]), f32, NAN), "valid_pool": ((N, geom["Lk"]), u8, 9), "klen_pool": ((N,), i32, -3),
        "prefix_pool": ((N, geom["t0_max"]), i64, -7), "prefix_len": ((N,), i32, -3), "limit": ((N,), i32, -3),
        "out_ys": ((N, geom["width"]), i64, -11), "out_len": ((N,), i32, -13), "row_of": ((N,), i32, -15),
        "start_step": ((N,), i32, -17), "next_item": ((1,), i32, 0), "n_harvested": ((1,), i32, 0),
        "enable": ((1,), i32, 1),
    }
    for l in range(geom["layers"]):
        spec[f"ckv{l}"] = ((R, geom["ckv_row"]), f32, NAN)
        spec[f"ckv_pool{l}"] = ((N, geom["ckv_row"]), f32, NAN)
    allocs = {}
    for name, (shape, dtype, fill) in spec.items():
        allocs[name] = (torch.full((int(np.prod(shape)) + 2 * MARGIN,), fill, dtype=dtype), shape)
    v = {name: view_of(*a) for name, a in allocs.items()}
    v["z_pool"][:] = _pattern(v["z_pool"].shape, 1)
    for l in range(geom["layers"]):
        v[f"ckv_pool{l}"][:] = _pattern(v[f"ckv_pool{l}"].shape, 100 + 37 * l)
    v["valid_pool"][:] = (torch.rand(v["valid_pool"].shape, generator=g) < 0.7).to(u8)
    v["klen_pool"][:] = torch.randint(1, geom["Lk"] + 1, (N,), generator=g).to(i32)
    plen = torch.randint(1, geom["t0_max"] + 1, (N,), generator=g)
    v["prefix_len"][:] = plen.to(i32)
    v["limit"][:] = (1 + (torch.rand(N, generator=g) * (geom["width"] - plen)).long()).clamp(max=geom["width"] - plen).to(i32)
    pre = torch.randint(1, 50, (N, geom["t0_max"]), generator=g)
    pre[torch.rand(N, geom["t0_max"], generator=g) < 0.15] = geom["pad_id"]          # a <pad> inside a prefix: flag 0
    pre[torch.arange(geom["t0_max"])[None, :] >= plen[:, None]] = geom["pad_id"]
    v["prefix_pool"][:] = pre
    return geom, allocs


def stream_state(geom, allocs):
    """The dict stream_refill_reference takes (and whose tensors ops.StreamState points to): views into the allocations
    (on whatever device they are) and the geometry."""
    v = {name: view_of(*a) for name, a in allocs.items()}
    s = {name: t for name, t in v.items() if not name.startswith("ckv")}
    s["ckv"] = [v[f"ckv{l}"] for l in range(geom["layers"])]
    s["ckv_pool"] = [v[f"ckv_pool{l}"] for l in range(geom["layers"])]
    s.update(geom)
    return s


STREAM_KINDS = ("at the limit", "one short", "parked", "id N", "id -5", "in the prefix, done set", "done")


def stream_midstream(R, layout, spare, seed):
    """A call in the middle of a stream: *pos = 9, n_harvested = 7, N = 2 R + 3 items of which the last `spare` are not
    handed out yet.  Row r is of kind STREAM_KINDS[r % 7]; a row that runs holds a distinct item below R, whose prefix
    length and limit fit the kind, at its own row_off (generated so far = 11 - row_off - prefix_len), with ys / valid
    filled as a run would have: so a wanting row takes an item only while the pool lasts, in row order."""
    N = 2 * R + 3
    geom, allocs = stream_alloc(R, N, layout, seed)
    s = stream_state(geom, allocs)
    g = torch.Generator().manual_seed(seed + 1)
    s["pos"][0], s["n_harvested"][0], s["next_item"][0] = 9, 7, N - spare
    holds = torch.randperm(R, generator=g).tolist()
    for r in range(R):
        kind = STREAM_KINDS[r % 7]
        if kind in ("parked", "id N", "id -5"):
            s["item"][r] = {"parked": -1, "id N": N, "id -5": -5}[kind]
            s["row_off"][r] = int(torch.randint(0, 10, (1,), generator=g))
            s["done"][r] = 1
            continue
        it = holds[r]
        plen = int(torch.randint(3 if kind.startswith("in the prefix") else 1, geom["t0_max"] + 1, (1,), generator=g))
        limit = int(torch.randint(2, 11 - plen + 1, (1,), generator=g))
        if kind == "at the limit":
            gen, done = limit, 0
        elif kind == "one short":
            gen, done = limit - 1, 0
        elif kind == "done":
            gen, done = int(torch.randint(1, limit, (1,), generator=g)), 1
        else:
            gen, done = int(torch.randint(-1, 1, (1,), generator=g)), 1
        s["item"][r], s["prefix_len"][it], s["limit"][it] = it, plen, limit
        s["row_off"][r], s["done"][r] = 11 - plen - gen, done
        s["prefix_pool"][it, plen:] = geom["pad_id"]
        s["ys"][r, :geom["T"]] = torch.randint(1, 50, (geom["T"],), generator=g)
        s["valid"][r, geom["valid_off"]:geom["valid_off"] + geom["T"]] = 1
    return geom, allocs


# ------------------------------------------------------------------------------------------------ a scripted stream
def stream_script(R, layout, seed):
    """The state in front of the first call of a whole stream without a model: N = 5 R + 3 items, item = -1, *pos = -1;
    and the items whose rows also raise `done` when they reach their cap (the cap is the limit either way)."""
    N = 5 * R + 3
    geom, allocs = stream_alloc(R, N, layout, seed)
    raises_done = torch.rand(N, generator=torch.Generator().manual_seed(seed + 2)) < 0.5
    return geom, allocs, raises_done


def script_step(s, raises_done):
    """What a decode step does to the rows between two refills, from the HOST state s (after *pos was advanced): every
    row that holds an item and is behind its prefix writes a token at column *pos - row_off + 1 (flag 1), and raises
    done when that was the item's last token and the item is one of raises_done.  -> index tensors for apply_step."""
    p = int(s["pos"][0])
    rows, cols, toks, dones = [], [], [], []
    items, offs = s["item"].tolist(), s["row_off"].tolist()
    plen, limit = s["prefix_len"].tolist(), s["limit"].tolist()
    for r, it in enumerate(items):
        col = p - offs[r] + 1
        if it < 0 or col < plen[it]:
            continue
        rows.append(r), cols.append(col), toks.append(1 + (it * 31 + col) % 49)
        if col + 1 - plen[it] == limit[it] and bool(raises_done[it]):
            dones.append(r)
    as_t = lambda x: torch.tensor(x, dtype=torch.int64)      # noqa: E731
    return as_t(rows), as_t(cols), as_t(toks), as_t(dones)


def apply_step(s, step):
    """The writes of script_step on a state on any device."""
    rows, cols, toks, dones = (t.to(s["ys"].device) for t in step)
    s["ys"][rows, cols] = toks
    s["valid"][rows, s["valid_off"] + cols] = 1
    s["done"][dones] = 1
