"""Host reference of the row maps of csrc/liverows.hip (gct_live_rows / gct_key_rows): plain torch on the CPU, nothing
from the GPU side.  The device kernels are compared with this, integer for integer (tests/test_row_maps_gpu.py); the
reference itself is held to the contract of the maps in tests/test_row_maps_host.py.

The rules, from the top of liverows.hip:
  live[b,t]   the row has a non-zero element (key side: the key is visible)
  violation   per sample: a dead key visible to a live query; or a live row that sees no key while a dead row exists;
              or mask=None with live and dead rows side by side
  non-prefix  per sample: a dead row directly in front of a live one
  quads       aligned groups of 4 rows of the flat [B*T] row space; quad_list = the quads that hold a live row,
              ascending, padded with -1 to a multiple of 32 quads; Mc = 4 * padded quads
  cstart[b]   compact row of (b, 0): 4 * (live quads in front of the quad of row b*T) + (b*T & 3) when that quad is
              live, and without the offset when it is dead (a sample without a live row): never decreasing
  tiles       32-row tiles that hold a live row -- every tile when a sample violates
"""
import torch


def _mask3(mask, B, T):
    """None | [B,T] (key padding) | [B,T,T] -> bool [B,T,T] (query, key)."""
    if mask is None:
        return None
    m = torch.as_tensor(mask) != 0
    if m.numel() == B * T and m.dim() <= 2:
        return m.reshape(B, 1, T).expand(B, T, T)
    return m.reshape(B, T, T)


def row_plan_reference(live, mask=None, key_side=False):
    """live [B,T] bool (key side: the key-padding mask != 0); mask: the self-attention mask the live rows are checked
    against (ignored on the key side).  Returns a dict of everything the device emits."""
    live = torch.as_tensor(live) != 0
    B, T = live.shape
    M = B * T
    rows = live.tolist()                                   # plain lists: the maps are integer bookkeeping
    flat = [x for r in rows for x in r]
    n_list = [sum(r) for r in rows]
    viol = nonpre = empty = 0
    m3 = None if key_side else _mask3(mask, B, T)
    for b in range(B):
        r = rows[b]
        if any((not r[t]) and r[t + 1] for t in range(T - 1)):
            nonpre += 1
        if key_side:
            empty += int(not any(r))
            continue
        anyl, anyd = any(r), not all(r)
        if m3 is None:
            viol += int(anyl and anyd)
            continue
        lv, mb = live[b], m3[b]
        bad = bool((lv[:, None] & ~lv[None, :] & mb).any())            # live query i, dead key j, visible
        if anyd and bool((lv & ~mb.any(1)).any()):                     # a live row without a key, next to a dead row
            bad = True
        viol += int(bad)
    Q = (M + 3) // 4
    qlive = [any(flat[4 * q:4 * q + 4]) for q in range(Q)]
    quads = [q for q in range(Q) if qlive[q]]
    total = len(quads)
    padded = (total + 31) // 32 * 32
    rank, seen = [], 0                                     # live quads in front of quad q
    for q in range(Q):
        rank.append(seen)
        seen += int(qlive[q])
    cs = []
    for b in range(B):
        q = (b * T) >> 2
        cs.append(4 * rank[q] + ((b * T) & 3 if qlive[q] else 0))
    n_b = torch.tensor(n_list, dtype=torch.int64)
    quad_list = torch.tensor(quads + [-1] * (padded - total), dtype=torch.int64)
    cstart = torch.tensor(cs, dtype=torch.int64)
    tile_list = None
    ntile = 0
    if not key_side:
        nt = (M + 31) // 32
        tiles = [t for t in range(nt) if viol or any(flat[32 * t:32 * t + 32])]
        tile_list = torch.tensor(tiles, dtype=torch.int64)
        ntile = len(tiles)
    info = [sum(n_list), viol, nonpre, ntile, 4 * padded, total, empty, 0]
    return dict(B=B, T=T, M=M, live=live.clone(), n_b=n_b, quad_list=quad_list, cstart=cstart, Mc=4 * padded,
                info=info, tile_list=tile_list, usable=(viol == 0 and nonpre == 0))


def compact_rows(plan):
    """(orig, prefix): orig[Mc] = the original row of every compact row, or -1 (padding quads, rows past M);
    prefix[Mc] bool = the compact row lies in some sample's live prefix [cstart[b], cstart[b] + n_b[b])."""
    Mc, M = plan["Mc"], plan["M"]
    ql = plan["quad_list"]
    orig = (4 * ql[:, None] + torch.arange(4)[None, :]).reshape(-1)
    orig = torch.where((ql[:, None].expand(-1, 4).reshape(-1) < 0) | (orig >= M), torch.full_like(orig, -1), orig)
    prefix = torch.zeros(Mc, dtype=torch.bool)
    for b in range(plan["B"]):
        c, n = int(plan["cstart"][b]), int(plan["n_b"][b])
        prefix[c:c + n] = True
    return orig, prefix


def gap_rows(plan, nrows):
    """bool [nrows]: the rows gct_zero_gap_rows must zero = [0, nrows) outside every live prefix."""
    _, prefix = compact_rows(plan)
    out = torch.ones(nrows, dtype=torch.bool)
    n = min(nrows, plan["Mc"])
    out[:n] = ~prefix[:n]
    return out


def prefix_live(B, T, lengths):
    return torch.arange(T)[None, :] < torch.as_tensor(lengths).reshape(B, 1)


def causal_pad_mask(B, T, lengths):
    """uint8 [B,T,T]: key j visible to query i <=> j <= i and j < lengths[b] (the decoder's mask for right-padded rows)."""
    pad = prefix_live(B, T, lengths)
    return (pad[:, None, :] & torch.tril(torch.ones(T, T, dtype=torch.bool))[None]).to(torch.uint8)


def random_plans(seed=20240607, count=60):
    """The plans of the device tests: (name, live [B,T] bool, mask | None).  Five kinds in turn: three usable ones
    (prefix rows under the causal-and-padding mask, under the key-padding mask, and all-or-nothing samples without a
    mask), a violating one (a key-padding mask that shows dead keys to the live queries) and a non-prefix one (random rows).  Lengths are
    drawn from {0, T, uniform}, so empty and full samples are frequent."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))                           # noqa: E731
    out = []
    for i in range(count):
        B, T = ri(1, 6), ri(1, 40)
        kind = i % 6

        def lengths():
            return [(0, T, ri(0, T), ri(1, T))[ri(0, 3)] for _ in range(B)]

        if kind in (0, 3):
            n = lengths()
            out.append((f"causal{i}", prefix_live(B, T, n), causal_pad_mask(B, T, n)))
        elif kind == 1:
            n = lengths()
            out.append((f"keypad{i}", prefix_live(B, T, n), prefix_live(B, T, n).to(torch.uint8)))
        elif kind == 2:
            n = [(0, T)[ri(0, 1)] for _ in range(B)]
            out.append((f"nomask{i}", prefix_live(B, T, n), None))
        elif kind == 4:
            n = lengths()
            seen = [min(T, x + ri(1, 3)) for x in n]                  # the mask shows up to 3 keys more than are live
            out.append((f"violate{i}", prefix_live(B, T, n), prefix_live(B, T, seen).to(torch.uint8)))
        else:
            lv = torch.rand(B, T, generator=g) < 0.5
            out.append((f"random{i}", lv, lv[:, None, :].expand(B, T, T).to(torch.uint8).contiguous()))
    return out
