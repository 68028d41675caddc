"""tests/decode_aux_ref.py held to itself, and the inputs of tests/test_decode_aux_kernels_gpu.py shown to discriminate:
a plain fp32 evaluation of the latent cross-attention stays well inside the tolerance the kernel is held to, while a
kernel with one index space, the clamp, the scale or the mask off by a little would miss it a hundredfold on at least
one case; the single-call statement of the stream refill, driven without a model, gives the schedule
decode.stream_schedule_reference states.  No GPU, no library."""
import math

import pytest
import torch

from gct_plus_amd.decode import stream_schedule_reference
from tests import decode_aux_ref as A
from tests.decode_step_ref import cached_attention

NAN = float("nan")
SHORT = [dict(klen=2), dict(klen=3)]                 # the separate cases with nc = 3 (lat 16, 3 heads of 32, Le 5)


def all_z_cases():
    for args in A.z_grid():
        yield args, A.z_case(*args)
    for kw in SHORT:
        yield (16, 3, 32, 5, 3, kw["klen"]), A.z_case(16, 3, 32, 5, 3, **kw)


# ================================================================================================ latent cross-attention
def test_latent_cross_attention_against_a_loop():
    g = torch.Generator().manual_seed(2)
    n, H, dk, lat, Le, nc = 3, 2, 4, 8, 5, 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)        # noqa: E731
    qf, q, z, ck, cv = r(n, H, lat), r(n, H, dk), r(n, Le, lat), r(n, nc, H, dk), r(n, nc, H, dk)
    valid = torch.tensor([[1, 0, 1, 1, 0, 1, 1], [0] * 7, [1] * 7], dtype=torch.uint8)
    klen = torch.tensor([7, 7, 4])
    z[2, 2:] = NAN                                                          # behind klen - nc: never looked at
    ctx, cond = A.latent_cross_attention(qf, q, z, ck, cv, valid, klen, 0.5)
    for b in range(n):
        L = int(klen[b])
        for h in range(H):
            s = [float(q[b, h] @ ck[b, j, h]) if j < nc else float(qf[b, h] @ z[b, j - nc]) for j in range(L)]
            s = [t * 0.5 if valid[b, j] else -1e9 for j, t in enumerate(s)]
            e = [math.exp(t - max(s)) for t in s]
            want = sum(e[j] / sum(e) * z[b, j - nc] for j in range(nc, L))
            assert torch.allclose(ctx[b, h], want, rtol=1e-13, atol=1e-13)
            want = sum(e[j] / sum(e) * cv[b, j, h] for j in range(nc))
            assert torch.allclose(cond[b, h], want, rtol=1e-13, atol=1e-13)
    # all masked: uniform over the nc + Le keys, so ctx is the mean of the z rows scaled by Le / Lk
    assert torch.allclose(ctx[1], (z[1].mean(0) * Le / (nc + Le)).expand(H, lat), rtol=1e-13, atol=1e-13)
    ctx0, none = A.latent_cross_attention(qf[:2], None, z[:2], None, None, None, None, 0.5)
    assert none is None and ctx0.shape == (2, H, lat)


def test_grid_is_the_one_stated():
    grid = A.z_grid()
    assert len(grid) == 3 * 3 * 9 * 2 and len(set(grid)) == len(grid)
    assert {(a[3] + a[4]) % 4 for a in grid} == {0, 1, 2, 3} and max(a[3] + a[4] for a in grid) == 259
    for args in [(4, 2, 16, 1, 0), (16, 3, 32, 5, 3), (128, 8, 64, 256, 3)]:
        c = A.z_case(*args)
        Lk = c.Le + c.nc
        assert c.klen.tolist()[:2] == [Lk, Lk] and c.klen.tolist()[3:] == [Lk, Lk + 7]
        assert c.nc < int(c.klen[2]) <= Lk and int(c.valid[3].sum()) == 0 and int(c.valid[0].sum()) == Lk
        assert bool(c.z[2, int(c.klen[2]) - c.nc:].isnan().all()) and not bool(c.z[2, :int(c.klen[2]) - c.nc].isnan().any())
        assert bool(c.q.isnan().all()) == (c.nc == 0)
        ctx, cond = c.reference()
        mean = c.z[3].double().mean(0) * c.Le / Lk                          # no visible key at klen = Lk: uniform
        assert torch.allclose(ctx[3], mean.expand(c.H, c.lat), rtol=1e-12, atol=1e-12)
    c = A.z_case(16, 3, 32, 5, 3, klen=3)                                   # no latent row visible: ctx exactly 0
    ctx, cond = c.reference()
    assert bool((ctx == 0).all()) and bool(torch.isfinite(cond).all()) and bool(c.z.isnan().all())
    c = A.z_case(16, 3, 32, 5, 3, klen=2)
    assert bool(c.ck[:, 2:].isnan().all()) and bool((c.reference()[0] == 0).all())


def test_fp32_restatement_stays_inside_a_quarter_of_the_tolerance():
    worst = 0.0
    for args, c in all_z_cases():
        ctx64, cond64 = c.reference()
        ctx32, cond32 = c.reference(torch.float32)
        worst = max(worst, A.worst_ratio(ctx32, ctx64))
        if cond64 is not None:
            worst = max(worst, A.worst_ratio(cond32, cond64))
    print(f"fp32 restatement against fp64, worst error / (1e-5 + 1e-5 |ref|) over the grid: {worst:.3f}")
    assert worst <= 0.25


# ------------------------------------------------------------------------------------------------ mutants
def score_buffer_model(c, mutant=None):
    """The reference's operation restated with the kernel's three index spaces -- condition rows j, latent rows j, and
    per-head score rows of Lp = (Lk + 3) & ~3 entries in one flat buffer -- in fp64; `mutant` breaks one rule.  What
    lies behind a sample's rows (the next sample, a gap) reads as NaN, flags behind a row of flags as 1."""
    n, H, lat, Le, nc = A.Z_N, c.H, c.lat, c.Le, c.nc
    Lk = nc + Le
    Lp = (Lk + 3) & ~3
    far = Lk + 16
    scale = 1.0 if mutant == "scale dropped" else c.scale
    ctx, cond = torch.zeros(n, H, lat, dtype=torch.float64), torch.zeros(n, H, c.dk, dtype=torch.float64)
    for b in range(n):
        kl = int(c.klen[b]) + {"klen + 1": 1, "klen - 1": -1}.get(mutant, 0)
        Lvis = kl if mutant == "klen not clamped" else min(kl, Lk)
        ncv = min(nc, Lvis)
        nz = Lvis - ncv
        z = torch.full((far, lat), NAN, dtype=torch.float64)
        z[:Le] = c.z[b]
        vl = torch.ones(far, dtype=torch.uint8)
        vl[:Lk] = c.valid[b]
        wst = rst = Lp
        if mutant == "scores written at stride Lk, read at Lp":
            wst = Lk
        if mutant == "score rows of Lk & ~3 entries":
            wst = rst = Lk & ~3
        ps = torch.zeros(H * max(Lp, far) + far, dtype=torch.float64)
        swap = mutant == "condition and latent scores swapped"
        for h in range(H):
            sc = (z[:nz] @ c.qf[b, h].double()) * scale
            at = torch.arange(nz) + (0 if mutant == "mask at j" else ncv)
            sc = sc.masked_fill(vl[at] == 0, -1e9)
            lo = h * wst + (0 if swap else ncv)
            ps[lo:lo + nz] = sc
        for h in range(H):
            if ncv:
                sc = (c.ck[b, :ncv, h].double() @ c.q[b, h].double()) * scale
                sc = sc.masked_fill(vl[:ncv] == 0, -1e9)
                lo = h * wst + (nz if swap else 0)
                ps[lo:lo + ncv] = sc
        for h in range(H):
            ps[h * rst:h * rst + Lvis] = torch.softmax(ps[h * rst:h * rst + Lvis], 0)
        for h in range(H):
            ctx[b, h] = ps[h * rst + ncv:h * rst + ncv + nz] @ z[:nz]
            if ncv:
                cond[b, h] = ps[h * rst:h * rst + ncv] @ c.cv[b, :ncv, h].double()
    return ctx, (cond if nc else None)


Z_MUTANTS = ["klen + 1", "klen - 1", "klen not clamped", "scores written at stride Lk, read at Lp",
             "score rows of Lk & ~3 entries", "condition and latent scores swapped", "scale dropped", "mask at j"]


def separation(got, want):
    worst = A.worst_ratio(got[0], want[0])
    if want[1] is not None:
        worst = max(worst, A.worst_ratio(got[1], want[1]))
    return worst


def test_score_buffer_model_is_the_reference_and_its_mutants_are_not():
    """Without a mutant the restatement over the kernel's index spaces equals the reference to rounding on every case;
    every mutant differs from it by >= 100 x the tolerance on at least one case (NaN counts: it came from a row that
    must not be read).  lat = 128 adds nothing a mutant of the index spaces could hide behind: left out for time."""
    sep = dict.fromkeys(Z_MUTANTS, 0.0)
    hit = dict.fromkeys(Z_MUTANTS, 0)
    cases = 0
    for args, c in all_z_cases():
        if c.lat == 128:
            continue
        cases += 1
        want = c.reference()
        assert separation(score_buffer_model(c), want) < 1e-6, args
        for m in Z_MUTANTS:
            s = separation(score_buffer_model(c, m), want)
            sep[m] = max(sep[m], s)
            hit[m] += s >= 100
    for m in Z_MUTANTS:
        print(f"latent cross-attention mutant '{m}': worst separation {sep[m]:.3g} x tolerance, "
              f">= 100 x on {hit[m]} of {cases} cases")
        assert sep[m] >= 100, m


# ================================================================================================ the map
def mapped_mutant(c, mutant):
    """tests/decode_aux_ref.mapped_cache over the ALLOCATIONS (physical row r is allocation row r + 1, so an entry that
    is not clamped reads a guard row), with one rule broken."""
    n, H, dk, d, Lold = c.n, c.H, c.dk, c.d, c.Lold
    src = c.kv_src.long()
    if mutant == "map entry j + 1":
        src = src[:, 1:]
    src = src[:, :Lold]
    if mutant != "no clamp":
        src = src.clamp(0, n - 1)
    j = torch.arange(Lold)[None, :]
    b = torch.arange(n)
    own = c.kv_src[b, Lold].long().clamp(0, n - 1) if mutant == "own flag from the mapped row" else b
    flag_src = b[:, None].expand(n, Lold) if mutant == "flags from row b" else src
    keys = torch.cat([c.kc_all[src + 1, j, :d], c.qkv[:, None, d:2 * d]], 1).double().reshape(n, Lold + 1, H, dk)
    vals = torch.cat([c.vc_all[src + 1, j, :d], c.qkv[:, None, 2 * d:3 * d]], 1).double().reshape(n, Lold + 1, H, dk)
    flags = torch.cat([c.valid_all[flag_src + 1, j], c.valid_all[own + 1, Lold][:, None]], 1)
    return cached_attention(c.qkv[:, :d].double().reshape(n, H, dk), keys, vals, flags, c.scale)


MAP_MUTANTS = ["flags from row b", "own flag from the mapped row", "map entry j + 1", "no clamp"]


def beam_cases():
    for dk in (16, 32, 64):
        for i, (T, Lold) in enumerate(A.BEAM_LOLD):
            for kind in ("random", "clamp"):
                yield A.beam_case(dk, Lold, T, kind, seed=1000 * dk + 10 * i + (kind == "clamp"))


def test_mapped_reference_and_its_mutants():
    sep = dict.fromkeys(MAP_MUTANTS, 0.0)
    cases = 0
    for c in beam_cases():
        cases += 1
        want = A.beam_reference(c)
        assert bool(torch.isfinite(want).all())
        assert torch.equal(mapped_mutant(c, None), want)                    # the restatement over the allocations
        for m in MAP_MUTANTS:
            sep[m] = max(sep[m], A.worst_ratio(mapped_mutant(c, m), want))
    for m in MAP_MUTANTS:
        print(f"mapped attention mutant '{m}': worst separation {sep[m]:.3g} x tolerance over {cases} cases")
        assert sep[m] >= 100, m


def test_mapped_cache_rules():
    c = A.beam_case(16, 5, 256, "clamp", seed=3)
    assert int(c.kv_src[0, 0]) == c.n and int(c.kv_src[c.n - 1, 4]) == -1
    assert {-1, c.n} >= set(c.kv_src[:, :5].flatten().tolist()) - set(range(c.n))
    keys, vals, flags = A.mapped_cache(c.rows(c.kc_all), c.rows(c.vc_all), c.rows(c.valid_all), c.kv_src, 5,
                                       c.qkv[:, c.d:2 * c.d], c.qkv[:, 2 * c.d:3 * c.d], c.H, c.dk)
    assert torch.equal(keys[0, 0].flatten(), c.kc_all[c.n, 0, :c.d].double())          # n -> row n - 1
    assert torch.equal(vals[c.n - 1, 4].flatten(), c.vc_all[1, 4, :c.d].double())      # -1 -> row 0
    assert torch.equal(keys[:, 5].reshape(c.n, c.d), c.qkv[:, c.d:2 * c.d].double())   # the step's own key
    assert flags[:, 5].tolist() == c.rows(c.valid_all)[:, 5].tolist() and flags[1, 5] == 0 and flags[2, 5] == 1
    assert bool(c.kc_all[0].isnan().all()) and bool(c.kc_all[:, 5:].isnan().all()) and int(c.valid_all[c.n + 1].sum()) == 0


# ================================================================================================ the stream refill
def test_stream_refill_reference_single_call_rules():
    geom, allocs = A.stream_midstream(16, "mid", 3, seed=4)
    s = A.stream_state(geom, allocs)
    before = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.items() if k not in ("ckv", "ckv_pool")}
    N = geom["items"]
    s["enable"][0] = 0
    A.stream_refill_reference(s)
    assert all(A.same(s[k], v) for k, v in before.items() if isinstance(v, torch.Tensor) and k != "enable")
    s["enable"][0] = 1
    A.stream_refill_reference(s)
    wanting = [r for r in range(16) if A.STREAM_KINDS[r % 7] not in ("one short", "in the prefix, done set")]
    keeps = [r for r in range(16) if r not in wanting]
    assert s["fresh"].tolist() == [int(r in wanting) for r in range(16)]
    assert [int(s["item"][r]) for r in wanting[:3]] == [N - 3, N - 2, N - 1]           # ascending row order
    assert all(int(s["item"][r]) == -1 and int(s["row_off"][r]) == 10 for r in wanting[3:])
    assert all(int(s["item"][r]) == int(before["item"][r]) and int(s["row_off"][r]) == int(before["row_off"][r])
               and torch.equal(s["ys"][r], before["ys"][r]) for r in keeps)
    harvested = [r for r in range(16) if A.STREAM_KINDS[r % 7] in ("at the limit", "done")]
    assert int(s["n_harvested"][0]) == 7 + len(harvested) and int(s["next_item"][0]) == N
    for r in harvested:
        it = int(before["item"][r])
        assert int(s["harvest"][r]) == it and torch.equal(s["out_ys"][it], before["ys"][r, :geom["width"]])
        assert int(s["out_len"][it]) == 11 - int(before["row_off"][r]) - int(s["prefix_len"][it])
    r, it = wanting[0], N - 3
    plen = int(s["prefix_len"][it])
    assert torch.equal(s["ys"][r, :plen], s["prefix_pool"][it, :plen]) and bool((s["ys"][r, plen:16] == 0).all())
    assert bool((s["ys"][r, 16:] == before["ys"][r, 16:]).all())                       # behind T: left alone
    assert torch.equal(s["valid"][r, 3:19], (s["ys"][r, :16] != 0).to(torch.uint8)) and int(s["done"][r]) == 0
    assert torch.equal(s["z3"][r], s["z_pool"][it]) and torch.equal(s["ckv"][0][r], s["ckv_pool"][0][it])
    assert int(s["row_of"][it]) == r and int(s["start_step"][it]) == 10 and int(s["src_klen"][r]) == int(s["klen_pool"][it])


def run_script(R, layout, seed):
    """The scripted stream on the host -> (state, makespan)."""
    geom, allocs, raises_done = A.stream_script(R, layout, seed)
    s = A.stream_state(geom, allocs)
    A.stream_refill_reference(s)
    step = 0
    while int(s["n_harvested"][0]) < geom["items"]:
        assert step < 10000
        s["pos"][0] = step
        A.apply_step(s, A.script_step(s, raises_done))
        A.stream_refill_reference(s)
        step += 1
    return s, step


@pytest.mark.parametrize("R", [3, 8])
def test_scripted_stream_follows_the_schedule(R):
    s, makespan = run_script(R, "small", seed=10 + R)
    N = 5 * R + 3
    assert s["items"] == N
    plen, limit = s["prefix_len"].long(), s["limit"].long()
    row_of, start, span = stream_schedule_reference(plen + limit - 1, R)
    assert torch.equal(s["row_of"].long(), row_of) and torch.equal(s["start_step"].long(), start) and makespan == span
    assert torch.equal(s["out_len"].long(), limit)
    assert int(s["next_item"][0]) == N and bool((s["item"] == -1).all())
    for it in range(N):                                                     # the prefix, then the tokens of the script
        p, g = int(plen[it]), int(limit[it])
        want = s["prefix_pool"][it, :p].tolist() + [1 + (it * 31 + c) % 49 for c in range(p, p + g)]
        assert s["out_ys"][it, :p + g].tolist() == want and bool((s["out_ys"][it, p + g:] == 0).all())
