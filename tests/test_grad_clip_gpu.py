"""Global gradient-norm clipping on the device: gct_grad_norm against the fp64 rule (tests/test_grad_clip_host.
clip_reference), its counters, gct_adam_step with that state against the fp64 Adam rule of
tests/test_loss_optim_edges_gpu.py and bit for bit against gct_adam_step without one where nothing needs clipping, the
non-finite skip, FusedAdam(max_grad_norm=...) on the tiny model against torch's clip_grad_norm_ + Adam in fp64,
reinforce_step / ppo_update with and without the argument, and two data-parallel ranks.

Tolerances.  The kernel accumulates in fp64 from the first product on, so the one rounding that matters is the final one
to fp32, 2^-24; norm and coef are held to 2^-22 relative (the rest is margin).  The Adam outputs take the tolerances of
tests/test_loss_optim_edges_gpu.py: p 1e-7 / 1e-6, m 1e-7 / 1e-5, v 1e-9 / 1e-5 (absolute / relative)."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gct_plus_amd.ops import GRAD_NORM_MAX_GRID
from tests.test_dp_gpu import _build as dp_build, _port, _step_fn
from tests.test_grad_clip_host import (CLIPPED_STEPS, COEF, LARGEST, NONFINITE, NONFINITE_STEPS, NORM, RESERVED, STEPS,
                                       clip_reference)
from tests.test_loss_optim_edges_gpu import B1, B2, EPS, LR, _adam_reference, ratio
from tests.test_model_gpu import PAD, build, run_fwd_loss, set_eps

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 2.0 ** -22
FB1, FB2 = (float(torch.tensor(b, dtype=torch.float32)) for b in (B1, B2))


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def spread(n, seed):
    """n fp32 values of magnitude 1e-12 .. 1e3 (log-uniform) with random signs."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * 15 - 12)
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (mag * sign).float()


def words(state):
    """(the 8 words as floats, the 8 words as int32) on the host."""
    host = state.cpu()
    return host.tolist(), host.view(torch.int32).tolist()


def run_norm(ops, g, max_norm, gscale=1.0, state=None):
    gd = g.to(DEV)
    state = ops.new_clip_state(gd.device) if state is None else state
    ops.grad_norm(gd, state, ops.grad_norm_ws(gd.numel(), gd.device), max_norm, gscale)
    return state


# ------------------------------------------------------------------------------------------------- 1. gct_grad_norm
SWEEP = GRAD_NORM_MAX_GRID * 256 * 4                   # elements of one trip of the capped grid, one float4 per lane


# 4 sweeps + 7: each lane's four loads in flight once, then one float4 and a scalar tail of 3 behind them
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 1025, SWEEP + 7, 4 * SWEEP + 7])
def test_norm_against_fp64(ops, n, gscale):
    g = spread(n, seed=n % 1000 + 1)
    norm, _, bad = clip_reference(g, gscale, 1.0)
    assert not bad
    max_norm = 0.5 * norm if n else 1.0                # clips, except for the empty buffer
    _, coef, _ = clip_reference(g, gscale, max_norm)
    runs = [words(run_norm(ops, g, max_norm, gscale)) for _ in range(2)]
    assert runs[0] == runs[1], "the same buffer twice: different state words"
    f, i = runs[0]
    print(f"n={n} gscale={gscale}: norm {f[NORM]!r} (fp64 {norm!r}), coef {f[COEF]!r} (fp64 {coef!r})")
    if n == 0:
        assert f[NORM] == 0.0 and f[COEF] == 1.0
    assert abs(f[NORM] - norm) <= TOL * norm
    assert abs(f[COEF] - coef) <= TOL * coef
    assert (i[NONFINITE], i[STEPS], i[CLIPPED_STEPS], i[NONFINITE_STEPS], i[RESERVED]) == (0, 1, int(n > 0), 0, 0)
    assert f[LARGEST] == f[NORM]


def test_the_slab_is_sized_by_the_capped_grid(ops):
    L = ops._L()
    assert L.gct_grad_norm_ws_bytes(0) == 16 and L.gct_grad_norm_ws_bytes(5) == 16
    assert L.gct_grad_norm_ws_bytes(257 * 4) == 16 and L.gct_grad_norm_ws_bytes(513 * 4) == 32   # 2 and 3 workgroups
    assert L.gct_grad_norm_ws_bytes(SWEEP) == 8 * GRAD_NORM_MAX_GRID == L.gct_grad_norm_ws_bytes(100 * SWEEP)
    g = torch.zeros(4096, device=DEV)
    with pytest.raises(ValueError, match="ws"):
        ops.grad_norm(g, ops.new_clip_state(g.device), torch.empty(1, dtype=torch.float64, device=DEV), 1.0)
    with pytest.raises(Exception, match="max_norm"):
        ops.grad_norm(g, ops.new_clip_state(g.device), ops.grad_norm_ws(4096, g.device), 0.0)


@pytest.mark.parametrize("factor", [0.01, 0.5, 0.999, 1.001, 2.0, 1e6])
def test_coef(ops, factor):
    """Within 2^-22 of the fp64 rule when clipping; exactly 1.0 when norm + 1e-6 lies below max_norm by more than that."""
    g = spread(10007, seed=3)
    norm, _, _ = clip_reference(g, 0.25, 1.0)
    max_norm = float(torch.tensor(factor * norm, dtype=torch.float32))
    _, coef, _ = clip_reference(g, 0.25, max_norm)
    f, i = words(run_norm(ops, g, max_norm, 0.25))
    print(f"max_norm = {factor} x norm: coef {f[COEF]!r} (fp64 {coef!r})")
    if norm + 1e-6 < max_norm * (1 - TOL):
        assert f[COEF] == 1.0 and i[CLIPPED_STEPS] == 0
    else:
        assert coef < 1 - TOL and abs(f[COEF] - coef) <= TOL * coef and i[CLIPPED_STEPS] == 1


def test_counters_over_a_sequence_of_steps(ops):
    g = spread(1025, seed=5)
    norm, _, _ = clip_reference(g, 1.0, 1.0)
    inf, nan = g.clone(), g.clone()
    inf[1000], nan[1024] = float("inf"), float("nan")
    huge = torch.full((1025,), 3e38)                   # finite elements, a norm beyond fp32: counts as non-finite
    state = ops.new_clip_state(torch.zeros(1, device=DEV).device)
    seq = [(g, 0.5 * norm), (g, 2 * norm), (inf, 1.0), (3 * g, norm), (nan, 1.0), (huge, 1.0), (0.5 * g, norm)]
    for buf, max_norm in seq:
        run_norm(ops, buf, max_norm, state=state)
    f, i = words(state)
    assert (i[STEPS], i[CLIPPED_STEPS], i[NONFINITE_STEPS], i[NONFINITE]) == (7, 2, 3, 0)
    assert abs(f[LARGEST] - 3 * norm) <= TOL * 3 * norm and f[COEF] == 1.0 and abs(f[NORM] - 0.5 * norm) <= TOL * norm
    run_norm(ops, inf, 1.0, state=state)               # the latest step's words when it is the non-finite one
    f, i = words(state)
    assert f[NORM] == float("inf") and f[COEF] == 0.0 and i[NONFINITE] == 1 and i[NONFINITE_STEPS] == 4


# --------------------------------------------------------------------------------- 2. gct_adam_step with a clip state
def clipped_adam_run(ops, p, g, m, v, steps, gscale, max_norm, what):
    pg, mg, vg, gg = p.to(DEV).clone(), m.to(DEV).clone(), v.to(DEV).clone(), g.to(DEV)
    state = ops.new_clip_state(gg.device)
    ws = ops.grad_norm_ws(gg.numel(), gg.device)
    worst = 0.0
    for step in steps:
        ops.grad_norm(gg, state, ws, max_norm, gscale)
        coef = words(state)[0][COEF]
        assert 0 < coef < 1, (what, coef)
        scale = float(torch.tensor(gscale, dtype=torch.float32)) * coef
        # the reference restarts from the device's state: one step's error, not the accumulated drift
        ref = _adam_reference(pg.cpu(), g, mg.cpu(), vg.cpu(), LR, B1, B2, EPS, step, scale)
        ops.adam_step(pg, gg, mg, vg, LR, B1, B2, EPS, step, gscale=gscale, guard=False, clip_state=state)
        worst = max(worst, ratio(pg, ref[0], 1e-7, 1e-6, f"clipped adam p {what} step={step}"),
                    ratio(mg, ref[1], 1e-7, 1e-5, f"clipped adam m {what} step={step}"),
                    ratio(vg, ref[2], 1e-9, 1e-5, f"clipped adam v {what} step={step}"))
    return worst


def rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("n", [1, 5, 10007])
def test_clipped_adam_against_the_fp64_rule(ops, n):
    p, g = rnd(n, 1), rnd(n, 2)
    max_norm = 0.5 * clip_reference(g, 0.25, 1.0)[0]
    z = torch.zeros(n)
    w1 = clipped_adam_run(ops, p, g, z, z, (1, 2, 3), 0.25, max_norm, f"n={n} cold")
    w2 = clipped_adam_run(ops, p, g, rnd(n, 3, 0.1), rnd(n, 4).square() * 0.01, (20000,), 0.25, max_norm, f"n={n} warm")
    print(f"clipped adam n={n}: worst error / tolerance {max(w1, w2):.3f}")


@pytest.mark.parametrize("n", [1, 5, 10007])
def test_a_step_that_needs_no_clipping_is_the_unclipped_step_bit_for_bit(ops, n):
    g = rnd(n, 2).to(DEV)
    runs = []
    for clipped in (False, True):
        p, m, v = rnd(n, 1).to(DEV), rnd(n, 3, 0.1).to(DEV), (rnd(n, 4).square() * 0.01).to(DEV)
        state = ops.new_clip_state(g.device) if clipped else None
        for step in (1, 2, 20000):
            if clipped:
                ops.grad_norm(g, state, ops.grad_norm_ws(n, g.device), 1e6, 0.25)
            ops.adam_step(p, g, m, v, LR, B1, B2, EPS, step, gscale=0.25, guard=False, clip_state=state)
        runs.append((p, m, v))
    assert words(state)[0][COEF] == 1.0 and words(state)[1][CLIPPED_STEPS] == 0
    for a, b, name in zip(runs[0], runs[1], "pmv"):
        assert torch.equal(a, b), f"{name}: coef == 1 changed the update"


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step_on_the_device(ops, poison):
    n = 10007
    g = rnd(n, 2)
    bad = g.clone()
    bad[n - 2] = poison
    p, m, v = rnd(n, 1).to(DEV), rnd(n, 3, 0.1).to(DEV), (rnd(n, 4).square() * 0.01).to(DEV)
    before = [t.clone() for t in (p, m, v)]
    state = ops.new_clip_state(p.device)
    ws = ops.grad_norm_ws(n, p.device)
    ops.grad_norm(bad.to(DEV), state, ws, 1.0)
    ops.adam_step(p, bad.to(DEV), m, v, LR, B1, B2, EPS, 7, guard=False, clip_state=state)
    for a, b, name in zip((p, m, v), before, "pmv"):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name} changed under a non-finite norm"
    f, i = words(state)
    assert i[NONFINITE] == 1 and i[NONFINITE_STEPS] == 1 and i[STEPS] == 1 and f[COEF] == 0.0
    # the following finite step updates as usual
    max_norm = 0.5 * clip_reference(g, 1.0, 1.0)[0]
    ops.grad_norm(g.to(DEV), state, ws, max_norm)
    f, i = words(state)
    assert i[NONFINITE] == 0 and i[NONFINITE_STEPS] == 1 and i[STEPS] == 2 and 0 < f[COEF] < 1
    ref = _adam_reference(p.cpu(), g, m.cpu(), v.cpu(), LR, B1, B2, EPS, 8, f[COEF])
    ops.adam_step(p, g.to(DEV), m, v, LR, B1, B2, EPS, 8, guard=False, clip_state=state)
    ratio(p, ref[0], 1e-7, 1e-6, "p after the skip")
    ratio(m, ref[1], 1e-7, 1e-5, "m after the skip")
    ratio(v, ref[2], 1e-9, 1e-5, "v after the skip")
    assert not torch.equal(p, before[0])


# ------------------------------------------------------------------------------------------------ 3. the tiny model
MTYPE = "pscavaetf"


def model_batches(steps):
    from gct_plus_amd import synthetic
    nc = synthetic.n_conds(MTYPE)
    out = []
    for s in range(steps):
        ds = synthetic.make_dataset(6, max_len=24, model_type=MTYPE, seed=90 + s)
        eps = torch.randn(6, 24 + nc, 16, generator=torch.Generator().manual_seed(s))
        out.append((ds, eps))
    return out


def backward(model, ds, eps, opt, per_token=True):
    """per_token: the trainer's loss per target token -- the gradient entries are then of order 1 and below, the
    magnitudes the absolute parts of the Adam tolerances were written for (see the tests below); else its sum loss."""
    set_eps(model, eps)
    opt.zero_grad(set_to_none=True)
    tokens = int((ds["trg"][:, 1:] != PAD).sum()) if per_token else 1
    (run_fwd_loss(model, MTYPE, ds, 0.1)[5] / tokens).backward()


def within(got, ref, bound, what):
    """max |got - ref| / bound elementwise (bound > 0); asserts <= 1."""
    err = (got.detach().cpu().double() - ref).abs()
    r = float((err / bound).max())
    assert r <= 1.0, f"{what}: error {r:.3f} x bound (max err {float(err.max()):.3e})"
    return r


def test_fused_adam_with_max_grad_norm_on_the_tiny_model():
    three_clipped_steps(per_token=True)


def test_fused_adam_with_max_grad_norm_at_the_trainers_gradient_magnitudes():
    """The same three steps on the trainer's SUM loss, where the absolute parts of the tolerances above mean nothing for
    the moments.  p keeps its tolerance (1e-7 / 1e-6: Adam's update does not scale with the gradient).  m and v are held
    to the roundings of their own operands, elementwise, against a reference that takes the fp32 values of the betas:
    |dm| <= 5 * 2^-24 * (b1 |m| + (1 - b1) |g coef|) -- max_norm and coef rounded to fp32, g * coef, the product with
    1 - b1 and the fma -- and |dv| <= 8 * 2^-24 * (b2 v + (1 - b2) (g coef)^2): the three roundings of g coef twice for
    the square, the product with 1 - b2 and the fma."""
    three_clipped_steps(per_token=False)


def three_clipped_steps(per_token):
    """Three steps, every one clipped (c = half the first step's norm); after each the parameters and moments against
    torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in fp64 on the CPU, restarted from the device's state before the
    step and fed the device's gradients of that step.

    per_token: the loss is the trainer's divided by the batch's target tokens, and the tolerances (p 1e-7 / 1e-6,
    m 1e-7 / 1e-5, v 1e-9 / 1e-5) are those of the kernel tests, whose gradients are of order 1: an absolute 1e-7 is about one fp32
    ulp of 1.  The trainer's SUM loss gives this batch first moments up to 7.7 after two steps, and where b1 * m and
    (1 - b1) * g * coef cancel, fp32 cannot hold m to 1e-7 (an ulp of 4 is 4.8e-7): measured with the sum loss, step 2,
    m of encoder.embed_sentence.embed.weight: error 1.14e-6 at a reference scale of 7.7, 1.49 x the tolerance (the
    first miss; step 1 passed).  That is the arithmetic of fp32, the same in the unclipped kernel.  Not per_token: the
    sum loss, with m and v held to the operand-scaled bounds of the second test above instead.

    lr = 1e-4, the trainer's default: at 1e-3 the first steps from a fresh initialisation halve the gradient norm each
    (12.6, 6.8, 4.1 measured), and a bound of half the FIRST norm then no longer clips the third."""
    from gct_plus_amd.optim import FusedAdam
    batches = model_batches(3)
    probe = build(MTYPE).train()
    probe_opt = FusedAdam(probe.parameters(), lr=LR, betas=(B1, B2), eps=EPS, model=probe)
    backward(probe, *batches[0], probe_opt, per_token)
    probe.sync_grads_to_flat()
    c = 0.5 * float(probe.flat_grads().double().norm())
    assert c > 0

    model = build(MTYPE).train()
    opt = FusedAdam(model.parameters(), lr=LR, betas=(B1, B2), eps=EPS, model=model, max_grad_norm=c)
    names = [k for k, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    norms = []
    for t, (ds, eps) in enumerate(batches, start=1):
        backward(model, ds, eps, opt, per_token)
        cpu = [torch.nn.Parameter(p.detach().cpu().double()) for p in params]
        for q, p in zip(cpu, params):
            q.grad = torch.zeros_like(q) if p.grad is None else p.grad.detach().cpu().double()
        ref = torch.optim.Adam(cpu, lr=LR, betas=(FB1, FB2), eps=EPS)    # the betas the kernel is given: fp32 values
        for q, p in zip(cpu, params):
            st = opt.state.get(p, {})
            ref.state[q] = dict(step=torch.tensor(float(t - 1)),
                                exp_avg=st["exp_avg"].detach().cpu().double() if "exp_avg" in st else torch.zeros_like(q),
                                exp_avg_sq=(st["exp_avg_sq"].detach().cpu().double() if "exp_avg_sq" in st
                                            else torch.zeros_like(q)))
        norms.append(float(torch.nn.utils.clip_grad_norm_(cpu, c)))          # q.grad is g * coef from here on
        u = 2.0 ** -24
        bound_m = [5 * u * (FB1 * ref.state[q]["exp_avg"].abs() + (1 - FB1) * q.grad.abs()) + 1e-30 for q in cpu]
        bound_v = [8 * u * (FB2 * ref.state[q]["exp_avg_sq"] + (1 - FB2) * q.grad.square()) + 1e-30 for q in cpu]
        ref.step()
        opt.step()
        stats = opt.grad_norm_stats()
        assert abs(stats["norm"] - norms[-1]) <= TOL * norms[-1], (t, stats, norms[-1])
        print(f"step {t}: norm {norms[-1]:.6f} against c = {c:.6f}")
        assert abs(stats["coef"] - min(1.0, c / (norms[-1] + 1e-6))) <= TOL
        worst = 0.0
        for k, q, p, bm, bv in zip(names, cpu, params, bound_m, bound_v):
            worst = max(worst, ratio(p, q, 1e-7, 1e-6, f"step {t} p {k}"))
            dm, dv, rm, rv = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"]
            if per_token:
                worst = max(worst, ratio(dm, rm, 1e-7, 1e-5, f"step {t} m {k}"), ratio(dv, rv, 1e-9, 1e-5, f"step {t} v {k}"))
            else:
                worst = max(worst, within(dm, rm.detach(), bm, f"step {t} m {k}"), within(dv, rv.detach(), bv, f"step {t} v {k}"))
        print(f"step {t}: norm {norms[-1]:.6f}, coef {stats['coef']:.6f}, worst error / tolerance {worst:.3f}")
    stats = opt.grad_norm_stats(reset=True)
    assert (stats["steps"], stats["clipped_steps"], stats["nonfinite_steps"]) == (3, 3, 0)
    assert abs(stats["max_norm"] - max(norms)) <= TOL * max(norms)
    again = opt.grad_norm_stats()
    assert (again["steps"], again["clipped_steps"], again["max_norm"]) == (0, 0, 0.0) and again["norm"] == stats["norm"]
    # the checkpoint layout is torch Adam's, with or without the setting
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd["param_groups"][0]
    stock = torch.optim.Adam(model.parameters(), lr=LR, betas=(B1, B2), eps=EPS)
    stock.load_state_dict(sd)
    assert torch.equal(stock.state[params[0]]["exp_avg"], opt.state[params[0]]["exp_avg"])


def test_the_generic_path_writes_the_same_state():
    """A FusedAdam without a flat model (one launch per tensor): the state comes from torch ops, the update from the
    clipped kernel."""
    from gct_plus_amd.optim import FusedAdam
    shapes = [(5,), (33, 7), (1,)]
    ps = [torch.nn.Parameter(rnd(math.prod(s), 10 + i).view(s).to(DEV)) for i, s in enumerate(shapes)]
    gs = [rnd(p.numel(), 20 + i).view(p.shape) for i, p in enumerate(ps)]
    flat = torch.cat([g.view(-1) for g in gs])
    max_norm = 0.5 * clip_reference(flat, 1.0, 1.0)[0]
    opt = FusedAdam(ps, lr=LR, betas=(B1, B2), eps=EPS, max_grad_norm=max_norm)
    start = [p.detach().cpu() for p in ps]
    for p, g in zip(ps, gs):
        p.grad = g.to(DEV)
    opt.step()
    norm, coef, _ = clip_reference(flat, 1.0, max_norm)
    stats = opt.grad_norm_stats()
    assert abs(stats["norm"] - norm) <= TOL * norm and abs(stats["coef"] - coef) <= TOL * coef
    assert (stats["steps"], stats["clipped_steps"], stats["nonfinite_steps"]) == (1, 1, 0)
    for p, p0, g in zip(ps, start, gs):
        ref = _adam_reference(p0.view(-1), g.view(-1), torch.zeros(g.numel()), torch.zeros(g.numel()), LR, B1, B2, EPS, 1,
                              stats["coef"])
        ratio(p.view(-1), ref[0], 1e-7, 1e-6, "generic p")
    ps[1].grad[3, 3] = float("nan")
    before = [p.detach().clone() for p in ps]
    opt.step()
    stats = opt.grad_norm_stats()
    assert (stats["steps"], stats["nonfinite_steps"], stats["coef"]) == (2, 1, 0.0)
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))


# ------------------------------------------------------------------------------------------- 4. the fine-tuning steps
def snapshot(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def test_reinforce_step_default_and_clipped():
    from gct_plus_amd.Train.finetune import reinforce_loss, reinforce_step
    from tests.test_ppo_gpu import fused_adam, ppo_sampler
    # the default: the keys and the bits of the step as it was before the argument existed, written out by hand
    sp, t, rows, reward = ppo_sampler()
    stats = reinforce_step(sp, fused_adam(sp.model), rows, reward)
    assert set(stats) == {"loss", "mean_reward", "mean_logp", "tokens"}
    sp2, _, rows2, _ = ppo_sampler()
    opt2 = fused_adam(sp2.model)
    sp2.model.train()
    scores = sp2.logp(*rows2)
    opt2.zero_grad(set_to_none=True)
    reinforce_loss(scores.logp, reward, "mean").backward()
    opt2.step()
    sp2.model.eval()
    got, want = snapshot(sp.model), snapshot(sp2.model)
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: the default reinforce_step is not the step it was"
    assert opt2.clip_state is None
    # clipped: half of that gradient's norm
    sp3, _, rows3, _ = ppo_sampler()
    opt3 = fused_adam(sp3.model)
    opt3.max_grad_norm = 1e9                                      # the optimizer's own setting; the call's value wins
    norm = float(sp2.model.flat_grads().double().norm())
    stats3 = reinforce_step(sp3, opt3, rows3, reward, max_grad_norm=0.5 * norm)
    assert set(stats3) == set(stats) | {"grad_norm", "clipped"}
    dev = opt3.grad_norm_stats()
    assert stats3["grad_norm"] == dev["norm"] and stats3["clipped"] is True and dev["clipped_steps"] == 1
    assert abs(dev["norm"] - norm) <= TOL * norm
    assert opt3.max_grad_norm == 1e9                              # put back
    assert {k: stats3[k] for k in stats} == stats                 # the forward and the loss are the unclipped ones
    # a call that passes None leaves the optimizer's own setting in force
    stats4 = reinforce_step(sp3, opt3, rows3, reward)
    assert stats4["clipped"] is False and opt3.grad_norm_stats()["steps"] == 2
    # ... and an exception (a reward per row is required) still puts the setting back
    with pytest.raises(ValueError, match="rewards"):
        reinforce_step(sp3, opt3, rows3, reward[:-1], max_grad_norm=0.25)
    assert opt3.max_grad_norm == 1e9 and not sp3.model.training


def test_ppo_update_default_and_clipped():
    from gct_plus_amd.Train.finetune import _row_slice, advantages, ppo_loss, ppo_update
    from gct_plus_amd.decode import clip_pair
    from tests.test_ppo_gpu import fused_adam, ppo_sampler
    sp, t, rows, reward = ppo_sampler()
    n, half = len(reward), len(reward) // 2
    hist = ppo_update(sp, fused_adam(sp.model), rows, reward, epochs=2, minibatch=half)
    assert len(hist) == 2 and all(set(h) == {"loss", "mean_surrogate", "clip_fraction", "approx_kl", "tokens"} for h in hist)
    # the same updates written out by hand, as ppo_update ran them before the argument existed
    sp2, _, rows2, _ = ppo_sampler()
    opt2 = fused_adam(sp2.model)
    rows2 = tuple(rows2)
    sp2.model.eval()
    adv = advantages(reward.to(sp2.device), "mean", False).cpu()
    with torch.no_grad():
        old = sp2.logp(*rows2).token_logp
    for _ in range(2):
        for lo in range(0, n, half):
            terms = sp2.ppo_terms(*_row_slice(rows2, lo, lo + half), old_token_logp=old[lo:lo + half],
                                  advantage=adv[lo:lo + half], clip=clip_pair(0.2), prior=None, entropy=False)
            opt2.zero_grad(set_to_none=True)
            ppo_loss(terms, 0.0, 0.0).backward()
            opt2.step()
    got, want = snapshot(sp.model), snapshot(sp2.model)
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: the default ppo_update is not the update it was"
    # clipped
    sp3, _, rows3, _ = ppo_sampler()
    opt3 = fused_adam(sp3.model)
    hist3 = ppo_update(sp3, opt3, rows3, reward, epochs=2, minibatch=half, max_grad_norm=1e-3)
    assert all(set(h) == set(hist[0]) | {"grad_norm", "clipped_updates"} for h in hist3)
    dev = opt3.grad_norm_stats()
    assert (dev["steps"], dev["nonfinite_steps"]) == (4, 0)
    assert sum(h["clipped_updates"] for h in hist3) == dev["clipped_steps"] == 4     # 1e-3: far below these gradients
    assert max(h["grad_norm"] for h in hist3) == dev["max_norm"] and all(h["grad_norm"] > 1e-3 for h in hist3)
    assert opt3.max_grad_norm is None
    # an exception from inside the update loop puts the optimizer's OWN setting back (the call's value was installed)
    opt3.max_grad_norm = 7.0
    seen = []

    def failing_terms(*a, **kw):
        seen.append(opt3.max_grad_norm)
        raise RuntimeError("stop here")
    sp3.ppo_terms = failing_terms
    with pytest.raises(RuntimeError, match="stop here"):
        ppo_update(sp3, opt3, rows3, reward, epochs=2, minibatch=half, max_grad_norm=0.25)
    del sp3.ppo_terms
    assert seen == [0.25] and opt3.max_grad_norm == 7.0 and not sp3.model.training


# ---------------------------------------------------------------------------------------------------- 5. two ranks
def _dp_data(world):
    from gct_plus_amd import synthetic
    ds = synthetic.make_dataset(8 * world * 3, 20, "pvaetf", seed=5)
    eps_all = torch.randn(8 * world * 3, 23, 16, generator=torch.Generator().manual_seed(9))
    return ds, eps_all


def _clip_worker(rank, world, port, out, c):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gct_plus_amd.dp import FlatDataParallel
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.testing import host_staged_allreduce, host_staged_broadcast
    model = dp_build(100 + rank)
    ddp = FlatDataParallel(model, allreduce=host_staged_allreduce, broadcast=host_staged_broadcast)
    opt = FusedAdam(model.parameters(), lr=LR, betas=(0.9, 0.98), eps=1e-9, model=model, max_grad_norm=c)
    ds, eps_all = _dp_data(world)
    coefs = []
    for step in range(3):
        idx = torch.arange(8) + (step * world + rank) * 8
        _step_fn("pvaetf", ddp, opt, {k: v[idx].cuda() for k, v in ds.items()}, eps_all[idx])
        coefs.append(opt.clip_state.cpu().view(torch.int32)[:2].clone())          # norm and coef, as bits
    out[rank] = dict(state={k: v.detach().cpu() for k, v in model.state_dict().items()}, coefs=torch.stack(coefs),
                     stats=opt.grad_norm_stats())
    dist.barrier()
    dist.destroy_process_group()


class _BackwardOnly:
    """_step_fn's optimizer for a forward and backward without an update."""

    def __init__(self, opt):
        self.zero_grad = opt.zero_grad

    def step(self):
        pass


def _single_process(world):
    """Three clipped steps of one process on the global batch, gradient scaled by 1 / world, with c = half the norm of
    the first step's MEAN gradient (measured by a backward without an update): (c, parameters, grad_norm_stats())."""
    from gct_plus_amd.optim import FusedAdam
    model = dp_build(100)
    opt = FusedAdam(model.parameters(), lr=LR, betas=(0.9, 0.98), eps=1e-9, model=model)
    opt.grad_scale = 1.0 / world
    ds, eps_all = _dp_data(world)
    for step in (None, 0, 1, 2):
        idx = torch.arange(8 * world) + (step or 0) * 8 * world
        _step_fn("pvaetf", model, _BackwardOnly(opt) if step is None else opt, {k: v[idx].cuda() for k, v in ds.items()},
                 eps_all[idx])
        if step is None:
            model.sync_grads_to_flat()
            opt.max_grad_norm = 0.5 * opt.grad_scale * float(model.flat_grads().double().norm())
    return opt.max_grad_norm, {k: v.detach().cpu() for k, v in model.state_dict().items()}, opt.grad_norm_stats()


def test_two_ranks_clip_alike_and_match_the_global_batch():
    world = 2
    c, ref, stats = _single_process(world)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_clip_worker, args=(world, _port(), out, c), nprocs=world, join=True)
    a, b = out[0], out[1]
    assert torch.equal(a["coefs"], b["coefs"]), "the ranks disagree on norm / coef"
    assert a["stats"] == b["stats"] and a["stats"]["clipped_steps"] == 3 and a["stats"]["steps"] == 3
    for k in a["state"]:
        assert torch.equal(a["state"][k], b["state"][k]), f"ranks diverged on {k}"
    assert stats["clipped_steps"] == 3 and stats["steps"] == 3
    assert abs(stats["max_norm"] - a["stats"]["max_norm"]) <= 1e-4 * stats["max_norm"]
    for k in ref:
        if k.endswith("k_linear.bias"):                              # tests/test_dp_gpu.py: an analytically zero gradient
            assert torch.allclose(a["state"][k], ref[k], atol=7e-3), k
            continue
        assert torch.allclose(a["state"][k], ref[k], atol=2e-5, rtol=1e-4), k
