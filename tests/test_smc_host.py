"""Sequential Monte Carlo decoding, the part that needs no GPU: the stated rules (decode.smc_step_reference,
systematic_resample_reference) on a toy model small enough to enumerate, the step plan, the refusals, and the share of
the selection kernel's test cases that sits on a near tie."""
import math

import pytest
import torch

from gct_plus_amd import data
from gct_plus_amd.decode import (BEAM, GRAMMAR, MIXED, SBEAM, SMC, STREAM, UNIFORM, KVDecoder, SmcSamples, StepPlan,
                                 smc_finalize, smc_init, smc_row_weights, smc_step_reference,
                                 systematic_resample_reference)
from gct_plus_amd.smiles import SmilesGrammar
from tests import smc_ref
from tests.test_grammar_host import EOS, PAD, SOS, VOCAB31, VOCAB70, grammar, tiny_model

N_RUNS = 2000


# ------------------------------------------------------------------------------------------- unbiasedness
def _estimates(out, strings, Z):
    """Per run: Z^ = exp(log_z), and for each string x the unnormalised weighted frequency Z^ sum_i W_i 1[x_i = x] / Z,
    whose expectation is pi(x) / Z exactly (the self-normalised frequency alone is only consistent in k)."""
    zhat = torch.exp(out.log_z)
    W = torch.exp(out.logw.double())
    rows = [[smc_ref.string_of(r) for r in sample] for sample in out.ys.tolist()]
    freq = torch.tensor([[sum(float(W[s, i]) for i, r in enumerate(sample) if r == x) for x in strings]
                         for s, sample in enumerate(rows)], dtype=torch.float64)
    return zhat, freq * zhat.view(-1, 1) / Z


@pytest.mark.parametrize("tau", [0.0, 0.5, 1.0])
def test_the_stated_rules_are_unbiased_on_the_toy_model(tau):
    """The toy model of tests/smc_ref.py (table seed 1: 660 well-formed strings within G = 5, Z = 0.1420), K = 4,
    N = 2 000 runs per threshold.  mean(Z^) lies within 4 standard errors of Z, and the weighted frequencies of the five
    likeliest well-formed strings (pi / Z = 0.356, 0.206, 0.161, 0.060, 0.059) within 4 standard errors of pi(x) / Z.
    The locally renormalised sampler (K = 1, weights ignored) draws them with probabilities 0.109, 0.043, 0.029, 0.020,
    0.150 instead: with this seed every one of the five is off by more than 11 binomial standard errors at N = 2 000
    (35, 36, 35, 13, 11), where the test asks for one beyond 6."""
    toy = smc_ref.toy()
    assert len(toy.strings) == 660 and abs(toy.Z - 0.1420) < 1e-4
    top = sorted(toy.strings, key=lambda x: -toy.strings[x][0])[:5]
    want = torch.tensor([toy.strings[x][0] / toy.Z for x in top], dtype=torch.float64)
    out = toy.run(N_RUNS, 4, tau, seed=100 + int(10 * tau))
    assert all(toy.gr.well_formed(r) for r in out.ys.view(-1, out.ys.shape[2])[:400].tolist())
    if tau == 0.0:
        assert int(out.resamples.max()) == 0
    if tau == 1.0:
        assert int(out.resamples.min()) >= 1
    zhat, freq = _estimates(out, top, toy.Z)
    se_z = float(zhat.std()) / math.sqrt(N_RUNS)
    print(f"tau={tau}: mean Z^ {float(zhat.mean()):.5f} (Z {toy.Z:.5f}, se {se_z:.5f}); mean ESS {float(out.ess.mean()):.2f}")
    assert abs(float(zhat.mean()) - toy.Z) <= 4 * se_z
    se = freq.std(0) / math.sqrt(N_RUNS)
    print("   weighted frequencies", [f"{v:.3f}" for v in freq.mean(0).tolist()], "want", [f"{v:.3f}" for v in want.tolist()])
    assert bool(((freq.mean(0) - want).abs() <= 4 * se).all()), ((freq.mean(0) - want) / se).tolist()
    # the locally renormalised sampler: K = 1, weights ignored
    plain = toy.run(N_RUNS, 1, tau, seed=200 + int(10 * tau))
    drawn = [smc_ref.string_of(r[0]) for r in plain.ys.tolist()]
    f1 = torch.tensor([sum(r == x for r in drawn) / N_RUNS for x in top], dtype=torch.float64)
    se1 = torch.sqrt((f1 * (1 - f1)).clamp(min=1.0 / N_RUNS ** 2) / N_RUNS)
    off = ((f1 - want).abs() / se1)
    print("   locally normalised", [f"{v:.3f}" for v in f1.tolist()], "off by (se)", [f"{v:.1f}" for v in off.tolist()])
    assert float(off.max()) > 6.0
    q = torch.tensor([toy.strings[x][1] for x in top], dtype=torch.float64)      # ... and it draws q, as enumerated
    assert bool(((f1 - q).abs() <= 4 * torch.sqrt(q * (1 - q) / N_RUNS)).all())


def test_step_reference_edge_rules():
    """Idle samples, dead particles, an all-dead sample, finished parents, on a hand-made step."""
    inf = math.inf
    k, V, pad, eos = 3, 5, 0, 1
    x = torch.zeros(3 * k, V, dtype=torch.float64)
    y = x.clone()
    y[:, pad] = -inf
    y[4] = -inf                                                       # sample 1, particle 1: nothing allowed
    y[6:9] = -inf                                                     # sample 2: all dead
    logw = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    fin = torch.tensor([[True, True, True], [True, False, False], [False, False, False]])
    lens = torch.tensor([[2, 3, 4], [2, 3, 4], [1, 1, 1]])
    u = torch.full((3, k + 1), 0.5, dtype=torch.float64)
    log_z, res = torch.tensor([-1.0, -2.0, -3.0], dtype=torch.float64), torch.tensor([1, 2, 3])
    anc, tok, lw, lp, f2, l2, lz, rs = smc_step_reference(logw, torch.zeros(3, k, dtype=torch.float64), fin, lens, x, y, u,
                                                          k, pad, eos, 0.0, log_z, res)
    a = math.log(4 / 5)                                               # four of five equal tokens allowed
    assert anc.tolist() == [[0, 1, 2]] * 3 and rs.tolist() == [1, 2, 3]
    assert tok[0].tolist() == [pad] * 3 and lw[0].tolist() == [0.0] * 3 and l2[0].tolist() == [2, 3, 4]     # idle
    assert tok[1, 0] == pad and tok[1, 1] == pad and tok[1, 2] != pad
    assert lw[1, 0] == 0.0 and lw[1, 1] == -inf and abs(float(lw[1, 2]) - (-1.0 + a)) < 1e-12
    assert f2[1].tolist() == [True, True, bool(tok[1, 2] == eos)] and l2[1].tolist() == [2, 3, 5]
    assert abs(float(lp[1, 2]) - math.log(1 / 5)) < 1e-12 and lp[1, 0] == 0.0
    assert lz.tolist()[:2] == [-1.0, -2.0] and lz[2] == -inf and bool(f2[2].all()) and tok[2].tolist() == [pad] * 3
    # tau = 1: sample 1 resamples among particles 0 (finished, w = 1) and 2 (w = 0.8 / e); the dead one is never chosen
    anc, tok, lw, lp, f2, l2, lz, rs = smc_step_reference(logw, torch.zeros(3, k, dtype=torch.float64), fin, lens, x, y, u,
                                                          k, pad, eos, 1.0, log_z, res)
    assert rs.tolist() == [1, 3, 3] and 1 not in anc[1].tolist() and lw[1].tolist() == [0.0] * 3
    w2 = math.exp(-1.0 + a)
    assert abs(float(lz[1]) - (-2.0 + math.log((1 + w2) / 3))) < 1e-12
    norm, lzf, ess = smc_finalize(lw, lz)
    assert abs(float(torch.logsumexp(norm[1], 0))) < 1e-12 and abs(float(ess[1]) - 3.0) < 1e-6 and lzf[2] == -inf
    assert float(ess[2]) == 0.0


# ------------------------------------------------------------------------------------------- systematic resampling
@pytest.mark.parametrize("k", [1, 2, 4, 16])
def test_systematic_resampling_counts(k):
    g = torch.Generator().manual_seed(k)
    n = 500
    w = torch.rand(n, k, generator=g, dtype=torch.float64) ** 3
    w[torch.rand(n, k, generator=g) < 0.3] = 0.0                                   # dead particles
    w[:, 0] = torch.where(w.sum(1) > 0, w[:, 0], torch.ones(n, dtype=torch.float64))
    u = torch.rand(n, generator=g, dtype=torch.float64).clamp(min=1e-9)
    u[0] = 1.0                                                                      # the draw's uniform reaches 1
    anc = systematic_resample_reference(w, u)
    assert anc.shape == (n, k) and bool((anc[:, 1:] >= anc[:, :-1]).all())          # ascending
    counts = torch.zeros(n, k, dtype=torch.float64).scatter_add_(1, anc, torch.ones(n, k, dtype=torch.float64))
    share = k * w / w.sum(1, keepdim=True)
    assert bool(((counts >= share.floor() - 1e-9) & (counts <= share.ceil() + 1e-9)).all())
    assert bool((counts[w == 0] == 0).all())                                        # dead particles are never chosen
    if k == 1:
        assert bool((anc == 0).all())


# ------------------------------------------------------------------------------------------- StepPlan, init, weights
def test_step_plan_smc():
    assert SMC == "smc" and StepPlan(SMC, UNIFORM, True).key == ("smc", "uniform", "grammar") == (SMC, UNIFORM, GRAMMAR)
    for kw in (dict(), dict(layout=MIXED, grammar=True), dict(layout=STREAM, grammar=True), dict(grammar=True, logp=True),
               dict(grammar=True, stats=True)):
        with pytest.raises(ValueError, match="sequential Monte Carlo step"):
            StepPlan(SMC, **kw)
    # what raised before still raises
    for sel, name in ((BEAM, "beam step"), (SBEAM, "stochastic beam step")):
        for kw in (dict(grammar=True), dict(layout=MIXED), dict(logp=True), dict(stats=True)):
            with pytest.raises(ValueError, match=name):
                StepPlan(sel, **kw)
    assert StepPlan(BEAM).key == "beam" and StepPlan(SBEAM).key == "sbeam" and StepPlan(1, UNIFORM, True).key == (1, UNIFORM, GRAMMAR)


def test_init_finalize_and_row_weights():
    logw, logp, fin, lens, log_z, res = smc_init(3, 4)
    assert logw.shape == logp.shape == fin.shape == lens.shape == (3, 4) and log_z.shape == res.shape == (3,)
    assert not bool(fin.any()) and float(logw.abs().sum() + logp.abs().sum()) == 0.0 and log_z.dtype == torch.float64
    lw = torch.tensor([[0.0, math.log(3.0)], [-1.0, -1.0]])
    norm, lz, ess = smc_finalize(lw, torch.tensor([-0.5, 0.0], dtype=torch.float64))
    torch.testing.assert_close(torch.exp(norm), torch.tensor([[0.25, 0.75], [0.5, 0.5]]))
    torch.testing.assert_close(lz, torch.tensor([-0.5 + math.log(2.0), -1.0], dtype=torch.float64))
    torch.testing.assert_close(ess, torch.tensor([1.6, 2.0]))
    s = SmcSamples(torch.zeros(2, 2, 1, dtype=torch.long), norm, norm, lz, torch.zeros(2, 2), ess, torch.zeros(2))
    torch.testing.assert_close(smc_row_weights(s), torch.tensor([0.5, 1.5, 1.0, 1.0]))


# ------------------------------------------------------------------------------------------- refusals
def test_generate_smc_refuses_before_any_device_work():
    kd = KVDecoder(tiny_model(VOCAB31), PAD, SOS, EOS)                               # no start(): no device state
    gr, ys0 = grammar(), torch.full((3, 1), SOS)
    for bad in (-0.1, 1.5, float("nan"), "0.5", True, None):
        with pytest.raises(ValueError, match="ess_threshold"):
            kd.generate_smc(ys0, 4, gr, 12, ess_threshold=bad)
    for bad in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError, match="particles"):
            kd.generate_smc(ys0, bad, gr, 12)
    with pytest.raises(ValueError, match="vocabulary"):
        kd.generate_smc(ys0, 4, grammar(VOCAB70), 12)
    with pytest.raises(ValueError, match="required"):
        kd.generate_smc(ys0, 4, None, 12)
    with pytest.raises(ValueError, match="at least 2"):
        kd.generate_smc(ys0, 4, gr, 2)                                               # max_strlen < 3
    with pytest.raises(ValueError, match="mixed prefix"):
        kd.generate_smc(ys0, 4, gr, 12, prefix_lens=[1, 1, 1])


def test_decode_smc_refuses_before_any_device_work():
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    model = tiny_model(VOCAB31)
    SRC, TRG = data.Vocab(["<unk>", "<pad>"] + VOCAB31[4:]), data.Vocab(VOCAB31)
    kw = dict(latent_dim=8, max_strlen=12, device="cpu")
    z, ys0, sm = torch.zeros(2, 5, 8), torch.full((2, 1), SOS), torch.ones(2, 1, 5, dtype=torch.bool)
    for sp in (get_sampler("vaetf", model, SRC, TRG, decode_algo="multinomial", well_formed=True, **kw),
               get_sampler("vaetf", model, SRC, TRG, decode_algo="beam", beam_size=2, **kw)):
        seed = sp.seed
        with pytest.raises(ValueError, match="ess_threshold"):
            sp.decode_smc(z, ys0, sm, ess_threshold=2.0)
        for bad in (0, 17):
            with pytest.raises(ValueError, match="particles"):
                sp.decode_smc(z, ys0, sm, k=bad)
        assert sp.seed == seed
    sp = get_sampler("vaetf", model, SRC, TRG, latent_dim=8, max_strlen=2, device="cpu")
    with pytest.raises(ValueError, match="at least 2"):
        sp.decode_smc(z, ys0, sm, k=2)
    # the refusals that were there stay
    sp = get_sampler("vaetf", model, SRC, TRG, decode_algo="multinomial", well_formed=True, **kw)
    with pytest.raises(ValueError, match="grammar"):
        sp.decode_beams(z, ys0, sm)
    with pytest.raises(ValueError, match="grammar"):
        sp.decode_unique(z, ys0, sm)


# ------------------------------------------------------------------------------------------- near-tie share
def test_kernel_cases_rarely_sit_on_a_near_tie():
    """A condition on the cases of tests/test_smc_gpu.py::test_smc_select_matches_reference, checked on the fp64 rules
    alone: of the six samples of any (k, V, tau) at most a quarter is undecidable in fp32 (smc_ref.kernel_reference)."""
    worst = 0.0
    for k, V, tau in smc_ref.kernel_params():
        und = torch.cat([smc_ref.kernel_reference(smc_ref.kernel_case(k, V, v, PAD, EOS), k, tau, PAD, EOS)[1]
                         for v in smc_ref.KERNEL_VARIANTS])
        worst = max(worst, float(und.float().mean()))
        assert float(und.float().mean()) <= smc_ref.UNDECIDABLE_CAP, (k, V, tau, und.tolist())
    print(f"largest undecidable share of a parameter set: {worst:.2f}")


def test_kernel_cases_cover_what_they_claim():
    """Finished and dead particles, an all-dead sample, single-token rows and an idle sample are in the cases; with
    tau = 0.5 and k > 1 some sample resamples and some does not."""
    for k in smc_ref.KERNEL_KS:
        for V in smc_ref.KERNEL_VS:
            seen = []
            for v in smc_ref.KERNEL_VARIANTS:
                case = smc_ref.kernel_case(k, V, v, PAD, EOS)
                (anc, tok, lw, lp, fin, lens, lz, rs), _ = smc_ref.kernel_reference(case, k, 0.5, PAD, EOS)
                seen.append((rs - case["res"]).tolist())
                if v == "mixed":
                    assert lz[2] == -math.inf and bool(fin[2].all()) and bool((tok[2] == PAD).all())
                    assert bool(case["fin"][1].any())
                    if k > 1:
                        assert bool((lw[1] == -math.inf).any()) or int(rs[1]) > int(case["res"][1])
                else:
                    only = torch.isfinite(case["masked"][:k]).int()
                    assert int(only.sum()) == k and int(only[0].argmax()) == EOS
                    assert torch.equal(tok[0], only.argmax(1)[anc[0]])             # each child: its ancestor's one token
                    assert bool(case["fin"][1].all()) and bool((tok[1] == PAD).all()) and lz[1] == case["log_z"][1]
            if k > 1:
                flat = sum(seen, [])
                assert 1 in flat and 0 in flat, (k, V, seen)
