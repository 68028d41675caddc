"""Beam-search rules on the host (gct_plus_amd.decode.beam_step_reference / beam_finalize): hand-built known answers,
and the beam-size validation of the sampling front end.  No GPU."""
import math

import pytest
import torch

from gct_plus_amd import synthetic
from gct_plus_amd.decode import (beam_finalize, beam_init, beam_log_softmax, beam_step_reference, check_beam_size)

PAD, EOS = 0, 2
NEG = -math.inf


def logp_of(rows):
    return beam_log_softmax(torch.tensor(rows, dtype=torch.float32))


def test_log_softmax_is_x_minus_m_minus_log_sum():
    x = torch.tensor([[1.0, 3.0, -2.0, 0.5]])
    m = 3.0
    want = x - m - math.log(float(torch.exp(x - m).sum()))
    assert torch.equal(beam_log_softmax(x), want)


def test_first_step_expands_beam_zero_only():
    """After the prefill every beam holds the same prefix; scores [0, -inf, -inf] keep the k children distinct."""
    scores, fin, lens = beam_init(1, 3)
    assert scores.tolist() == [[0.0, NEG, NEG]] and not fin.any() and not lens.any()
    row = [0.0, 1.0, 4.0, 3.0, 2.0]
    lp = logp_of([row] * 3)
    parent, tok, sc, f2, l2 = beam_step_reference(scores, fin, lens, lp, 3, PAD, EOS)
    assert parent.tolist() == [[0, 0, 0]]
    assert tok.tolist() == [[2, 3, 4]]                     # the three best tokens of beam 0, no duplicates
    assert torch.equal(sc[0], lp[0, [2, 3, 4]])
    assert f2.tolist() == [[True, False, False]]           # token 2 is <eos>
    assert l2.tolist() == [[1, 1, 1]]


def test_finished_beam_is_frozen_with_one_candidate():
    """A finished beam offers itself once (token pad, score unchanged, length unchanged) and is not extended."""
    scores = torch.tensor([[-0.5, -3.0]])
    fin = torch.tensor([[True, False]])
    lens = torch.tensor([[4, 6]])
    lp = logp_of([[9.0, 0.0, 0.0, 0.0, 0.0], [0.0, 5.0, 0.0, 4.0, 0.0]])   # beam 0's row must be ignored
    parent, tok, sc, f2, l2 = beam_step_reference(scores, fin, lens, lp, 2, PAD, EOS)
    assert parent.tolist() == [[0, 1]] and tok.tolist() == [[PAD, 1]]
    assert float(sc[0, 0]) == -0.5                          # frozen: exactly its old score
    assert float(sc[0, 1]) == float(torch.tensor(-3.0) + lp[1, 1])
    assert f2.tolist() == [[True, False]] and l2.tolist() == [[4, 7]]
    # the frozen beam is one candidate only: with a worse score it yields to both of beam 1's best tokens
    scores = torch.tensor([[-9.0, -3.0]])
    parent, tok, _, _, l2 = beam_step_reference(scores, fin, lens, lp, 2, PAD, EOS)
    assert parent.tolist() == [[1, 1]] and tok.tolist() == [[1, 3]] and l2.tolist() == [[7, 7]]


def test_all_finished_sample_stays_put():
    scores = torch.tensor([[-1.0, -2.0, -2.5]])
    fin = torch.ones(1, 3, dtype=torch.bool)
    lens = torch.tensor([[3, 5, 2]])
    lp = logp_of([[1.0, 2.0, 3.0, 4.0]] * 3)
    parent, tok, sc, f2, l2 = beam_step_reference(scores, fin, lens, lp, 3, PAD, EOS)
    assert parent.tolist() == [[0, 1, 2]] and tok.tolist() == [[PAD] * 3]
    assert torch.equal(sc, scores) and f2.all() and torch.equal(l2, lens)


def test_ties_go_to_the_lower_flat_index():
    """Equal candidates: lower beam * V + token wins -- across beams (identical rows and scores) and within a beam."""
    row = [0.0, 2.0, 2.0, 1.0, 2.0]
    scores = torch.tensor([[-1.0, -1.0]])
    fin = torch.zeros(1, 2, dtype=torch.bool)
    lens = torch.tensor([[3, 3]])
    lp = logp_of([row, row])
    parent, tok, sc, _, _ = beam_step_reference(scores, fin, lens, lp, 2, PAD, EOS)
    assert parent.tolist() == [[0, 0]] and tok.tolist() == [[1, 2]]
    assert float(sc[0, 0]) == float(sc[0, 1])
    # a frozen beam's candidate ties at flat index beam * V + pad: after beam 0's three equal best tokens
    lp = logp_of([row] * 4)
    best = float(torch.tensor(-1.0) + lp[0, 1])
    scores = torch.tensor([[-1.0, best, -100.0, -100.0]])
    fin = torch.tensor([[False, True, True, True]])
    parent, tok, sc, _, _ = beam_step_reference(scores, fin, torch.full((1, 4), 3), lp, 4, PAD, EOS)
    assert parent.tolist() == [[0, 0, 0, 1]] and tok.tolist() == [[1, 2, 4, PAD]]
    assert sc.tolist() == [[best] * 4]


def test_samples_are_independent():
    s1, f1, l1 = beam_init(2, 2)
    lp = logp_of([[0.0, 1.0, 2.0, 3.0]] * 2 + [[3.0, 2.0, 1.0, 0.0]] * 2)
    parent, tok, _, _, _ = beam_step_reference(s1, f1, l1, lp, 2, PAD, EOS)
    assert parent.tolist() == [[0, 0], [0, 0]] and tok.tolist() == [[3, 2], [0, 1]]


def test_final_ranking_is_length_normalised():
    """score / length**0.7, ties to the lower beam; ids cut to prefix + the longest beam."""
    t0 = 1
    ys = torch.tensor([[[1, 5, 2, 0, 0, 0], [1, 6, 7, 8, 2, 0], [1, 9, 2, 0, 0, 0]]])
    scores = torch.tensor([[-2.0, -2.6, -2.0]])
    lens = torch.tensor([[2, 4, 2]])
    out, sc, ln = beam_finalize(ys, scores, lens, t0, alpha=0.7)
    # -2/2^0.7 = -1.231, -2.6/4^0.7 = -0.985: the longer beam wins; beams 0 and 2 tie, 0 first
    assert torch.equal(sc, torch.tensor([[-2.6, -2.0, -2.0]])) and ln.tolist() == [[4, 2, 2]]
    assert out.tolist() == [[[1, 6, 7, 8, 2], [1, 5, 2, 0, 0], [1, 9, 2, 0, 0]]]
    out, sc, _ = beam_finalize(ys, scores, lens, t0, alpha=0.0)                     # no penalty: raw scores
    assert torch.equal(sc, torch.tensor([[-2.0, -2.0, -2.6]])) and out[0, 1, 1] == 9


def test_check_beam_size_limits():
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            check_beam_size(bad, 30)
    with pytest.raises(ValueError):
        check_beam_size(5, 4)                                  # more beams than tokens
    for ok in (1, 4, 16):
        check_beam_size(ok, 30)


def test_sampling_rejects_bad_beam_sizes_before_any_launch():
    from gct_plus_amd import data
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    from gct_plus_amd.Model import model_dict
    strs = ["CCO", "c1ccccc1", "CC(=O)N"]
    SRC, TRG = data.Vocab.build(strs, False, False), data.Vocab.build(strs, True, False)
    model = model_dict["vaetf"](len(SRC), len(TRG), N=1, d_model=32, dff=64, h=2, latent_dim=8, dropout=0.0, nconds=0)
    V = model.out.weight.shape[0]
    for bad in (0, 17, V + 1):
        with pytest.raises(ValueError):
            get_sampler("vaetf", model, SRC, TRG, latent_dim=8, decode_algo="beam", beam_size=bad, device="cpu")
    sp = get_sampler("vaetf", model, SRC, TRG, latent_dim=8, decode_algo="beam", beam_size=3, device="cpu")
    assert sp.beam_size == 3 and sp.beam_alpha == 0.7
    # greedy keeps ignoring the beam arguments
    get_sampler("vaetf", model, SRC, TRG, latent_dim=8, decode_algo="greedy", beam_size=0, device="cpu")
    with pytest.raises(ValueError):
        sp.decode_beams(torch.zeros(1, 4, 8), torch.ones(1, 1, dtype=torch.long), torch.ones(1, 1, 4, dtype=torch.bool),
                        beam_size=17)


def test_reference_beam_search_over_a_fixed_table():
    """A whole search over a position-indexed logit table with the rules above (the loop of
    reference_style_beam_decode without a model): frozen beams keep their ids, pads follow <eos>."""
    V, k, n = 5, 2, 1
    table = torch.tensor([[0.0, 0.0, 1.0, 3.0, 0.0],      # step 0: token 3 best, <eos> second
                          [0.0, 0.0, 4.0, 0.0, 0.0],      # step 1: <eos> after anything
                          [0.0, 0.0, 4.0, 0.0, 0.0]])
    scores, fin, lens = beam_init(n, k)
    ys = torch.full((n * k, 1), synthetic.SOS_ID)
    for t in range(3):
        lp = beam_log_softmax(table[t].expand(n * k, V))
        parent, tok, scores, fin, lens = beam_step_reference(scores, fin, lens, lp, k, PAD, EOS)
        ys = torch.cat([ys[parent.view(-1)], tok.view(-1, 1)], 1)
        if fin.all():
            break
    out, sc, ln = beam_finalize(ys.view(n, k, -1), scores, lens, 1)
    lp0, lp1 = beam_log_softmax(table[0]), beam_log_softmax(table[1])
    # beam "3 <eos>" (2 tokens) against "<eos>" (1 token, frozen after step 0)
    assert sorted(ln[0].tolist()) == [1, 2]
    a = float(lp0[3] + lp1[2]) / 2 ** 0.7
    b = float(lp0[2]) / 1 ** 0.7
    best = [synthetic.SOS_ID, 3, EOS] if a > b else [synthetic.SOS_ID, EOS, PAD]
    assert out[0, 0].tolist() == best
