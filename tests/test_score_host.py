"""The scoring rule on the CPU (decode.score_reference, check_score_inputs) and the front end's argument checks: the
rule against F.cross_entropy in fp64, the columns that are not scored, an empty row, ties, malformed inputs."""
import pytest
import torch
import torch.nn.functional as F

from gct_plus_amd.decode import check_score_inputs, score_reference

PAD = 1


def make_rows(n, W, V, seed, lens=None):
    """Random full rows: <sos> (id 2), tokens in [4, V), pad behind a random end; logits fp64 [n, W - 1, V]."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.randint(4, V, (n, W), generator=g)
    ys[:, 0] = 2
    end = torch.randint(2, W + 1, (n,), generator=g)
    ys[torch.arange(W)[None, :] >= end[:, None]] = PAD
    logits = torch.randn(n, W - 1, V, generator=g, dtype=torch.float64) * 3
    return ys, logits, end


def test_logp_is_minus_the_summed_cross_entropy():
    """Over the scored columns only: the prefix columns are taken out of the cross-entropy's targets by hand."""
    n, W, V = 7, 12, 30
    ys, logits, _ = make_rows(n, W, V, 1)
    lens = torch.tensor([1, 3, 12, 2, 5, 1, 8])
    token_logp, logp, tokens, hits = score_reference(logits, ys, lens, PAD)
    assert token_logp.dtype == torch.float64 and tokens.dtype == torch.int32 and hits.dtype == torch.int32
    tgt = ys[:, 1:].clone()
    tgt[torch.arange(1, W)[None, :] < lens[:, None]] = PAD
    want = -F.cross_entropy(logits.reshape(-1, V), tgt.reshape(-1), ignore_index=PAD, reduction="sum")
    assert abs(float(logp.sum() - want)) < 1e-10 * max(1.0, abs(float(want)))
    assert torch.equal(tokens.long(), (tgt != PAD).sum(1))
    assert torch.allclose(logp, token_logp.sum(1), atol=1e-12, rtol=0)
    # prefix_lens=None: only <sos> is given
    _, logp1, tokens1, _ = score_reference(logits, ys, None, PAD)
    want1 = -F.cross_entropy(logits.reshape(-1, V), ys[:, 1:].reshape(-1), ignore_index=PAD, reduction="sum")
    assert abs(float(logp1.sum() - want1)) < 1e-10 * abs(float(want1))
    assert torch.equal(tokens1.long(), (ys[:, 1:] != PAD).sum(1))


def test_prefix_and_pad_columns_are_zero():
    n, W, V = 6, 10, 17
    ys, logits, end = make_rows(n, W, V, 2)
    lens = torch.tensor([1, 4, 2, 10, 3, 6])
    token_logp, _, _, _ = score_reference(logits.float(), ys, lens, PAD)
    assert token_logp.dtype == torch.float32
    cols = torch.arange(W)[None, :]
    scored = (cols >= lens[:, None]) & (ys != PAD)
    assert bool((token_logp[~scored] == 0).all())
    assert bool((token_logp[scored] < 0).all())
    assert bool((token_logp[:, 0] == 0).all())


def test_a_row_whose_prefix_fills_it_gives_zeros():
    n, W, V = 3, 6, 9
    ys, logits, _ = make_rows(n, W, V, 3)
    ys[1] = torch.tensor([2, 5, 6, 7, 4, 8])                                      # no pad: the prefix is the whole row
    token_logp, logp, tokens, hits = score_reference(logits, ys, [1, W, 2], PAD)
    assert float(logp[1]) == 0.0 and int(tokens[1]) == 0 and int(hits[1]) == 0
    assert not token_logp[1].any()
    ys[2] = PAD                                                                   # an all-pad row as well
    _, logp, tokens, hits = score_reference(logits, ys, [1, W, 2], PAD)
    assert float(logp[2]) == 0.0 and int(tokens[2]) == 0 and int(hits[2]) == 0


def test_a_tie_counts_for_the_lower_index_only():
    V = 8
    x = torch.zeros(2, 1, V)
    x[:, 0, 3] = x[:, 0, 6] = 2.5                                                 # two equal maxima
    ys = torch.tensor([[2, 3], [2, 6]])
    token_logp, _, tokens, hits = score_reference(x, ys, None, PAD)
    assert tokens.tolist() == [1, 1] and hits.tolist() == [1, 0]
    assert float(token_logp[0, 1]) == float(token_logp[1, 1])


@pytest.mark.parametrize("ys,lens", [
    (torch.zeros(4, dtype=torch.long), None),                                     # not 2-D
    (torch.zeros(2, 3, 4, dtype=torch.long), None),
    (torch.zeros(3, 1, dtype=torch.long), None),                                  # narrower than 2 columns
    (torch.zeros(3, 5), None),                                                    # floating-point ids
    (torch.zeros(3, 5, dtype=torch.bool), None),
    (torch.zeros(3, 5, dtype=torch.long), torch.tensor([1.0, 2.0, 3.0])),         # floating-point prefix_lens
    (torch.zeros(3, 5, dtype=torch.long), torch.tensor([True, True, True])),
    (torch.zeros(3, 5, dtype=torch.long), [0, 1, 2]),                             # below 1
    (torch.zeros(3, 5, dtype=torch.long), [1, 6, 2]),                             # beyond W
    (torch.zeros(3, 5, dtype=torch.long), [1, 2]),                                # wrong shape
    (torch.zeros(3, 5, dtype=torch.long), [[1, 2, 3]]),
    (torch.full((3, 5), 9, dtype=torch.long), None),                              # id == V
    (torch.full((3, 5), -1, dtype=torch.long), None),                             # negative id
])
def test_check_score_inputs_refuses(ys, lens):
    with pytest.raises(ValueError):
        check_score_inputs(ys, lens, 9)


def test_check_score_inputs_accepts():
    ys = torch.randint(0, 9, (3, 5))
    assert check_score_inputs(ys, None, 9).tolist() == [1, 1, 1]
    assert check_score_inputs(ys.int(), [1, 5, 3], 9).tolist() == [1, 5, 3]
    with pytest.raises(ValueError):
        score_reference(torch.zeros(3, 5, 9), ys, None, PAD)                      # W - 1 = 4 logits rows per sequence


def test_with_logp_and_beam_search_do_not_combine():
    """The constructor refuses before it touches the model's device state: a CPU model is enough."""
    from gct_plus_amd import data
    from gct_plus_amd.Inference import sampling_tool
    from gct_plus_amd.Model import model_dict
    strs = ["c1ccccc1", "CCO"]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    model = model_dict["vaetf"](len(SRC), len(TRG), N=1, d_model=16, dff=32, h=2, latent_dim=8, dropout=0.0, nconds=0)
    with pytest.raises(ValueError, match="decode_beams"):
        sampling_tool.VaetfSampling(model, SRC, TRG, latent_dim=8, decode_algo="beam", with_logp=True)
    sp = sampling_tool.VaetfSampling(model, SRC, TRG, latent_dim=8, decode_algo="beam")
    assert sp.with_logp is False
