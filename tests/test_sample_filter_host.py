"""Top-k / nucleus / temperature sampling on the host: known answers of decode.sample_filter_reference (the statement of
the rules the gfx950 kernel implements), agreement with a torch.topk statement of the reference's top_k_logits, the
settings record, and argument validation of the sampler front end and KVDecoder.generate.  No GPU."""
import math

import pytest
import torch

from gct_plus_amd import data, ops, synthetic
from gct_plus_amd.decode import KVDecoder, check_sample_filter, sample_filter_reference
from gct_plus_amd.Inference.sampling_tool import get_sampler
from tests.test_data_pipeline import SMILES

TINY = dict(N=1, d_model=32, dff=64, h=4, latent_dim=8)


def normalised(w):
    w = torch.as_tensor(w, dtype=torch.float64)
    return w / w.sum(-1, keepdim=True)


def close(a, b, tol=1e-7):
    return torch.allclose(a.double(), torch.as_tensor(b).double(), atol=tol, rtol=0)


def test_top_k_keeps_ties_at_the_kth_logit():
    x = torch.tensor([[3.0, 2.0, 2.0, 1.0, 0.0]])
    p = torch.softmax(x, -1)[0].double()
    want = normalised([p[0], p[1], p[2], 1e-6, 1e-6])
    assert close(sample_filter_reference(x, top_k=2)[0], want)
    assert close(sample_filter_reference(x, top_k=3)[0], want)                  # 3 tokens have < 3 larger logits
    assert close(sample_filter_reference(x, top_k=4)[0], normalised([p[0], p[1], p[2], p[3], 1e-6]))


def test_top_k_floor_and_renormalisation_exact():
    # one token in, three at the floor: w = [p0, 1e-6, 1e-6, 1e-6] / (p0 + 3e-6)
    x = torch.tensor([10.0, 0.0, 0.0, 0.0])
    p0 = float(torch.softmax(x, -1)[0])
    got = sample_filter_reference(x, top_k=1).double()
    floor = float(torch.tensor(1e-6, dtype=torch.float32))
    s = p0 + 3 * floor
    want = torch.tensor([p0 / s, floor / s, floor / s, floor / s], dtype=torch.float64)
    assert torch.allclose(got, want, rtol=1e-6, atol=0)                          # fp32: relative, to a few ulp
    assert float(got[1]) == float(got[2]) == float(got[3]) and abs(float(got[1]) - floor / s) < 1e-12
    # equal logits: every token ties at the k-th value, nothing is floored
    assert close(sample_filter_reference(torch.zeros(6), top_k=1), torch.full((6,), 1 / 6))


def test_neutral_settings_are_no_ops():
    x = torch.randn(5, 37, generator=torch.Generator().manual_seed(0))
    plain = sample_filter_reference(x)
    assert torch.equal(sample_filter_reference(x, top_k=37, top_p=1.0, temperature=1.0), plain)
    assert close(plain, torch.softmax(x, -1))
    assert not check_sample_filter(None, None, 1.0, 37) and not check_sample_filter(37, 1.0, 1, 37)
    assert check_sample_filter(36, None, 1.0, 37) and check_sample_filter(None, 0.99, 1.0, 37)
    assert check_sample_filter(None, None, 0.5, 37)


def test_nucleus_keeps_boundary_ties():
    x = torch.log(torch.tensor([0.4, 0.2, 0.2, 0.2]))
    # tokens 1..3 each have a strictly larger mass of 0.4: all kept below 0.4 < top_p, all dropped above
    assert close(sample_filter_reference(x, top_p=0.45), [0.4, 0.2, 0.2, 0.2], 1e-6)
    assert close(sample_filter_reference(x, top_p=0.35), [1.0, 0.0, 0.0, 0.0])
    x = torch.log(torch.tensor([0.1, 0.4, 0.2, 0.3]))
    # masses strictly above: 0.9, 0, 0.7, 0.4
    assert close(sample_filter_reference(x, top_p=0.65), [0.0, 4 / 7, 0.0, 3 / 7], 1e-6)
    assert close(sample_filter_reference(x, top_p=0.75), [0.0, 0.4 / 0.9, 0.2 / 0.9, 0.3 / 0.9], 1e-6)


def test_tiny_top_p_keeps_only_the_argmax_and_its_ties():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [0.5, -1.0, 2.0, 1.9]])
    got = sample_filter_reference(x, top_p=1e-9)
    assert close(got, [[0.0, 0.5, 0.5, 0.0], [0.0, 0.0, 1.0, 0.0]])


def test_temperature_is_softmax_of_scaled_logits():
    x = torch.randn(4, 30, generator=torch.Generator().manual_seed(1)) * 3
    for T in (0.7, 1.5, 0.05, 20.0):
        assert close(sample_filter_reference(x, temperature=T), torch.softmax(x / T, -1), 1e-6)
    # temperature keeps the order, so the top-k set is the one of the raw logits
    assert bool(((sample_filter_reference(x, top_k=5, temperature=3.0) > 1e-5).sum(-1) == 5).all())


def test_filters_combined():
    x = torch.log(torch.tensor([0.4, 0.3, 0.2, 0.1]))
    # top-k 2: w = [0.4, 0.3, 1e-6, 1e-6]; masses above in s = w / sum w: 0, 0.571, ~1, ~1
    assert close(sample_filter_reference(x, top_k=2, top_p=0.6), [4 / 7, 3 / 7, 0.0, 0.0], 1e-6)
    assert close(sample_filter_reference(x, top_k=2, top_p=0.5), [1.0, 0.0, 0.0, 0.0])
    # with top_p = 1 the floored tokens stay at their 1e-6
    got = sample_filter_reference(x, top_k=2, top_p=1.0).double()
    assert close(got, normalised([0.4, 0.3, 1e-6, 1e-6]), 1e-7)
    # temperature first: T = 0.5 squares the odds, p = [16, 9, 4, 1] / 30; top-k 3 floors token 3; masses above:
    # 0, 0.533, 0.833, ~1
    got = sample_filter_reference(x, top_k=3, top_p=0.8, temperature=0.5)
    assert close(got, [16 / 25, 9 / 25, 0.0, 0.0], 1e-6)
    got = sample_filter_reference(x, top_k=3, top_p=0.9, temperature=0.5)
    assert close(got, [16 / 29, 9 / 29, 4 / 29, 0.0], 1e-6)


def topk_logits_statement(x, k):
    """The reference's top_k_logits on softmax probabilities, through torch.topk: tokens below the k-th largest
    probability get 1e-6, then torch.multinomial's renormalisation."""
    p = torch.softmax(x.float(), -1)
    vk = torch.topk(p, k, dim=-1).values[..., -1:]
    return normalised(torch.where(p < vk, torch.full_like(p, 1e-6), p))


@pytest.mark.parametrize("V", [30, 64, 65, 1024])
def test_top_k_matches_a_topk_statement_on_random_rows(V):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(64, V, generator=g) * 2
    for k in (1, 2, 4, V // 2, V - 1, V):
        # relative: a token floored on one side only would be off by orders of magnitude
        got = sample_filter_reference(x, top_k=k).double()
        assert torch.allclose(got, topk_logits_statement(x, k), rtol=2e-6, atol=0), k


def test_nucleus_against_a_sorted_cumulative_statement():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 40, generator=g) * 2
    for p in (0.3, 0.7, 0.95):
        s = torch.softmax(x, -1).double()
        desc, order = s.sort(-1, descending=True)
        before = desc.cumsum(-1) - desc                                        # mass ahead of each sorted token
        keep = torch.zeros_like(s, dtype=torch.bool).scatter(-1, order, before < p)
        assert close(sample_filter_reference(x, top_p=p), normalised(torch.where(keep, s, torch.zeros_like(s))), 1e-6)


def test_settings_record_layout():
    t = ops.sample_filter_settings(4, 0.9, 0.8, 30)
    assert t.dtype == torch.int32 and t.shape == (4,)
    f = t.view(torch.float32)
    assert int(t[0]) == 4 and float(f[1]) == float(torch.tensor(0.9)) and float(f[2]) == float(torch.tensor(1 / 0.8))
    t = ops.sample_filter_settings(None, None, 1.0, 30)
    assert int(t[0]) == 30 and float(t.view(torch.float32)[1]) == 1.0 and float(t.view(torch.float32)[2]) == 1.0


BAD = [dict(top_k=0), dict(top_k=-3), dict(top_k=2.5), dict(top_k=True), dict(top_k="4"),
       dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=math.nan), dict(top_p=True),
       dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.inf), dict(temperature=math.nan),
       dict(temperature=1e-300), dict(temperature=None)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_bad_settings_raise(bad):
    with pytest.raises(ValueError):
        check_sample_filter(vocab=30, **bad)
    with pytest.raises(ValueError):
        sample_filter_reference(torch.zeros(2, 30), **bad)


def build_model(mtype):
    from gct_plus_amd.Model import model_dict
    sep = mtype in ("scavaetf", "pscavaetf")
    strs = [("c1ccccc1<sep>" + s) if sep else s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, sep), data.Vocab.build(strs, True, sep)
    nc = synthetic.n_conds(mtype)
    torch.manual_seed(0)
    model = model_dict[mtype](len(SRC), len(TRG), dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).eval()
    return model, SRC, TRG, nc


@pytest.mark.parametrize("mtype", ["vaetf", "pvaetf", "scavaetf", "pscavaetf"])
def test_get_sampler_accepts_the_reference_top_k(mtype):
    model, SRC, TRG, nc = build_model(mtype)
    kw = dict(latent_dim=TINY["latent_dim"], max_strlen=12, cond_dim=nc, device="cpu")
    sp = get_sampler(mtype, model, SRC, TRG, top_k=None, **kw)                 # the reference's kwargs always carry it
    assert sp.top_k is None and sp.top_p is None and sp.temperature == 1.0
    sp = get_sampler(mtype, model, SRC, TRG, decode_algo="multinomial", top_k=4, top_p=0.9, temperature=0.8, **kw)
    assert (sp.top_k, sp.top_p, sp.temperature) == (4, 0.9, 0.8)
    get_sampler(mtype, model, SRC, TRG, decode_algo="greedy", top_k=4, **kw)  # greedy ignores the filters
    V = len(TRG)
    for bad in BAD + [dict(top_k=V + 1)]:
        with pytest.raises(ValueError):
            get_sampler(mtype, model, SRC, TRG, decode_algo="multinomial", **kw, **bad)
    for filt in (dict(top_k=4), dict(top_p=0.9), dict(temperature=0.8)):
        with pytest.raises(ValueError):
            get_sampler(mtype, model, SRC, TRG, decode_algo="beam", beam_size=2, **kw, **filt)
    # neutral values are no filter: beam search takes them
    get_sampler(mtype, model, SRC, TRG, decode_algo="beam", beam_size=2, top_k=V, top_p=1.0, temperature=1.0, **kw)


def test_generate_rejects_bad_settings_before_any_device_work():
    model, SRC, TRG, _ = build_model("vaetf")
    kd = KVDecoder(model, SRC.stoi["<pad>"], TRG.stoi["<sos>"], TRG.stoi["<eos>"])     # no start(): no device state
    ys0 = torch.ones(3, 1, dtype=torch.long)
    for algo in ("multinomial", "greedy"):
        for bad in BAD + [dict(top_k=len(TRG) + 1)]:
            with pytest.raises(ValueError):
                kd.generate(ys0, 10, algo=algo, **bad)
