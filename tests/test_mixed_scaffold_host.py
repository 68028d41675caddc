"""Mixed-scaffold batches on the host: prefix packing, per-row latent geometry, length grouping and order restoration
for beam search, the generated-token slice, and argument validation.  No GPU (the decoder itself is replaced by a
stand-in that records its calls)."""
import numpy as np
import pytest
import torch

from gct_plus_amd import data, synthetic
from gct_plus_amd.decode import KVDecoder, check_prefix_lens, generated_tokens
from gct_plus_amd.Inference.sampling_tool import (PscavaetfSampling, ScaVaeSampling, group_by_length,
                                                  latent_setup_rows, pack_prefixes)
from tests.test_data_pipeline import SMILES

TINY = dict(N=1, d_model=32, dff=64, h=4, latent_dim=8)
SCAFFOLDS = ["c1ccccc1", "C1CC1", "c1ccncc1", "C1CC1", "c1ccc2ccccc2c1", "CC"]


def test_pack_prefixes_right_pads():
    ys0, lens = pack_prefixes([[1, 5, 6], [1], [1, 7, 8, 9, 2]], pad_id=0)
    assert ys0.tolist() == [[1, 5, 6, 0, 0], [1, 0, 0, 0, 0], [1, 7, 8, 9, 2]]
    assert lens.tolist() == [3, 1, 5] and ys0.dtype == torch.long
    with pytest.raises(ValueError):
        pack_prefixes([[1], []], 0)
    with pytest.raises(ValueError):
        pack_prefixes([], 0)


def test_group_by_length_shortest_first_input_order_within():
    groups = group_by_length(torch.tensor([4, 2, 4, 7, 2, 4]))
    assert [t for t, _ in groups] == [2, 4, 7]
    assert [idx.tolist() for _, idx in groups] == [[1, 4], [0, 2, 5], [3]]
    assert sorted(i for _, idx in groups for i in idx.tolist()) == list(range(6))


def test_generated_tokens_slices_each_row_from_its_own_prefix():
    # row r: prefix of t0_r tokens (1..), generated tokens 100 + r*10 + j, pad (0) behind them
    lens = torch.tensor([2, 4, 3])
    G = 3
    ys = torch.zeros(3, 4 + G, dtype=torch.long)
    for r, t in enumerate(lens.tolist()):
        ys[r, :t] = torch.arange(1, t + 1)
        ys[r, t:t + G] = 100 + 10 * r + torch.arange(G)
    gen = generated_tokens(ys, lens)
    assert gen.tolist() == [[100, 101, 102], [110, 111, 112], [120, 121, 122]]
    assert torch.equal(generated_tokens(ys, torch.full((3,), 4)), ys[:, 4:])


def test_check_prefix_lens():
    assert check_prefix_lens(None, 3, 5) is None
    assert check_prefix_lens(torch.tensor([5, 5, 5]), 3, 5) is None          # all full width: the uniform path
    assert check_prefix_lens([5, 2, 3], 3, 5).tolist() == [5, 2, 3]
    assert check_prefix_lens(np.array([1, 5, 4], dtype=np.int32), 3, 5).dtype == torch.int64
    for bad in ([0, 2, 3], [6, 2, 3], [2, 3], [[2, 3, 4]], [1.0, 2.0, 3.0], [True, True, True]):
        with pytest.raises(ValueError):
            check_prefix_lens(bad, 3, 5)


def test_latent_setup_rows_per_row_lengths_and_masks():
    extras = [9, 4, 6]
    zs, toklen, m = latent_setup_rows(extras, None, [10, 20, 3], 8, None, lambda L, n: torch.zeros(n, L, 8))
    assert toklen == [10, 20, 3] and zs.shape == (3, 24, 8) and m.shape == (3, 1, 24)
    assert m.sum(-1).view(-1).tolist() == [19, 24, 9]
    assert all(bool(m[r, 0, :k].all()) and not bool(m[r, 0, k:].any()) for r, k in enumerate([19, 24, 9]))
    # explicit zs without toklen: every row sees all of zs (sample_smiles' rule per row)
    z = torch.randn(3, 30, 8)
    zs, toklen, m = latent_setup_rows(extras, z, None, 8, None, None)
    assert toklen == [21, 26, 24] and torch.equal(zs, z) and bool(m.all())
    # explicit zs wider than needed: cut to L_e
    zs, _, m = latent_setup_rows(extras, z, [1, 2, 3], 8, None, None)
    assert zs.shape[1] == 10 and torch.equal(zs, z[:, :10]) and m.sum(-1).view(-1).tolist() == [10, 6, 9]
    with pytest.raises(ValueError):
        latent_setup_rows(extras, z, [30, 2, 3], 8, None, None)               # zs too short
    with pytest.raises(ValueError):
        latent_setup_rows(extras, z[:2], None, 8, None, None)                 # row count
    with pytest.raises(ValueError):
        latent_setup_rows(extras, None, [1, 2], 8, None, None)                # toklen count


def make_sampler(cls, mtype, decode_algo="greedy"):
    from gct_plus_amd.Model import model_dict
    strs = ["c1ccccc1<sep>" + s for s in SMILES]
    SRC, TRG = data.Vocab.build(strs, False, True), data.Vocab.build(strs, True, True)
    nc = synthetic.n_conds(mtype)
    torch.manual_seed(0)
    model = model_dict[mtype](len(SRC), len(TRG), dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).eval()
    return cls(model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=12, cond_dim=nc, decode_algo=decode_algo,
               toklen_data=[8, 9, 10, 12], device="cpu", beam_size=2)


class FakeDecode:
    """Stands in for Sampling.decode: the generated tokens of row r are a function of z row r (so order mistakes
    show), written behind each row's own prefix; records every call."""

    def __init__(self, sp, gen_len=4):
        self.sp, self.gen_len, self.calls = sp, gen_len, []
        self.toks = [i for t, i in sp.TRG.stoi.items() if t not in ("<pad>", "<sos>", "<eos>", "<sep>", "<unk>")]

    def tokens(self, z):
        k = int(z.abs().sum() * 1000) % len(self.toks)
        return [self.toks[(k + j) % len(self.toks)] for j in range(self.gen_len)] + [self.sp.eos_id]

    def __call__(self, zs, ys, src_mask, dconds=None, prefix_lens=None):
        self.calls.append(dict(zs=zs, ys=ys, src_mask=src_mask, dconds=dconds, prefix_lens=prefix_lens))
        n, t0 = ys.shape
        lens = [t0] * n if prefix_lens is None else prefix_lens.tolist()
        out = torch.full((n, t0 + self.gen_len + 1), self.sp.pad_id, dtype=torch.long)
        for r in range(n):
            out[r, :lens[r]] = ys[r, :lens[r]]
            out[r, lens[r]:lens[r] + self.gen_len + 1] = torch.tensor(self.tokens(zs[r]))
        return out


@pytest.mark.parametrize("algo", ["greedy", "beam"])
def test_sample_multiple_smiles_packs_groups_and_restores_order(algo):
    sp = make_sampler(PscavaetfSampling, "pscavaetf", algo)
    fake = sp.decode = FakeDecode(sp)
    n = len(SCAFFOLDS)
    z = torch.randn(n, 40, TINY["latent_dim"])
    dconds = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    toklen = [5, 9, 7, 6, 8, 4]
    smiles, tl, tl_gen = sp.sample_multiple_smiles(dconds, SCAFFOLDS, zs=z, toklen=toklen, transform=False)
    sca = [sp.smi_to_id(s) for s in SCAFFOLDS]
    extras = [len(s) + 1 for s in sca]
    Le = max(e + t for e, t in zip(extras, toklen))
    want = [sp.id_to_smi(fake.tokens(z[r, :Le])) for r in range(n)]
    assert smiles == want and tl == toklen and tl_gen == [len(data.tokenize(s, True)) for s in want]
    if algo == "greedy":
        assert len(fake.calls) == 1
        c = fake.calls[0]
        assert c["prefix_lens"].tolist() == [len(s) + 2 for s in sca]
        for r in range(n):
            assert c["ys"][r, :len(sca[r]) + 2].tolist() == [sp.sos_id] + sca[r] + [sp.sep_id]
            assert bool((c["ys"][r, len(sca[r]) + 2:] == sp.pad_id).all())
        assert c["zs"].shape[1] == Le
        assert c["src_mask"].sum(-1).view(-1).tolist() == [e + t for e, t in zip(extras, toklen)]
        assert torch.equal(c["dconds"], torch.as_tensor(dconds))
    else:
        lens = [len(s) + 2 for s in sca]
        assert [c["ys"].shape[1] for c in fake.calls] == sorted(set(lens))      # one decode per prefix length
        assert all(c["prefix_lens"] is None for c in fake.calls)
        assert sorted(c["ys"].shape[0] for c in fake.calls) == sorted(lens.count(t) for t in set(lens))
        for c in fake.calls:
            assert bool((c["ys"] != sp.pad_id).all())                          # uniform prefixes, no padding
            for row, dc in zip(c["ys"], c["dconds"]):
                r = int(dc[0]) // 3
                assert row.tolist() == [sp.sos_id] + sca[r] + [sp.sep_id]


def test_scavae_sample_multiple_smiles_and_validation():
    sp = make_sampler(ScaVaeSampling, "scavaetf")
    sp.decode = FakeDecode(sp)
    smiles, tl, _ = sp.sample_multiple_smiles(SCAFFOLDS[:3])                   # sampled lengths and z
    assert len(smiles) == 3 and len(tl) == 3 and all(isinstance(s, str) for s in smiles)
    with pytest.raises(ValueError):
        sp.sample_multiple_smiles([])
    psp = make_sampler(PscavaetfSampling, "pscavaetf")
    with pytest.raises(ValueError):
        psp.sample_multiple_smiles(np.zeros((2, 3)), SCAFFOLDS[:3], transform=False)


def test_decoder_argument_validation_without_a_device():
    sp = make_sampler(PscavaetfSampling, "pscavaetf")
    kd = KVDecoder(sp.model, sp.pad_id, sp.sos_id, sp.eos_id)
    ys0 = torch.ones(3, 5, dtype=torch.long)
    with pytest.raises(ValueError):
        kd.generate_beam(ys0, 2, prefix_lens=torch.tensor([5, 3, 2]))
    for bad in (torch.tensor([0, 3, 2]), torch.tensor([6, 3, 2]), torch.tensor([5, 3])):
        with pytest.raises(ValueError):
            kd.generate(ys0, 10, prefix_lens=bad)
    with pytest.raises(ValueError):                                            # beam search takes one length per call
        make_sampler(PscavaetfSampling, "pscavaetf", "beam").decode(None, ys0, None, prefix_lens=torch.tensor([5, 3, 2]))
