"""Continuous batching on the host: the schedule's one statement (stream_schedule_reference), the step counts it
predicts at MOSES-like lengths, argument validation of start_stream / generate_stream / Sampling(stream_rows=) without
a device, the binding of GctStreamState, and the front end's routing (the decoder replaced by a stand-in)."""
import math

import numpy as np
import pytest
import torch

from gct_plus_amd import ops
from gct_plus_amd.decode import (KVDecoder, check_max_new_tokens, check_stream_rows, generated_tokens,
                                 stream_schedule_reference)
from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling, VaetfSampling
from tests.test_mixed_scaffold_host import SCAFFOLDS, TINY, make_sampler


def moses_like_lengths(n, rng):
    """Generated lengths, <eos> included: clip(round(N(35, 8)), 15, 78) + 1 (tools/decode_bench.py's length model)."""
    return np.clip(np.rint(rng.normal(35, 8, n)), 15, 78).astype(int) + 1


def check_schedule(need, rows):
    need = [int(x) for x in need]
    row_of, start, makespan = stream_schedule_reference(need, rows)
    n = len(need)
    assert row_of.shape == start.shape == (n,) and row_of.dtype == start.dtype == torch.int64
    assert bool(((row_of >= 0) & (row_of < rows)).all()) and bool((start >= 0).all())          # every item started once
    end = start + torch.tensor(need)
    assert makespan == (int(end.max()) if n else 0)
    assert bool((start[1:] >= start[:-1]).all())                                              # items start in index order
    for r in range(rows):                                                                     # a row holds one item at a time
        mine = (row_of == r).nonzero().view(-1)
        assert bool((start[mine][1:] == end[mine][:-1]).all())                                 # and takes the next at once
    assert math.ceil(sum(need) / rows) <= makespan
    # after every step the freed rows take the next items in ascending row order
    for s in torch.unique(start).tolist():
        got = (start == s).nonzero().view(-1)
        assert row_of[got].tolist() == sorted(row_of[got].tolist())
    return row_of, start, makespan


def test_schedule_properties_on_random_pools():
    rng = np.random.default_rng(3)
    for n, rows in ((1, 1), (5, 8), (8, 8), (43, 8), (200, 7), (64, 64), (300, 1)):
        need = rng.integers(1, 30, n)
        _, start, makespan = check_schedule(need, rows)
        if rows >= n:
            assert makespan == int(need.max()) and bool((start == 0).all())
        if rows == 1:
            assert makespan == int(need.sum())


def test_schedule_ties_go_to_rows_in_ascending_order():
    # rows 0..2 hold items 0..2; after step 2 (two steps run) rows 0 and 2 are free together: item 3 -> row 0, item 4 ->
    # row 2; row 1 frees after 3 steps and takes item 5; item 6 goes to row 2 (free after 2 + 1 = 3 steps, with row 1:
    # row 1 is lower and takes item 5 first)
    row_of, start, makespan = stream_schedule_reference([2, 3, 2, 4, 1, 2, 5], 3)
    assert row_of.tolist() == [0, 1, 2, 0, 2, 1, 2]
    assert start.tolist() == [0, 0, 0, 2, 2, 3, 3]
    assert makespan == 8
    # a parked row stays parked: two items, four rows
    row_of, start, makespan = stream_schedule_reference([3, 1], 4)
    assert row_of.tolist() == [0, 1] and start.tolist() == [0, 0] and makespan == 3
    assert stream_schedule_reference([], 4)[2] == 0
    for bad in (([1, 0], 2), ([1, 2], 0)):
        with pytest.raises(ValueError):
            stream_schedule_reference(*bad)


@pytest.mark.parametrize("n,rows,streamed,plain,bound", [(32768, 4096, 329, 517, 289), (8192, 512, 609, 946, 577),
                                                         (30000, 512, 2147, 3554, 2113)])
def test_step_counts_at_moses_like_lengths(n, rows, streamed, plain, bound):
    """<sos> prefix: an item needs as many steps as it generates tokens.  Plain chunks run until their longest row is
    done (the prefill counted as one step); the lower bound is ceil(sum / rows).  DESIGN section 4's table."""
    g = moses_like_lengths(n, np.random.default_rng(0))
    _, _, makespan = stream_schedule_reference(g, rows)
    assert makespan == streamed
    assert sum(int(g[i:i + rows].max()) for i in range(0, n, rows)) == plain
    assert math.ceil(int(g.sum()) / rows) == bound <= makespan


def test_step_counts_with_scaffold_prefixes():
    """Prefixes of 3..30 tokens are re-consumed one token per step: 870 steps against 946 for plain mixed-prefix chunks
    (whose prefill takes a prefix in one step) at N = 8192, R = 512 -- the case that does not pay."""
    rng = np.random.default_rng(0)
    g = moses_like_lengths(8192, rng)
    t0 = rng.integers(3, 31, 8192)
    assert check_schedule(t0 + g - 1, 512)[2] == 870
    assert sum(int(g[i:i + 512].max()) for i in range(0, 8192, 512)) == 946


def test_small_validators():
    assert check_stream_rows(1) == 1 and check_stream_rows(ops.STREAM_MAX_ROWS) == ops.STREAM_MAX_ROWS
    for bad in (0, -3, ops.STREAM_MAX_ROWS + 1, 2.0, True, None):
        with pytest.raises(ValueError):
            check_stream_rows(bad)
    assert check_max_new_tokens(None, 3, 9).tolist() == [9, 9, 9]
    assert check_max_new_tokens(np.array([1, 9, 4], dtype=np.int32), 3, 9).dtype == torch.int64
    for bad in ([0, 2, 3], [10, 2, 3], [2, 3], [[2, 3, 4]], [1.0, 2.0, 3.0], [True, True, True]):
        with pytest.raises(ValueError):
            check_max_new_tokens(bad, 3, 9)


def test_stream_state_binding_follows_the_header():
    fields = ops.stream_state_fields()
    names = [f for f, _ in fields]
    assert names[0] == "ys" and names[-1] == "pad_id" and len(set(names)) == len(names)
    assert dict(fields)["ckv"] == dict(fields)["ckv_pool"] == ops.STREAM_MAX_LAYERS
    st = ops.StreamState()
    assert len(st.words) == sum(c for _, c in fields)
    st.set(rows=7, pad_id=3, ckv=[])
    assert st.words[st.slot["rows"][0]] == 7 and st.words[st.slot["pad_id"][0]] == 3
    with pytest.raises(ValueError):
        st.set(ckv=[0] * (ops.STREAM_MAX_LAYERS + 1))
    with pytest.raises(KeyError):
        st.set(no_such_field=1)
    # the limits the header defines are the ones ops states
    text = open(ops._lib.INCLUDE_DIR + "/gctplus_hip.h", encoding="utf-8").read()
    assert f"#define GCT_STREAM_MAX_ROWS {ops.STREAM_MAX_ROWS}\n" in text
    assert f"#define GCT_STREAM_MAX_LAYERS {ops.STREAM_MAX_LAYERS}\n" in text


def test_stream_argument_validation_without_a_device():
    sp = make_sampler(PscavaetfSampling, "pscavaetf")
    kd = KVDecoder(sp.model, sp.pad_id, sp.sos_id, sp.eos_id)
    n, Le, lat = 3, 10, TINY["latent_dim"]
    z, mask, dconds = torch.zeros(n, Le, lat), torch.ones(n, 1, Le, dtype=torch.bool), torch.zeros(n, 3)
    for rows in (0, ops.STREAM_MAX_ROWS + 1, 2.5):
        with pytest.raises(ValueError):
            kd.start_stream(z, mask, dconds, rows=rows)
    with pytest.raises(ValueError):                                            # a latent the z cross-attention does not take
        kd.start_stream(torch.zeros(n, Le, 6), mask, dconds, rows=2)
    with pytest.raises(ValueError):
        kd.start_stream(z, mask, None, rows=2)                                 # cond2lat without conditions
    for bad_mask in (mask[:2], mask[:, :, :-1]):                              # a flag per item and latent row
        with pytest.raises(ValueError):
            kd.start_stream(z, bad_mask, dconds, rows=2)
    ys0 = torch.ones(n, 5, dtype=torch.long)
    with pytest.raises(ValueError):
        kd.generate_stream(ys0, 10, algo="beam")
    for bad in (torch.tensor([0, 3, 2]), torch.tensor([6, 3, 2]), torch.tensor([5, 3])):
        with pytest.raises(ValueError):
            kd.generate_stream(ys0, 10, prefix_lens=bad)
    for bad in (torch.tensor([0, 3, 2]), torch.tensor([10, 3, 2]), torch.tensor([5, 3]), torch.tensor([1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            kd.generate_stream(ys0, 10, max_new_tokens=bad)
    for kw in (dict(top_k=0), dict(top_p=1.5), dict(temperature=0.0), dict(check_every=0), dict(max_strlen=1)):
        with pytest.raises(ValueError):
            kd.generate_stream(ys0, **dict(dict(max_strlen=10, algo="multinomial"), **kw))
    with pytest.raises(ValueError, match="positional table"):
        kd.generate_stream(torch.ones(n, 150, dtype=torch.long), 80)
    with pytest.raises(ValueError, match="start_stream"):                     # valid arguments, but no pool
        kd.generate_stream(ys0, 10, prefix_lens=torch.tensor([5, 3, 2]), max_new_tokens=torch.tensor([1, 9, 4]))
    # use_cond2dec models keep their condition rows in the caches (prefill writes them): refused
    from gct_plus_amd.Model import model_dict
    c2d = model_dict["pvaetf"](30, 30, dropout=0.0, nconds=3, use_cond2dec=True, use_cond2lat=False, **TINY).eval()
    kc = KVDecoder(c2d, 0, 1, 2)
    with pytest.raises(ValueError, match="cond2dec"):
        kc.start_stream(z, mask, dconds, rows=2)
    with pytest.raises(ValueError, match="cond2dec"):
        kc.generate_stream(ys0, 10)


def test_sampler_stream_rows_validation():
    for bad in (0, ops.STREAM_MAX_ROWS + 1, 1.5):
        with pytest.raises(ValueError):
            make_sampler_rows(PscavaetfSampling, "pscavaetf", "greedy", bad)
    with pytest.raises(ValueError, match="beam"):
        make_sampler_rows(PscavaetfSampling, "pscavaetf", "beam", 8)
    assert make_sampler_rows(PscavaetfSampling, "pscavaetf", "multinomial", 8).stream_rows == 8
    # models the stream refuses are refused in the constructor: use_cond2dec, a latent gct_attn_decode_z does not take
    from gct_plus_amd.Inference.sampling_tool import CvaetfSampling
    from gct_plus_amd.Model import model_dict
    sp = make_sampler(PscavaetfSampling, "pscavaetf")
    c2d = model_dict["pvaetf"](len(sp.SRC), len(sp.TRG), dropout=0.0, nconds=3, use_cond2dec=True, use_cond2lat=False,
                               **TINY).eval()
    with pytest.raises(ValueError, match="cond2dec"):
        CvaetfSampling(c2d, sp.SRC, sp.TRG, latent_dim=TINY["latent_dim"], cond_dim=3, device="cpu", stream_rows=8)
    assert CvaetfSampling(c2d, sp.SRC, sp.TRG, latent_dim=TINY["latent_dim"], cond_dim=3, device="cpu").stream_rows is None
    for lat in (6, 132, 20):                                                  # 20: H * lat = 80 > 2 d_model = 64
        wide = model_dict["pscavaetf"](len(sp.SRC), len(sp.TRG), dropout=0.0, nconds=3, use_cond2lat=True,
                                       **dict(TINY, latent_dim=lat)).eval()
        with pytest.raises(ValueError, match="latent"):
            PscavaetfSampling(wide, sp.SRC, sp.TRG, latent_dim=lat, cond_dim=3, device="cpu", stream_rows=8)
    assert make_sampler(PscavaetfSampling, "pscavaetf").stream_rows is None


def make_sampler_rows(cls, mtype, decode_algo, stream_rows):
    sp = make_sampler(cls, mtype)
    return cls(sp.model, sp.SRC, sp.TRG, latent_dim=TINY["latent_dim"], max_strlen=12, cond_dim=sp.cond_dim,
               decode_algo=decode_algo, toklen_data=[8, 9, 10, 12], device="cpu", beam_size=2, stream_rows=stream_rows)


class FakeKV:
    """Stands in for the sampler's KVDecoder: item i's generated tokens are a function of z row i (so order mistakes
    show), of its own length, written behind its own prefix; records every call."""
    off = 0

    def __init__(self, sp):
        self.sp, self.calls = sp, []
        self.toks = [i for t, i in sp.TRG.stoi.items() if t not in ("<pad>", "<sos>", "<eos>", "<sep>", "<unk>")]

    def tokens(self, z):
        k = int(z.abs().sum() * 1000) % len(self.toks)
        return [self.toks[(k + j) % len(self.toks)] for j in range(2 + k % 4)] + [self.sp.eos_id]

    def start(self, z, src_mask, dconds=None, **kw):
        self.calls.append(("start", dict(kw)))
        self.z = z

    def start_stream(self, z, src_mask, dconds=None, **kw):
        self.calls.append(("start_stream", dict(kw, n=z.shape[0], dconds=dconds, src_mask=src_mask)))
        self.z = z

    def _out(self, ys, max_strlen, prefix_lens):
        n, t0 = ys.shape
        lens = [t0] * n if prefix_lens is None else [int(t) for t in prefix_lens]
        out = torch.full((n, t0 + max_strlen - 1), self.sp.pad_id, dtype=torch.long)
        for r in range(n):
            toks = self.tokens(self.z[r])
            out[r, :lens[r]] = ys[r, :lens[r]]
            out[r, lens[r]:lens[r] + len(toks)] = torch.tensor(toks)
        return out

    def generate(self, ys, max_strlen, prefix_lens=None, **kw):
        self.calls.append(("generate", dict(kw)))
        return self._out(ys, max_strlen, prefix_lens)

    def generate_stream(self, ys, max_strlen, prefix_lens=None, **kw):
        self.calls.append(("generate_stream", dict(kw, prefix_lens=prefix_lens)))
        return self._out(ys, max_strlen, prefix_lens), dict(steps=0)


def test_stream_rows_routes_sample_smiles_and_keeps_the_order():
    base = make_sampler(VaetfSampling, "vaetf")
    n = 9
    z = torch.randn(n, 12, TINY["latent_dim"])
    toklen = [5, 9, 7, 6, 8, 4, 10, 11, 12]
    for rows, algo in ((None, "greedy"), (4, "greedy"), (4, "multinomial"), (16, "greedy")):
        sp = VaetfSampling(base.model, base.SRC, base.TRG, latent_dim=TINY["latent_dim"], max_strlen=12,
                           decode_algo=algo, toklen_data=[8, 9, 10, 12], device="cpu", stream_rows=rows, top_k=5)
        fake = sp.kv = FakeKV(sp)
        smiles, tl, _ = sp.sample_smiles(n, zs=z, toklen=toklen)
        assert smiles == [sp.id_to_smi(fake.tokens(z[r])) for r in range(n)] and tl == toklen
        names = [c[0] for c in fake.calls]
        if rows is None:
            assert names == ["start", "generate"]                              # today's path
            continue
        assert names == ["start_stream", "generate_stream"]
        kw0, kw1 = fake.calls[0][1], fake.calls[1][1]
        assert kw0["rows"] == rows and kw0["n"] == n and kw0["max_total_len"] == 1 + 12
        assert kw1["algo"] == algo and kw1["top_k"] == 5 and kw1["prefix_lens"] is None and kw1["seed"] == sp.seed


def test_stream_rows_routes_sample_multiple_smiles_and_keeps_the_order():
    sp = make_sampler_rows(PscavaetfSampling, "pscavaetf", "greedy", 4)
    fake = sp.kv = FakeKV(sp)
    n = len(SCAFFOLDS)
    z = torch.randn(n, 40, TINY["latent_dim"])
    dconds = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    toklen = [5, 9, 7, 6, 8, 4]
    smiles, tl, _ = sp.sample_multiple_smiles(dconds, SCAFFOLDS, zs=z, toklen=toklen, transform=False)
    sca = [sp.smi_to_id(s) for s in SCAFFOLDS]
    Le = max(len(s) + 1 + t for s, t in zip(sca, toklen))
    assert smiles == [sp.id_to_smi(fake.tokens(z[r, :Le])) for r in range(n)] and tl == toklen
    assert [c[0] for c in fake.calls] == ["start_stream", "generate_stream"]
    assert fake.calls[1][1]["prefix_lens"].tolist() == [len(s) + 2 for s in sca]
    assert torch.equal(fake.calls[0][1]["dconds"], torch.as_tensor(dconds))
    out = fake._out(torch.ones(2, 3, dtype=torch.long), 12, torch.tensor([3, 1]))
    assert generated_tokens(out, torch.tensor([3, 1])).shape == (2, 11)
