"""Molecular descriptors on the device.  gct_smiles_desc (ops.smiles_desc, SmilesDescriptors.desc_rows) against
SmilesDescriptors.desc_reference, exactly -- every output is an integer: the randomise test's molecules and kept rows in
every layout, the edges of the kernel's LDS record, rows the wrapper cannot vouch for, spellings made on the device.  And
the front ends: Sampling.descriptors on strings against the known answers, Sampling.property_report against
property_errors of the reference rows, property_reward on the device against the host's, one reinforce_step on it."""
import pytest
import torch

from gct_plus_amd import data, ops as _ops, synthetic
from gct_plus_amd.descriptor import DescRows, SmilesDescriptors, property_errors
from gct_plus_amd.Train.finetune import property_reward, validity_reward
from tests import descriptor_ref as ref
from tests.test_descriptor_host import KNOWN, TPSA_CASES
from tests.test_molkey_host import CORPUS
from tests.test_randomize_gpu import RZ, batch
from tests.test_randomize_host import EOS, PAD, PATTERN, SEP, VOCAB, ids_of

pytestmark = pytest.mark.gpu

DS = {True: SmilesDescriptors(VOCAB, PAD, EOS, SEP), False: SmilesDescriptors(VOCAB, PAD, EOS)}
SENT = -77


@pytest.fixture(scope="module")
def ops():
    _ops._L()
    return _ops


def same(got, want):
    a, b = got.values.cpu(), want.values
    assert a.dtype == b.dtype == torch.int32 and a.shape == b.shape
    bad = (a != b).any(1).nonzero().view(-1).tolist()
    assert not bad, [(r, a[r].tolist(), b[r].tolist()) for r in bad[:3]]


# --------------------------------------------------------------------------------- 1. every layout against the reference
@pytest.mark.parametrize("sep", [False, True], ids=["nosep", "sep"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_rows_equal_the_reference(ops, n, sep):
    """n = 1, 5 and 257 rows (the last workgroup holds one row of four); a strided ys; start 0, 1 and mixed, from the host
    and as an int32 tensor on the device; junk in front of the start and behind the pads of a quarter of the rows."""
    ds = DS[sep]
    seen = set()
    for c, mode in enumerate(("zero", "one", "mixed")):
        big, ys, starts = batch(n, sep, mode, c)
        dev = big.cuda()[:, :ys.shape[1]]                          # (the same view on the device: ld = W + 5)
        assert dev.stride(0) > dev.shape[1]
        want = ds.desc_reference(ys, starts)
        assert 4 * int((want.status == _ops.DESC_OK).sum()) >= n
        got = ds.desc_rows(dev, starts)
        assert got.values.is_cuda and got.values.dtype == torch.int32
        same(got, want)
        same(ds.desc_rows(dev, torch.tensor(starts, dtype=torch.int32, device="cuda")), want)
        seen |= set(want.status.tolist())
    if n == 257:
        assert {_ops.DESC_OK, _ops.DESC_SYNTAX, _ops.DESC_UNSUPPORTED} <= seen


def test_edges_of_the_lds_record(ops):
    """One row each, W = 260, the start that gives the row its span, as an int32 tensor on the device so that a start
    outside [0, W] reaches the kernel; the output is the middle of a sentinel-filled buffer whose guard rows must stay."""
    ds, W = DS[False], 260
    ring = [str(k) if k < 10 else f"%{k}" for k in range(40)]
    OK, SY, UN, UK = _ops.DESC_OK, _ops.DESC_SYNTAX, _ops.DESC_UNSUPPORTED, _ops.DESC_UNKNOWN_ATOM
    cubane = ["C", "1", "2", "C", "3", "C", "4", "C", "1", "C", "5", "C", "2", "C", "3", "C", "4", "5"]
    made = [(["C"] * 63, OK), (["C"] * 64, OK), (["C"] * 65, OK), (["C"] * 255, OK),            # 3: 254 bonds
            (["C", "1"] + ["C"] * 251 + ["C", "1"], OK),                                        # 4: a ring of 253 atoms
            (["c", "1"] + ["c"] * 251 + ["n", "1"], OK),                                        # 5: ... all of it aromatic
            (cubane, OK), (["C"] + ["(", "C"] * 83 + [")"] * 83, OK),                           # 6, 7
            (["S"] + ["(", "C", ")"] * 7 + ["C"], OK), (["S"] + ["(", "C", ")"] * 8 + ["C"], UN),  # 8, 9
            ([t for k in range(40) for t in ("C", ring[k])] * 2, OK),                           # 10: 40 rings open at once
            (["N"] + ["C"] * 252 + ["O"], OK), (["C"] * 100 + ["*"], UK), ([], SY)]             # 11, 12, 13
    rows, starts, status = [], [], []
    for toks, st in made:
        ids = [VOCAB.index(t) for t in toks] + [EOS]
        rows.append([PAD] * (W - len(ids)) + ids)
        starts.append(W - len(ids))
        status.append(st)
    C = VOCAB.index("C")
    rows += [[C] * W, [PAD] * W, rows[0], rows[0], rows[0], rows[0]]   # a span of exactly 256 without <eos>; an empty span
    starts += [4, W, -1, W + 1, -2 ** 31, 3]                        # ... starts outside [0, W]; a span wider than 256
    status += [-1] * 6
    bad_id = list(rows[1])
    bad_id[W - 10] = len(VOCAB)                                     # a token id outside [0, V)
    rows.append(bad_id), starts.append(starts[1]), status.append(SY)
    ys = torch.tensor(rows)
    ys[3, :starts[3]] = torch.randint(0, len(VOCAB), (starts[3],), generator=torch.Generator().manual_seed(1))
    want = ds.desc_reference(ys, starts)
    v = want.values
    assert want.status.tolist() == status
    assert v[3].tolist() == [OK, 255, 512, 255 * 12011 + 512 * 1008, 0, 0, 0, 252, 0, 0, 0, 0]
    assert v[4].tolist() == [OK, 253, 506, 253 * 14027, 0, 0, 0, 0, 1, 0, 0, 253]
    assert v[5].tolist() == [OK, 253, 252, 252 * 13019 + 14007, 0, 0, 1, 0, 1, 1, 1289, 253]
    assert v[6].tolist() == [OK] + list(KNOWN[-1][1]) and KNOWN[-1][0] == "C12C3C4C1C5C2C3C45"
    assert v[7].tolist()[:3] == [OK, 84, 170] and v[8].tolist()[:3] == [OK, 9, 24] and v[9].tolist() == [UN, 10] + [0] * 10
    assert v[10].tolist()[7:] == [0, 40, 0, 0, 119] and v[11].tolist()[5:8] == [2, 2, 251]
    assert v[12].tolist() == [UK, 101] + [0] * 10 and not bool(v[13:, 1:].any())
    n = len(rows)
    table, desc = ds.device_tables("cuda")
    buf = torch.full((n + 2, 12), SENT, dtype=torch.int32, device="cuda")
    out = buf[1:n + 1]
    got = ops.smiles_desc(ys.cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda"), table, desc, PAD, EOS, -1,
                          out=out)
    assert got is out
    same(DescRows(got), want)
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    with pytest.raises(ValueError):
        ds.desc_rows(ys.cuda(), starts)                              # starts on the host are checked there
    with pytest.raises(ValueError):
        ops.smiles_desc(ys.cuda(), torch.zeros(3, dtype=torch.int32, device="cuda"), table, desc, PAD, EOS, -1)
    with pytest.raises(ValueError):
        ops.smiles_desc(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, desc, PAD, EOS, len(VOCAB))
    with pytest.raises(ValueError):
        ops.smiles_desc(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, desc[:-1], PAD, EOS, -1)
    with pytest.raises(ValueError):
        ops.smiles_desc(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, desc, PAD, EOS, -1,
                        out=buf[:n, :8])
    empty = ds.desc_rows(torch.zeros(0, W, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int64))
    assert empty.values.shape == (0, 12)


def test_device_spellings_keep_every_column(ops):
    """8 randomize_rows spellings of each corpus molecule that has descriptors, and of the known answers: one row of
    figures per molecule, the host statement's and the oracle's."""
    rz, ds, k = RZ[False], DS[False], 8
    smiles = [s for s, _ in KNOWN] + ["c1ccccc1c1ccccc1", "c1ccccc1-c1ccncc1"] + CORPUS
    toks = [t for t in (ids_of(s) for s in smiles) if ds.describe(t)[0] == _ops.DESC_OK]
    assert len(toks) >= 40
    W = max(len(t) for t in toks) + 1
    ys = torch.tensor([t + [EOS] + [PAD] * (W - len(t) - 1) for t in toks]).repeat_interleave(k, 0).cuda()
    n = ys.shape[0]
    spelt = rz.randomize_rows(ys, [0] * n, torch.arange(n), 11, 1.0, out_width=W + 24)
    assert int((spelt.info[:, 0] == _ops.RAND_OK).sum()) == n
    assert int((spelt.tokens[:, :W] != ys).any(1).sum()) >= n // 2
    got = ds.desc_rows(spelt.tokens, [0] * n).values.view(len(toks), k, 12).cpu()
    assert bool((got == got[:, :1]).all())
    assert got[:, 0].tolist() == [ds.describe(t) for t in toks] == [ref.describe([VOCAB[i] for i in t]) for t in toks]


# --------------------------------------------------------------------------------- 2. known answers and the front ends
def chem_sampler():
    """A PscavaetfSampling over the tiny config with synthetic.CHEM_VOCAB as its target vocabulary (strings only)."""
    from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling
    from gct_plus_amd.Model import model_dict
    from tests.test_chem_gpu import TINY
    nc = synthetic.n_conds("pscavaetf")
    TRG = data.Vocab(list(synthetic.CHEM_VOCAB))
    SRC = data.Vocab([t for t in synthetic.CHEM_VOCAB if t not in ("<sos>", "<eos>")])
    torch.manual_seed(3)
    model = model_dict["pscavaetf"](len(SRC), len(TRG), dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
    return PscavaetfSampling(model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=12, cond_dim=nc,
                             decode_algo="multinomial", seed=5)


def test_known_answers_on_the_device():
    sp = chem_sampler()
    assert sp.describer is sp.describer and sp.describer.keys is sp.keys
    smiles = [s for s, _ in KNOWN] + ["C[N+](C)(C)C", "CCCC", "CC#CC", "c1ccccc1c1ccccc1", "c1ccccc1-c1ccccc1", "C/C=C/C",
                                      "CC(", "C*"]
    got = sp.descriptors(smiles)
    assert got.values.is_cuda and tuple(got.values.shape) == (len(smiles), 12)
    v = got.values.cpu()
    for i, (s, want) in enumerate(KNOWN):
        assert v[i].tolist() == [_ops.DESC_OK] + list(want), s
    k = len(KNOWN)
    assert (int(v[k, 4]), int(v[k, 10]), int(v[k, 2])) == (1, 0, 12) and int(v[k + 1, 7]) == 1 and int(v[k + 2, 7]) == 0
    assert v[k + 3].tolist() == v[k + 4].tolist() and v[k + 3].tolist()[7:] == [1, 2, 2, 0, 12]
    assert v[k + 5:, 0].tolist() == [_ops.DESC_UNSUPPORTED, _ops.DESC_SYNTAX, _ops.DESC_UNKNOWN_ATOM]
    assert got.mw[1].item() == pytest.approx(180.159) and got.tpsa[1].item() == pytest.approx(63.60)
    tp = [s for s, _ in TPSA_CASES if all(t in synthetic.CHEM_VOCAB for t in PATTERN.findall(s))]
    assert len(tp) >= 24
    assert sp.descriptors(tp).tpsa_centi.tolist() == [dict(TPSA_CASES)[s] for s in tp]


def test_report_reward_and_one_policy_step():
    from gct_plus_amd.Train.finetune import reinforce_step
    from tests.test_chem_gpu import VOCAB31, tiny_inputs, tiny_sampler
    from tests.test_ppo_gpu import fused_adam
    sp = tiny_sampler(well_formed=True)
    z, ys0, src_mask, dconds, lens = tiny_inputs()
    _, rows = sp.decode(z, ys0, src_mask, dconds, prefix_lens=lens, return_rows=True)
    ys = rows.ys.clone()
    for r, s in enumerate(("CCO", "OCC", "CC(N)=O", "C1CC1", "NCCO", "N#N", "CC(=O)O", "OC(C)=O")):
        ids, t0 = ids_of(s, VOCAB31) + [sp.eos_id], int(rows.prefix_lens[r])
        assert t0 + len(ids) <= ys.shape[1]
        ys[r, t0:] = sp.pad_id
        ys[r, t0:t0 + len(ids)] = torch.tensor(ids, device=ys.device)
    rows = rows._replace(ys=ys)
    n = ys.shape[0]
    host = sp.describer.desc_reference(rows.ys.cpu(), rows.prefix_lens)
    dev = sp.descriptors(rows)
    same(dev, host)
    same(sp.descriptors((rows.ys, rows.prefix_lens)), host)
    assert int(host.ok.sum()) >= 8 and host.tpsa_centi[:3].tolist() == [2023, 2023, 4309]
    # property_report against property_errors of the reference rows
    valid = sp.chemistry.check_reference(rows.ys.cpu(), rows.prefix_lens).status == _ops.CHEM_OK
    targets = {"tpsa": torch.linspace(20.0, 60.0, n), "mw": 60.0, "hbd": 1, "rings": torch.ones(n)}
    for valid_only in (True, False):
        got = sp.property_report(rows, targets, valid_only=valid_only)
        want = property_errors(host, targets, valid if valid_only else None)
        assert list(got) == list(targets) and got["tpsa"]["n"] >= 8
        for name in targets:
            assert got[name]["n"] == want[name]["n"]
            for k, x in want[name].items():
                assert got[name][k] == pytest.approx(x, rel=1e-12, abs=1e-12), (name, k)
    # property_reward on the device against the host's, bit for bit
    mixed = torch.linspace(10.0, 70.0, n)
    for name, target, tol in (("tpsa", 40.0, 25.0), ("tpsa", mixed, 30.0), ("mw", 60.0, 40.0), ("hbd", 1, 2)):
        a = property_reward(dev, name, target.cuda() if torch.is_tensor(target) else target, tol)
        b = property_reward(host, name, target, tol)
        assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a.cpu(), b), name
    # one reinforce_step on validity_reward * property_reward runs and changes parameters
    reward = validity_reward(sp.check_rows(rows)) * property_reward(dev, "tpsa", mixed.cuda(), 60.0)
    assert reward.is_cuda and reward.dtype == torch.float32 and float(reward.max()) > 0.0
    start = {k: p.detach().clone() for k, p in sp.model.named_parameters()}
    stats = reinforce_step(sp, fused_adam(sp.model), rows, reward)
    assert stats["mean_reward"] > 0.0
    assert any(not torch.equal(p.detach(), start[k]) for k, p in sp.model.named_parameters())
