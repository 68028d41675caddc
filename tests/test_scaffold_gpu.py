"""Murcko scaffolds on the device: gct_smiles_scaffold (ops.smiles_scaffold, SmilesScaffolds.scaffold_rows) against
SmilesScaffolds.scaffold_reference, exactly, in tokens, key, info and member -- the randomise test's molecules and kept
rows in every layout, the edges of the kernel's LDS record, rows the wrapper cannot vouch for -- the match of a molecule
with the scaffold it was given, agreement with gct_smiles_key on the kernel's own spellings, and the front ends:
Sampling.scaffold_report on a tiny scavaetf decode, Sampling.murcko_scaffolds, scaffold_metrics, scaffold_reward."""
import pytest
import torch

from gct_plus_amd import data, ops as _ops, synthetic
from gct_plus_amd.smiles import ChemReport
from gct_plus_amd.molkey import scaffold_metrics
from gct_plus_amd.scaffold import ScaffoldRows, SmilesScaffolds, scaffold_match
from gct_plus_amd.Train.finetune import scaffold_reward
from tests.test_randomize_gpu import RZ, batch
from tests.test_randomize_host import EOS, PAD, SEP, VOCAB, ids_of
from tests.test_scaffold_host import TABLE

pytestmark = pytest.mark.gpu

SCAS = {True: SmilesScaffolds(VOCAB, PAD, EOS, SEP), False: SmilesScaffolds(VOCAB, PAD, EOS)}
SENT = -77
NAMES = ("tokens", "key", "info", "member")


@pytest.fixture(scope="module")
def ops():
    _ops._L()
    return _ops


def same(got, want):
    for name, a, b in zip(NAMES, got, want):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = (a != b).any(1).nonzero().view(-1).tolist()
        assert not bad, (name, [(r, a[r].tolist(), b[r].tolist()) for r in bad[:3]])


def launch(ops, sc, ys, start, out_width=None, out=None):
    table, labels = sc.keys.device_tables("cuda")
    rz = sc.randomizer
    none = lambda v: -1 if v is None else v                        # noqa: E731
    return ops.smiles_scaffold(ys, start, table, labels, rz.device_tables("cuda")[1], len(rz.ring_ids), rz.open_id,
                               rz.close_id, PAD, EOS, none(sc.sep_id), none(sc.n_id), none(sc.nh_id), out_width, out=out)


# --------------------------------------------------------------------------------- 1. every layout against the reference
@pytest.mark.parametrize("sep", [False, True], ids=["nosep", "sep"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_rows_equal_the_reference(ops, n, sep):
    """n = 1, 5 and 257 rows (the last workgroup holds one row of four); a strided ys; start 0, 1 and mixed, from the host
    and as an int32 tensor on the device; junk behind the pads of a quarter of the rows."""
    sc = SCAS[sep]
    seen, subst, shell = set(), 0, 0
    for c, mode in enumerate(("zero", "one", "mixed")):
        big, ys, starts = batch(n, sep, mode, c)
        dev = big.cuda()[:, :ys.shape[1]]                          # (the same view on the device: ld = W + 5)
        assert dev.stride(0) > dev.shape[1]
        want = sc.scaffold_reference(ys, starts)
        got = sc.scaffold_rows(dev, starts)
        assert isinstance(got, ScaffoldRows) and all(t.is_cuda for t in got)
        same(got, want)
        same(sc.scaffold_rows(dev, torch.tensor(starts, dtype=torch.int32, device="cuda")), want)
        seen |= set(want.info[:, 0].tolist()) | ({10 + s for s in want.info[:, 1].tolist()} if sep else set())
        subst += int(((want.tokens == sc.nh_id).sum(1) > 0).sum())
        shell += int(((want.member == 2).sum(1) > 0).sum())
        if n == 257:
            assert 2 * int((want.info[:, 0] == _ops.SCA_OK).sum()) >= n
    if n == 257:
        assert {_ops.SCA_OK, _ops.SCA_ACYCLIC, _ops.SCA_SYNTAX, _ops.SCA_UNSUPPORTED} <= seen and subst and shell
        assert not sep or {10 + s for s in (_ops.KEY_GRAPH, _ops.KEY_STRING_SYNTAX, _ops.KEY_STRING_UNSUPPORTED)} | {9} <= seen


def test_out_width_and_too_long(ops):
    """The spelling in rows narrower and wider than the input: TOO_LONG where it and its <eos> do not fit."""
    sc = SCAS[False]
    rows = [ids_of(s) for s in ("Cc1ccccc1", "CC(C)(C)c1ccc(O)cc1", "c1ccccc1-c1ccccc1", "CCO", "Cn1cccc1")]
    W = max(len(r) for r in rows) + 1
    ys = torch.tensor([r + [EOS] + [PAD] * (W - len(r) - 1) for r in rows])
    seen = set()
    for width in (1, 6, 8, 9, W, W + 7):
        want = sc.scaffold_reference(ys, [0] * 5, out_width=width)
        same(sc.scaffold_rows(ys.cuda(), [0] * 5, out_width=width), want)
        seen |= set(want.info[:, 0].tolist())
    assert {_ops.SCA_OK, _ops.SCA_TOO_LONG, _ops.SCA_ACYCLIC} <= seen


# --------------------------------------------------------------------------------- 2. the edges of the LDS record
def test_edges_of_the_lds_record(ops):
    """One row each, W = 260, the start that gives the row its span, as an int32 tensor on the device so that a start
    outside [0, W] reaches the kernel; the outputs are the middle of sentinel-filled buffers whose guard rows must stay."""
    sc, W = SCAS[False], 260
    ring = [str(k) if k < 10 else f"%{k}" for k in range(40)]
    OK, AC, SY, UN = _ops.SCA_OK, _ops.SCA_ACYCLIC, _ops.SCA_SYNTAX, _ops.SCA_UNSUPPORTED
    made = [(["C"] * 63, AC), (["C"] * 64, AC), (["C"] * 65, AC), (["C"] * 255, AC),
            (["C", "1"] + ["C"] * 251 + ["C", "1"], OK),                                  # 253 ring atoms, 255 tokens
            (["C"] + ["(", "C"] * 83 + ["1", "C", "C", "1"] + [")"] * 83, OK),             # a cyclopropane at depth 83
            (["S", "1"] + ["(", "C", ")"] * 6 + ["C", "C", "1"], OK),                      # 8 bonds, two of them in a ring
            (["S", "1"] + ["(", "C", ")"] * 7 + ["C", "C", "1"], UN),                      # a ninth
            ([t for k in range(40) for t in ("C", ring[k])] * 2, OK),                      # 40 rings open at once
            (["C"] * 100 + ["c", "1", "c", "c", "n", "(", "C", ")", "c", "1"] + ["C"] * 100, OK), ([], SY)]
    rows, starts, status = [], [], []
    for toks, st in made:
        ids = [VOCAB.index(t) for t in toks] + [EOS]
        rows.append([PAD] * (W - len(ids)) + ids)
        starts.append(W - len(ids))
        status.append(st)
    C = VOCAB.index("C")
    rows += [[C] * W, [PAD] * W, rows[4], rows[4], rows[4], rows[4]]   # a span of exactly 256 without <eos>; an empty span
    starts += [4, W, -1, W + 1, -2 ** 31, 3]                        # ... starts outside [0, W]; a span wider than 256
    status += [-1] * 6
    ys = torch.tensor(rows)
    ys[3, :starts[3]] = torch.randint(0, len(VOCAB), (starts[3],), generator=torch.Generator().manual_seed(1))
    want = sc.scaffold_reference(ys, starts)
    assert want.info[:, 0].tolist() == status
    assert want.info[4].tolist() == [OK, -1, 253, 255] and want.tokens[4, :256].tolist() == rows[4][W - 256:]
    assert want.info[5].tolist() == [OK, -1, 3, 5] and want.member[5, :87].tolist() == [0] * 83 + [1] * 3 + [-1]
    assert want.info[6].tolist() == [OK, -1, 3, 5] and want.info[8].tolist() == [OK, -1, 80, 160]
    assert want.info[9].tolist() == [OK, -1, 5, 7] and VOCAB.index("[nH]") in want.tokens[9].tolist()
    assert bool((want.key[[0, 1, 2, 3, 7, 10], 0] == 0).all()) and bool((want.key[11:] == 0).all())
    assert bool((want.member[3, :255] == 0).all()) and bool((want.member[11:] == -1).all())
    n = len(rows)
    bufs = [torch.full((n + 2, w), SENT, dtype=d, device="cuda")
            for w, d in ((W, torch.int64), (2, torch.int64), (4, torch.int32), (W, torch.int32))]
    out = tuple(b[1:n + 1] for b in bufs)
    got = launch(ops, sc, ys.cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda"), out=out)
    assert got[0] is out[0]
    same(got, want)
    for t in bufs:
        assert bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all())
    with pytest.raises(ValueError):
        sc.scaffold_rows(ys.cuda(), starts)                          # starts on the host are checked there
    with pytest.raises(ValueError):
        launch(ops, sc, ys.cuda(), torch.zeros(3, dtype=torch.int32, device="cuda"))
    table, labels = sc.keys.device_tables("cuda")
    with pytest.raises(ValueError):
        ops.smiles_scaffold(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, labels,
                            sc.randomizer.device_tables("cuda")[1], len(sc.randomizer.ring_ids), sc.randomizer.open_id,
                            sc.randomizer.close_id, PAD, EOS, -1, len(VOCAB), sc.nh_id)
    empty = sc.scaffold_rows(torch.zeros(0, W, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int64))
    assert [tuple(t.shape) for t in empty] == [(0, W), (0, 2), (0, 4), (0, W)]


def test_ids_outside_the_vocabulary_and_no_nh_token(ops):
    sc, V, C = SCAS[True], len(VOCAB), VOCAB.index("C")
    ring = ids_of("C1CC1")
    ys = torch.full((5, 14), PAD)
    ys[:, 0:6] = torch.tensor(ring + [EOS])
    ys[1, 1], ys[2, 2], ys[3, 0] = -1, V, 2 ** 40
    ys[4, 0:9] = torch.tensor([C, V + 3, SEP] + ring + [EOS])
    want = sc.scaffold_reference(ys, [0] * 5)
    assert want.info[:, 0].tolist() == [0, 2, 2, 2, 0] and want.info[4].tolist() == [0, _ops.KEY_STRING_SYNTAX, 3, 5]
    same(sc.scaffold_rows(ys.cuda(), [0] * 5), want)
    same(sc.scaffold_rows(ys.int()[:3].cuda(), [0] * 3), sc.scaffold_reference(ys[:3], [0] * 3))   # any integer dtype
    vocab = [t for t in VOCAB if t != "[nH]"]
    bare = SmilesScaffolds(vocab, vocab.index(VOCAB[PAD]), vocab.index(VOCAB[EOS]))
    rows = [ids_of(s, vocab) for s in ("Cn1cccc1", "c1ccn(-c2ccccc2)c1", "Cc1ccccc1")]
    W = max(len(r) for r in rows) + 1
    ys = torch.tensor([r + [bare.eos_id] + [bare.pad_id] * (W - len(r) - 1) for r in rows])
    want = bare.scaffold_reference(ys, [0] * 3)
    assert want.info[:, 0].tolist() == [_ops.SCA_NO_TOKEN, _ops.SCA_OK, _ops.SCA_OK] and want.info[0].tolist()[2:] == [5, 0]
    same(bare.scaffold_rows(ys.cuda(), [0] * 3), want)


# --------------------------------------------------------------------------------- 3. the match with the given scaffold
def test_match_with_the_true_a_respelled_and_a_wrong_scaffold(ops):
    """Rows `scaffold <sep> molecule <eos>` from the hand table: the true scaffold, the true scaffold in a spelling made by
    the device randomiser, and another molecule's scaffold: match is True, True, False."""
    sc, rz = SCAS[True], RZ[True]
    cases = [(ids_of(m), ids_of(s)) for m, st, s, _ in TABLE if st == _ops.SCA_OK]
    W = max(len(s) for _, s in cases) + 25
    sca_rows = torch.tensor([s + [EOS] + [PAD] * (W - len(s) - 1) for _, s in cases]).cuda()
    spelt = rz.randomize_rows(sca_rows, [0] * len(cases), torch.arange(len(cases)), 3, 1.0)
    assert int((spelt.info[:, 0] == _ops.RAND_OK).sum()) == len(cases)
    respelled = [r[:r.index(EOS)] for r in spelt.tokens.cpu().tolist()]
    assert sum(r != s for r, (_, s) in zip(respelled, cases)) >= len(cases) // 2
    rows, want_match = [], []
    for i, (mol, true) in enumerate(cases):
        wrong = next(s for _, s in cases[i + 1:] + cases[:i] if sc.keys.key(s) != sc.keys.key(true))
        rows += [true + [SEP] + mol, respelled[i] + [SEP] + mol, wrong + [SEP] + mol]
        want_match += [True, True, False]
    W = max(len(r) for r in rows) + 2
    ys = torch.tensor([[PAD] + r + [EOS] + [PAD] * (W - len(r) - 2) for r in rows])
    want = sc.scaffold_reference(ys, [1] * len(rows))
    got = sc.scaffold_rows(ys.cuda(), [1] * len(rows))
    same(got, want)
    assert scaffold_match(got).tolist() == want_match == scaffold_match(want).tolist()
    assert scaffold_reward(got).tolist() == [float(m) for m in want_match] and scaffold_reward(got).is_cuda
    ok = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
    got_metrics = scaffold_metrics(ChemReport(ok, ok, ok, ok), got, sc.keys.key_rows(ys.cuda(), [1] * len(rows)))
    assert got_metrics["same_scaffold"] == 2 / 3 and got_metrics["n_same"] == 2 * len(cases)
    assert got_metrics["n_scaffolds"] == len({sc.keys.key(s) for _, s in cases})
    assert got_metrics == scaffold_metrics(ChemReport(*(ok.cpu(),) * 4), want, sc.keys.key_reference(ys, [1] * len(rows)))


def test_agreement_with_the_key_kernel_on_its_own_spellings(ops):
    """key[:, 0] of scaffold_rows(x) is what gct_smiles_key makes of scaffold_rows' own output tokens, and the scaffold
    of those tokens is the same row again."""
    sc = SCAS[False]
    _, ys, starts = batch(257, False, "mixed", 2)
    got = sc.scaffold_rows(ys.cuda(), starts)
    ok = got.info[:, 0] == _ops.SCA_OK
    keyed = sc.keys.key_rows(got.tokens, [0] * 257)
    assert int(ok.sum()) >= 128 and bool((keyed.info[:, 0][ok] == _ops.KEY_GRAPH).all())
    assert torch.equal(keyed.key[:, 0][ok], got.key[:, 0][ok])
    assert torch.equal(keyed.info[:, 2][ok], got.info[:, 2][ok])
    again = sc.scaffold_rows(got.tokens, [0] * 257)
    assert torch.equal(again.tokens[ok], got.tokens[ok]) and torch.equal(again.key[:, 0][ok], got.key[:, 0][ok])


# --------------------------------------------------------------------------------- 4. the front ends
def test_sampler_scaffold_report_and_murcko_scaffolds():
    from gct_plus_amd.Inference.sampling_tool import ScaVaeSampling
    from gct_plus_amd.Model import model_dict
    from tests.test_chem_host import VOCAB31
    from tests.test_mixed_scaffold_decode_gpu import TINY
    TRG = data.Vocab(VOCAB31)
    SRC = data.Vocab([t for t in VOCAB31 if t not in ("<sos>", "<eos>")])
    torch.manual_seed(21)
    model = model_dict["scavaetf"](len(SRC), len(TRG), dropout=0.0, nconds=synthetic.n_conds("scavaetf"), **TINY).cuda().eval()
    sp = ScaVaeSampling(model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=14, cond_dim=0,
                        decode_algo="multinomial", seed=5, well_formed=True)
    assert sp.scaffolds is sp.scaffolds
    given = ["c1ccccc1", "C1CC1", "CC", "c1ccccc1", "C1CC1", "c1cc[nH]c1", "C1CC1", "c1ccccc1"]
    *_, rows = sp.sample_multiple_smiles(given, toklen=[12] * 8, return_rows=True)
    ys = rows.ys.clone()
    for r, s in enumerate(("Cc1ccccc1", "NC1CC1", "CCO", "C1CCCCC1")):             # four rows with known molecules
        ids, t0 = ids_of(s, VOCAB31) + [sp.eos_id], int(rows.prefix_lens[r])
        assert t0 + len(ids) <= ys.shape[1]
        ys[r, t0:] = sp.pad_id
        ys[r, t0:t0 + len(ids)] = torch.tensor(ids, device=ys.device)
    rows = rows._replace(ys=ys)
    got = sp.scaffold_report(rows)
    want = sp.scaffolds.scaffold_reference(rows.ys.cpu(), [1] * 8)
    same(got, want)
    assert scaffold_match(got).tolist()[:4] == [True, True, False, False]
    assert bool((got.info[:, 1] == _ops.KEY_GRAPH).all())                              # every row holds its given scaffold
    report = sp.check_rows(rows)
    metrics = scaffold_metrics(report, got, sp.molecule_keys(rows))
    assert metrics == scaffold_metrics(sp.chemistry.check_reference(rows.ys.cpu(), rows.prefix_lens), want,
                                       sp.keys.key_reference(rows.ys.cpu(), rows.prefix_lens))
    assert metrics["n"] == 8 and metrics["n_same"] >= 2
    # murcko_scaffolds: the molecule behind the prefix, and strings
    strings, sca = sp.murcko_scaffolds(rows)
    same(sca, sp.scaffolds.scaffold_reference(rows.ys.cpu(), rows.prefix_lens))
    assert strings[:4] == ["c1ccccc1", "C1CC1", "", "C1CCCCC1"]
    strings, sca = sp.murcko_scaffolds(["Cc1ccccc1", "CCO", "Cn1cccc1", "CC(", "O=C1CCCCC1C"])
    assert strings == ["c1ccccc1", "", "[nH]1cccc1", "", "O=C1CCCCC1"]
    assert sca.info[:, 0].tolist() == [_ops.SCA_OK, _ops.SCA_ACYCLIC, _ops.SCA_OK, _ops.SCA_SYNTAX, _ops.SCA_OK]
