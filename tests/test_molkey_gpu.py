"""Molecule identity keys on the device: gct_smiles_key (ops.smiles_key, SmilesKeys.key_rows) against
SmilesKeys.key_reference, exactly, in key and info -- the randomise test's molecules and kept rows in every layout, the
edges of the kernel's LDS record, rows the wrapper cannot vouch for -- keys of spellings made on the device, and the front
ends: Sampling.molecule_keys, Sampling.basic_metrics, MolKeyIndex.from_smiles."""
import itertools

import pytest
import torch

from gct_plus_amd import ops as _ops
from gct_plus_amd.molkey import MolKeyIndex, SmilesKeys, basic_metrics
from tests import molkey_ref as ref
from tests.test_molkey_host import CORPUS
from tests.test_randomize_gpu import RZ, batch
from tests.test_randomize_host import EOS, PAD, PATTERN, SEP, VOCAB, ids_of

pytestmark = pytest.mark.gpu

KEYS = {True: SmilesKeys(VOCAB, PAD, EOS, SEP), False: SmilesKeys(VOCAB, PAD, EOS)}
SENT = -77


@pytest.fixture(scope="module")
def ops():
    _ops._L()
    return _ops


def same(got, want):
    for name, a, b in zip(("key", "info"), got, want):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = (a != b).any(1).nonzero().view(-1).tolist()
        assert not bad, (name, [(r, a[r].tolist(), b[r].tolist()) for r in bad[:3]])


# --------------------------------------------------------------------------------- 1. every layout against the reference
@pytest.mark.parametrize("sep", [False, True], ids=["nosep", "sep"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_rows_equal_the_reference(ops, n, sep):
    """n = 1, 5 and 257 rows (the last workgroup holds one row of four); a strided ys; start 0, 1 and mixed, from the host
    and as an int32 tensor on the device; junk behind the pads of a quarter of the rows."""
    ks = KEYS[sep]
    seen = set()
    for c, mode in enumerate(("zero", "one", "mixed")):
        big, ys, starts = batch(n, sep, mode, c)
        dev = big.cuda()[:, :ys.shape[1]]                          # (the same view on the device: ld = W + 5)
        assert dev.stride(0) > dev.shape[1]
        want = ks.key_reference(ys, starts)
        assert 2 * int((want.info[:, 0] == _ops.KEY_GRAPH).sum()) >= n
        got = ks.key_rows(dev, starts)
        assert got.key.is_cuda and got.key.dtype == torch.int64 and got.info.dtype == torch.int32
        same(got, want)
        same(ks.key_rows(dev, torch.tensor(starts, dtype=torch.int32, device="cuda")), want)
        seen |= set(want.info[:, 0].tolist()) | ({10 + s for s in want.info[:, 1].tolist()} if sep else set())
    if n == 257:
        every = {_ops.KEY_GRAPH, _ops.KEY_STRING_SYNTAX, _ops.KEY_STRING_UNSUPPORTED}
        assert every <= seen and (not sep or {10 + s for s in every} | {9} <= seen)


# --------------------------------------------------------------------------------- 2. the edges of the LDS record
def test_edges_of_the_lds_record(ops):
    """One row each, W = 260, the start that gives the row its span, as an int32 tensor on the device so that a start
    outside [0, W] reaches the kernel; the outputs are the middle of sentinel-filled buffers whose guard rows must stay."""
    ks, W = KEYS[False], 260
    ring = [str(k) if k < 10 else f"%{k}" for k in range(40)]
    G, SY, UN = _ops.KEY_GRAPH, _ops.KEY_STRING_SYNTAX, _ops.KEY_STRING_UNSUPPORTED
    made = [(["C"] * 63, G), (["C"] * 64, G), (["C"] * 65, G), (["C"] * 255, G), (["C"] * 252 + ["O"], G),
            (["C"] + ["(", "C"] * 83 + [")"] * 83, G), (["S"] + ["(", "C", ")"] * 7 + ["C"], G),
            (["S"] + ["(", "C", ")"] * 8 + ["C"], UN), ([t for k in range(40) for t in ("C", ring[k])] * 2, G), ([], SY)]
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
    ys = torch.tensor(rows)
    ys[3, :starts[3]] = torch.randint(0, len(VOCAB), (starts[3],), generator=torch.Generator().manual_seed(1))
    want = ks.key_reference(ys, starts)
    assert want.info[:, 0].tolist() == status
    assert want.info[3].tolist() == [G, -1, 255, 254] and want.info[6].tolist() == [G, -1, 9, 8]
    assert want.info[8].tolist() == [G, -1, 80, 119] and want.info[7].tolist()[2:] == [10, 8]
    assert len(set(want.key[:9, 0].tolist())) == 9 and bool((want.key[10:] == 0).all())
    n = len(rows)
    table, labels = ks.device_tables("cuda")
    key = torch.full((n + 2, 2), SENT, dtype=torch.int64, device="cuda")
    info = torch.full((n + 2, 4), SENT, dtype=torch.int32, device="cuda")
    out = (key[1:n + 1], info[1:n + 1])
    got = ops.smiles_key(ys.cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, -1,
                         out=out)
    assert got[0] is out[0]
    same(got, want)
    for t in (key, info):
        assert bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all())
    with pytest.raises(ValueError):
        ks.key_rows(ys.cuda(), starts)                               # starts on the host are checked there
    with pytest.raises(ValueError):
        ops.smiles_key(ys.cuda(), torch.zeros(3, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, -1)
    with pytest.raises(ValueError):
        ops.smiles_key(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, len(VOCAB))
    empty = ks.key_rows(torch.zeros(0, W, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int64))
    assert empty.key.shape == (0, 2) and empty.info.shape == (0, 4)


def test_sep_and_eos_in_every_slot_of_the_staged_row(ops):
    """n = 5, W = 256, start 0: the <sep> in a lane's fourth slot (position 200), <sep> <eos> in the last two positions,
    a <sep> at 255 with no <eos>, two <sep> (the first one counts) and a <sep> behind the <eos> (none counts)."""
    ks, W, C = KEYS[True], 256, VOCAB.index("C")
    ys = torch.full((5, W), C)
    ys[0, 200], ys[0, 253:] = SEP, torch.tensor([EOS, PAD, PAD])
    ys[1, 254], ys[1, 255] = SEP, EOS
    ys[2, 255] = SEP
    ys[3, 70], ys[3, 130], ys[3, 190:] = SEP, SEP, torch.tensor([EOS] + [PAD] * 65)
    ys[4, 100], ys[4, 200] = EOS, SEP
    want = ks.key_reference(ys, [0] * 5)
    G, SY = _ops.KEY_GRAPH, _ops.KEY_STRING_SYNTAX
    assert want.info.tolist() == [[G, G, 52, 51], [SY, G, 0, 0], [-1, -1, 0, 0], [SY, G, 0, 0], [G, -1, 100, 99]]
    same(ks.key_rows(ys.cuda(), [0] * 5), want)


def test_ids_outside_the_vocabulary(ops):
    """Ids outside [0, V) make a part SYNTAX; its string key tells them apart, as the host statement does."""
    ks, V, C = KEYS[True], len(VOCAB), VOCAB.index("C")
    ys = torch.full((6, 12), PAD)
    ys[:, 0:4] = torch.tensor([C, C, C, EOS])
    ys[1, 1], ys[2, 1], ys[3, 1], ys[4, 1] = -1, V, 2 ** 40, -2 ** 62
    ys[5, 0:8] = torch.tensor([C, V + 3, SEP, C, C, C, C, EOS])
    want = ks.key_reference(ys, [0] * 6)
    assert want.info[:, 0].tolist() == [0, 1, 1, 1, 1, 0] and want.info[5].tolist() == [0, 1, 4, 3]
    assert len(set(want.key[:5, 0].tolist())) == 5
    same(ks.key_rows(ys.cuda(), [0] * 6), want)
    same(ks.key_rows(ys.int()[:3].cuda(), [0] * 3), ks.key_reference(ys[:3], [0] * 3))   # any integer dtype


# --------------------------------------------------------------------------------- 3. spellings made on the device
def test_device_spellings_keep_the_key_and_molecules_stay_apart(ops):
    """8 randomize_rows spellings of each of the 63 corpus molecules: one key per molecule, the host statement's, and
    two molecules share a key exactly when the oracle's backtracking test calls them isomorphic."""
    rz, ks, k = RZ[False], KEYS[False], 8
    toks = [ids_of(s) for s in CORPUS]
    W = max(len(t) for t in toks) + 1
    ys = torch.tensor([t + [EOS] + [PAD] * (W - len(t) - 1) for t in toks]).repeat_interleave(k, 0).cuda()
    n = ys.shape[0]
    spelt = rz.randomize_rows(ys, [0] * n, torch.arange(n), 11, 1.0, out_width=W + 24)
    assert int((spelt.info[:, 0] == _ops.RAND_OK).sum()) == n
    assert int((spelt.tokens[:, :W] != ys).any(1).sum()) >= n // 2
    got = ks.key_rows(spelt.tokens, [0] * n)
    key = got.key[:, 0].view(len(CORPUS), k).cpu()
    assert bool((got.info[:, 0] == _ops.KEY_GRAPH).all()) and bool((key == key[:, :1]).all())
    assert key[:, 0].tolist() == [ks.key(t)[1] for t in toks]
    graphs = [ref.graph(PATTERN.findall(s)) for s in CORPUS]
    for i, j in itertools.combinations(range(len(CORPUS)), 2):
        assert bool(key[i, 0] == key[j, 0]) == ref.isomorphic(graphs[i], graphs[j]), (CORPUS[i], CORPUS[j])


# --------------------------------------------------------------------------------- 4. the front ends
def test_sampler_molecule_keys_metrics_and_index():
    from tests.test_chem_gpu import VOCAB31, tiny_inputs, tiny_sampler
    sp = tiny_sampler(well_formed=True)
    assert sp.keys is sp.keys
    smiles = ["CCO", "OCC", "C(C)O", "c1ccccc1", "C1CC1N", "C[C@@H](N)O", "CC(", "N#N", "c1ccccc1"]
    scaffolds = ["c1ccccc1", "c1ccccc1", "CC", "CO", "C1CC1", "CC", "CC", "C/C=C/C", "C1=CC=CC=C1"]
    ks = sp.keys
    for sca in (None, scaffolds):
        got = sp.molecule_keys(smiles, sca)
        assert got.key.is_cuda and tuple(got.key.shape) == (9, 2)
        for i, s in enumerate(smiles):
            st, key = ks.key(ids_of(s, VOCAB31))
            assert (int(got.info[i, 0]), int(got.key[i, 0])) == (st, key), s
            if sca is not None:
                st, key = ks.key(ids_of(sca[i], VOCAB31))
                assert (int(got.info[i, 1]), int(got.key[i, 1])) == (st, key), sca[i]
            else:
                assert int(got.info[i, 1]) == -1 and int(got.key[i, 1]) == 0
        ids = [(ids_of(c, VOCAB31) + [sp.sep_id] if sca else []) + ids_of(s, VOCAB31) + [sp.eos_id]
               for c, s in zip(sca or smiles, smiles)]
        W = max(len(r) for r in ids) + 3
        rows = torch.tensor([[sp.sos_id] * 2 + r + [sp.pad_id] * (W - 2 - len(r)) for r in ids]).cuda()
        same(sp.molecule_keys((rows, torch.full((9,), 2))), type(got)(got.key.cpu(), got.info.cpu()))
    keys = sp.molecule_keys(smiles).key[:, 0].tolist()
    assert keys[0] == keys[1] == keys[2] and keys[3] == keys[8] and len(set(keys)) == 6
    with pytest.raises(ValueError):
        sp.molecule_keys(smiles, scaffolds[:3])
    # decoded rows, eight of them overwritten with molecules in several spellings
    z, ys0, src_mask, dconds, lens = tiny_inputs()
    _, rows = sp.decode(z, ys0, src_mask, dconds, prefix_lens=lens, return_rows=True)
    ys = rows.ys.clone()
    for r, s in enumerate(("CCO", "OCC", "C(C)O", "C1CC1", "C1CC1", "N#N", "CC(=O)O", "OC(C)=O")):
        ids, t0 = ids_of(s, VOCAB31) + [sp.eos_id], int(rows.prefix_lens[r])
        assert t0 + len(ids) <= ys.shape[1]
        ys[r, t0:] = sp.pad_id
        ys[r, t0:t0 + len(ids)] = torch.tensor(ids, device=ys.device)
    rows = rows._replace(ys=ys)
    same(sp.molecule_keys(rows), ks.key_reference(rows.ys.cpu(), rows.prefix_lens))
    train = ["OCC", "NCC", "C1CC1", "C/C=C/C", "CC("]
    index = MolKeyIndex.from_smiles(sp, train, chunk=2)
    W = max(len(ids_of(s, VOCAB31)) for s in train) + 1
    host_rows = torch.tensor([ids_of(s, VOCAB31) + [sp.eos_id] + [sp.pad_id] * (W - 1 - len(ids_of(s, VOCAB31))) for s in train])
    want_index = MolKeyIndex.from_rows(ks, [(host_rows, [0] * len(train))])
    assert index.keys.is_cuda and torch.equal(index.keys.cpu(), want_index.keys) and len(index) == 3
    assert torch.equal(MolKeyIndex.from_rows(ks, [(host_rows.cuda(), [0] * len(train))]).keys.cpu(), want_index.keys)
    for ix, wx in ((None, None), (index, want_index)):
        got = sp.basic_metrics(rows, ix)
        want = basic_metrics(sp.chemistry.check_reference(rows.ys.cpu(), rows.prefix_lens),
                             ks.key_reference(rows.ys.cpu(), rows.prefix_lens), wx)
        assert got == want, (got, want)
    assert got["n"] == 12 and got["n_valid"] >= 8 and got["n_unique"] <= got["n_valid"] - 4 and "novel" in got
    assert got["n_novel"] <= got["n_unique"] - 2                      # CCO and C1CC1 are in the index
