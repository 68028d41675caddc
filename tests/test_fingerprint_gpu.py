"""Circular fingerprints and Tanimoto aggregates on the device.  gct_smiles_fp (ops.smiles_fp,
SmilesFingerprints.fp_rows) against SmilesFingerprints.fp_reference, exactly, in bits and info -- the randomise test's
molecules and kept rows in every layout, the edges of the kernel's LDS record, rows the wrapper cannot vouch for,
spellings made on the device.  gct_fp_tanimoto (ops.fp_tanimoto, tanimoto_agg) against tanimoto_reference: best and arg
exactly, total within m * 2^-53 * total -- every term of the sum is exact in fp64 (an fp32 quotient, or the product of
two), so only the order of at most m fp64 additions can differ, each of which rounds by at most 2^-53 of a partial sum
that never exceeds the total (the terms are not negative).  And the front ends: Sampling.fingerprints, basic_metrics with
int_div, Sampling.snn, FingerprintIndex.from_smiles."""
import pytest
import torch

from gct_plus_amd import ops as _ops
from gct_plus_amd.fingerprint import (FingerprintIndex, FpRows, SmilesFingerprints, internal_diversity, snn, tanimoto_agg,
                                      tanimoto_reference)
from tests import fingerprint_ref as ref
from tests.test_molkey_host import CORPUS
from tests.test_randomize_gpu import RZ, batch
from tests.test_randomize_host import EOS, PAD, PATTERN, SEP, VOCAB, ids_of

pytestmark = pytest.mark.gpu

FPS = {True: SmilesFingerprints(VOCAB, PAD, EOS, SEP), False: SmilesFingerprints(VOCAB, PAD, EOS)}
SENT = -77


@pytest.fixture(scope="module")
def ops():
    _ops._L()
    return _ops


def same(got, want):
    for name, a, b in zip(("bits", "info"), got, want):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = (a != b).any(1).nonzero().view(-1).tolist()
        assert not bad, (name, [(r, a[r].tolist(), b[r].tolist()) for r in bad[:3]])


# --------------------------------------------------------------------------------- 1. gct_smiles_fp: every layout
@pytest.mark.parametrize("sep", [False, True], ids=["nosep", "sep"])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_rows_equal_the_reference(ops, n, sep):
    """n = 1, 5 and 257 rows (the last workgroup holds one row of four); a strided ys; start 0, 1 and mixed, from the host
    and as an int32 tensor on the device; junk behind the pads of a quarter of the rows."""
    fs = FPS[sep]
    seen = set()
    for c, mode in enumerate(("zero", "one", "mixed")):
        big, ys, starts = batch(n, sep, mode, c)
        dev = big.cuda()[:, :ys.shape[1]]                          # (the same view on the device: ld = W + 5)
        assert dev.stride(0) > dev.shape[1]
        want = fs.fp_reference(ys, starts)
        assert 2 * int((want.info[:, 0] == _ops.FP_GRAPH).sum()) >= n
        got = fs.fp_rows(dev, starts)
        assert got.bits.is_cuda and got.bits.dtype == torch.int64 and got.info.dtype == torch.int32
        same(got, want)
        same(fs.fp_rows(dev, torch.tensor(starts, dtype=torch.int32, device="cuda")), want)
        seen |= set(want.info[:, 0].tolist())
    if n == 257:
        assert {_ops.FP_GRAPH, _ops.FP_SYNTAX, _ops.FP_UNSUPPORTED} <= seen


def test_edges_of_the_lds_record(ops):
    """One row each, W = 260, the start that gives the row its span, as an int32 tensor on the device so that a start
    outside [0, W] reaches the kernel; the outputs are the middle of sentinel-filled buffers whose guard rows must stay."""
    fs, W = FPS[False], 260
    ring = [str(k) if k < 10 else f"%{k}" for k in range(40)]
    G, SY, UN = _ops.FP_GRAPH, _ops.FP_SYNTAX, _ops.FP_UNSUPPORTED
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
    want = fs.fp_reference(ys, starts)
    assert want.info[:, 0].tolist() == status
    assert want.info[3].tolist()[2:] == [255, 254] and want.info[6].tolist()[2:] == [9, 8]
    assert want.info[8].tolist()[2:] == [80, 119] and want.info[7].tolist() == [UN, 0, 10, 8]
    assert want.bits[0].tolist() == want.bits[3].tolist()           # a chain's environments do not depend on its length
    assert bool((want.info[:9, 1] > 0).sum() == 8) and not bool(want.bits[9:].any()) and not bool(want.info[9:, 1].any())
    n = len(rows)
    table, labels = fs.keys.device_tables("cuda")
    bits = torch.full((n + 2, 16), SENT, dtype=torch.int64, device="cuda")
    info = torch.full((n + 2, 4), SENT, dtype=torch.int32, device="cuda")
    out = (bits[1:n + 1], info[1:n + 1])
    got = ops.smiles_fp(ys.cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, -1,
                        out=out)
    assert got[0] is out[0]
    same(got, want)
    for t in (bits, info):
        assert bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all())
    with pytest.raises(ValueError):
        fs.fp_rows(ys.cuda(), starts)                                # starts on the host are checked there
    with pytest.raises(ValueError):
        ops.smiles_fp(ys.cuda(), torch.zeros(3, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, -1)
    with pytest.raises(ValueError):
        ops.smiles_fp(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, len(VOCAB))
    with pytest.raises(ValueError):
        ops.smiles_fp(ys.cuda(), torch.zeros(n, dtype=torch.int32, device="cuda"), table, labels, PAD, EOS, -1,
                      out=(bits[:n, :8], info[:n]))
    empty = fs.fp_rows(torch.zeros(0, W, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int64))
    assert empty.bits.shape == (0, 16) and empty.info.shape == (0, 4)


def test_sep_eos_slots_and_ids_outside_the_vocabulary(ops):
    """W = 256, start 0: the <sep> in a lane's fourth slot, <sep> <eos> in the last two positions, a <sep> with no
    <eos>, two <sep>, a <sep> behind the <eos>; and ids outside [0, V), which make a part SYNTAX."""
    fs, W, C, V = FPS[True], 256, VOCAB.index("C"), len(VOCAB)
    ys = torch.full((9, W), C)
    ys[0, 200], ys[0, 253:] = SEP, torch.tensor([EOS, PAD, PAD])
    ys[1, 254], ys[1, 255] = SEP, EOS
    ys[2, 255] = SEP
    ys[3, 70], ys[3, 130], ys[3, 190:] = SEP, SEP, torch.tensor([EOS] + [PAD] * 65)
    ys[4, 100], ys[4, 200] = EOS, SEP
    ys[5:, 3] = EOS
    ys[5, 1], ys[6, 1], ys[7, 1], ys[8, 1] = -1, V, 2 ** 40, -2 ** 62
    want = fs.fp_reference(ys, [0] * 9)
    G, SY = _ops.FP_GRAPH, _ops.FP_SYNTAX
    assert want.info[:, 0].tolist() == [G, SY, -1, SY, G, SY, SY, SY, SY] and want.info[0].tolist()[2:] == [52, 51]
    same(fs.fp_rows(ys.cuda(), [0] * 9), want)
    same(fs.fp_rows(ys.int()[:5].cuda(), [0] * 5), fs.fp_reference(ys[:5], [0] * 5))     # any integer dtype


def test_device_spellings_keep_the_fingerprint(ops):
    """8 randomize_rows spellings of each of the 63 corpus molecules: one fingerprint per molecule, the host
    statement's."""
    rz, fs, k = RZ[False], FPS[False], 8
    toks = [ids_of(s) for s in CORPUS]
    W = max(len(t) for t in toks) + 1
    ys = torch.tensor([t + [EOS] + [PAD] * (W - len(t) - 1) for t in toks]).repeat_interleave(k, 0).cuda()
    n = ys.shape[0]
    spelt = rz.randomize_rows(ys, [0] * n, torch.arange(n), 11, 1.0, out_width=W + 24)
    assert int((spelt.info[:, 0] == _ops.RAND_OK).sum()) == n
    assert int((spelt.tokens[:, :W] != ys).any(1).sum()) >= n // 2
    got = fs.fp_rows(spelt.tokens, [0] * n)
    bits = got.bits.view(len(CORPUS), k, 16).cpu()
    assert bool((got.info[:, 0] == _ops.FP_GRAPH).all()) and bool((bits == bits[:, :1]).all())
    assert bits[:, 0].tolist() == [fs.fingerprint(t)[1] for t in toks]
    assert got.info[:, 1].view(len(CORPUS), k)[:, 0].tolist() == [ref.popcount(ref.fingerprint(PATTERN.findall(s))[1])
                                                                  for s in CORPUS]


# --------------------------------------------------------------------------------- 2. gct_fp_tanimoto
def random_fps(n, seed, special=True):
    """n rows of random words, row r at bit density 1/64, 1/8 or 1/2 by r % 3 (the AND of 6, 3 or 1 random words); with
    `special` and four rows or more, row 1 has all 1024 bits, row 2 is absent and row 3 repeats row 0."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(-2 ** 63, 2 ** 63 - 1, (n, 6, 16), generator=g)
    bits = torch.empty(n, 16, dtype=torch.int64)
    for r in range(n):
        x = raw[r, 0]
        for k in range(1, (6, 3, 1)[r % 3]):
            x = x & raw[r, k]
        bits[r] = x
    if special and n >= 4:
        bits[1], bits[2], bits[3] = -1, 0, bits[0]
    return with_counts(bits)


def with_counts(bits):
    info = torch.zeros(bits.shape[0], 4, dtype=torch.int32)
    info[:, 1] = torch.tensor([sum(bin(v & (2 ** 64 - 1)).count("1") for v in row) for row in bits.tolist()], dtype=torch.int32)
    return FpRows(bits, info)


def cuda(fps):
    return FpRows(fps.bits.cuda(), fps.info.cuda())


def agree(got, want, m):
    assert got.best.dtype == torch.float32 and got.arg.dtype == torch.int32 and got.total.dtype == torch.float64
    assert got.best.cpu().tolist() == want.best.tolist() and got.arg.cpu().tolist() == want.arg.tolist()
    err = (got.total.cpu() - want.total).abs()
    assert bool((err <= m * 2.0 ** -53 * want.total).all()), (err.max().item(), m)
    assert int(got.present) == int(want.present)


def test_plan_is_a_function_of_the_shapes(ops):
    tile_b, one = ops.fp_tanimoto_plan(1, 1)
    assert tile_b == 128 and one == 1
    assert [ops.fp_tanimoto_plan(1, m)[1] for m in (tile_b - 1, tile_b, tile_b + 1, 2 * tile_b, 2 * tile_b + 1)] == [1, 1, 2, 2, 3]
    assert ops.fp_tanimoto_plan(4096, 1 << 20)[1] == 64 and ops.fp_tanimoto_plan(32768, 32768)[1] == 8
    assert ops.fp_tanimoto_plan(1, 1 << 30)[1] == 256 and ops.fp_tanimoto_plan(1 << 20, 1 << 20)[1] == 1
    assert ops.fp_tanimoto_plan(0, 0)[1] == 1
    with pytest.raises(ValueError):
        ops.fp_tanimoto_plan(-1, 4)


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tanimoto_equals_the_reference(ops, n, p):
    """m = 1, and one below, at and one above tile_b (128); tile_b + 1 is also the first m that fp_tanimoto_plan splits
    (two splits for n = 1 .. 257: the fold runs), and one above it; a holds a row of all 1024 bits, an absent row and a
    duplicate, b likewise (the lowest j wins)."""
    tile_b = ops.fp_tanimoto_plan(n, 1)[0]
    assert [ops.fp_tanimoto_plan(n, m)[1] for m in (tile_b, tile_b + 1)] == [1, 2]
    a = random_fps(n, 100 + n)
    for m in (1, tile_b - 1, tile_b, tile_b + 1, tile_b + 2):
        b = random_fps(m, 200 + m)
        am = a
        if n >= 4 and m >= 4:                                      # a[0] is b[0], which b[3] repeats: the lower one wins
            bits = a.bits.clone()
            bits[0] = b.bits[0]
            am = with_counts(bits)
        want = tanimoto_reference(am, b, p)
        agree(tanimoto_agg(cuda(am), cuda(b), p), want, m)
        if n >= 4 and m >= 4:
            assert want.best[1].item() == 1.0 and want.arg[1].item() == 1 and want.arg[2].item() == -1
            assert want.best[0].item() == 1.0 and want.arg[0].item() == 0 and 3 not in want.arg.tolist()


def test_tanimoto_edges_strides_guards_and_repeats(ops):
    tile_b = ops.fp_tanimoto_plan(1, 1)[0]
    # a equal to b, with duplicates: the diagonal is 1 and arg is the lowest copy
    a = random_fps(tile_b + 2, 7)
    a.bits[tile_b + 1] = a.bits[5]
    a = with_counts(a.bits)
    want = tanimoto_reference(a, a)
    present = a.info[:, 1] > 0
    assert bool((want.best[present] == 1.0).all()) and want.arg[3].item() == 0 and want.arg[tile_b + 1].item() == 5
    assert [i for i in range(tile_b + 2) if want.arg[i].item() != i] == [2, 3, tile_b + 1]
    agree(tanimoto_agg(cuda(a), cuda(a)), want, tile_b + 2)
    # b entirely absent, and b without rows
    b0 = with_counts(torch.zeros(tile_b + 1, 16, dtype=torch.int64))
    for b in (b0, FpRows(b0.bits[:0], b0.info[:0])):
        got = tanimoto_agg(cuda(a), cuda(b), 2)
        assert got.best.tolist() == [0.0] * (tile_b + 2) and got.arg.tolist() == [-1] * (tile_b + 2)
        assert got.total.tolist() == [0.0] * (tile_b + 2) and int(got.present) == 0
    # a zero similarity still names its row
    lone = with_counts(torch.tensor([[255] + [0] * 15]))
    other = with_counts(torch.tensor([[0] * 16, [0, 255] + [0] * 14]))
    got = tanimoto_agg(cuda(lone), cuda(other))
    assert (got.best.tolist(), got.arg.tolist(), got.total.tolist()) == ([0.0], [1], [0.0])
    # rows of a with stride 21, rows of b with stride 16 inside a wider buffer; outputs inside guarded buffers
    n, m = 65, tile_b + 1
    a, b = random_fps(n, 11), random_fps(m, 12)
    wide = torch.full((n, 21), SENT, dtype=torch.int64, device="cuda")
    wide[:, :16] = a.bits.cuda()
    av = wide[:, :16]
    assert av.stride() == (21, 1)
    best = torch.full((n + 2,), float(SENT), dtype=torch.float32, device="cuda")
    arg = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    total = torch.full((n + 2,), float(SENT), dtype=torch.float64, device="cuda")
    out = (best[1:n + 1], arg[1:n + 1], total[1:n + 1])
    ca, cb = a.info[:, 1].contiguous().cuda(), b.info[:, 1].contiguous().cuda()
    for p in (1, 2):
        got = ops.fp_tanimoto(av, ca, b.bits.cuda(), cb, p, out=out)
        assert got[0] is out[0]
        want = tanimoto_reference(a, b, p)
        agree(type(want)(*got, want.present), want, m)
        for t in (best, arg, total):
            assert t[0].item() == SENT and t[-1].item() == SENT
        again = ops.fp_tanimoto(av, ca, b.bits.cuda(), cb, p)
        assert torch.equal(again[2], got[2]) and torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    # the wrapper's refusals
    for bad in (lambda: ops.fp_tanimoto(av, ca, b.bits.cuda(), cb, 3),
                lambda: ops.fp_tanimoto(av, ca[:5], b.bits.cuda(), cb),
                lambda: ops.fp_tanimoto(av[:, :8], ca, b.bits.cuda(), cb),
                lambda: ops.fp_tanimoto(av, ca, b.bits.cuda().t().contiguous().t(), cb),
                lambda: ops.fp_tanimoto(av, ca, b.bits.cuda(), cb, out=out[:2])):
        with pytest.raises(ValueError):
            bad()
    none = ops.fp_tanimoto(av[:0], ca[:0], b.bits.cuda(), cb)
    assert [t.shape for t in none] == [(0,)] * 3


def test_metrics_on_the_device_equal_the_host(ops):
    fs = FPS[False]
    smiles = CORPUS[:30] + ["C/C=C/C", "C("]
    ids = [ids_of(s) for s in smiles]
    W = max(len(t) for t in ids) + 1
    ys = torch.tensor([t + [EOS] + [PAD] * (W - len(t) - 1) for t in ids])
    host, dev = fs.fp_reference(ys, [0] * len(ids)), fs.fp_rows(ys.cuda(), [0] * len(ids))
    xs = [ref.fingerprint(PATTERN.findall(s))[1] for s in smiles]
    valid = torch.tensor([i % 4 != 1 for i in range(len(ids))])
    for p in (1, 2):
        assert internal_diversity(dev, p=p) == pytest.approx(ref.int_div(xs, p), abs=1e-12)
        assert internal_diversity(dev, valid.cuda(), p) == pytest.approx(internal_diversity(host, valid, p), abs=1e-12)
    train = FpRows(dev.bits[10:], dev.info[10:])
    assert snn(dev, train) == pytest.approx(ref.snn(xs, xs[10:]), abs=1e-12)
    index = FingerprintIndex(host.bits[10:30], host.info[10:30, 1].contiguous())
    want = tanimoto_reference(host, FpRows(host.bits[10:30], host.info[10:30]))
    for chunk in (3, 7, 1 << 20):
        best, arg = index.nearest(dev, chunk=chunk)
        assert best.is_cuda and best.cpu().tolist() == want.best.tolist() and arg.cpu().tolist() == want.arg.tolist()


# --------------------------------------------------------------------------------- 3. the front ends
def test_sampler_fingerprints_metrics_snn_and_index():
    from gct_plus_amd.molkey import MolKeyIndex
    from tests.test_chem_gpu import VOCAB31, tiny_inputs, tiny_sampler
    sp = tiny_sampler(well_formed=True)
    fs = sp.fingerprinter
    assert sp.fingerprinter is fs and fs.keys is sp.keys
    smiles = ["CCO", "OCC", "C(C)O", "c1ccccc1", "C1CC1N", "C[C@@H](N)O", "CC(", "N#N", "c1ccccc1"]
    got = sp.fingerprints(smiles)
    assert got.bits.is_cuda and tuple(got.bits.shape) == (9, 16)
    for i, s in enumerate(smiles):
        st, words = fs.fingerprint(ids_of(s, VOCAB31))
        assert (int(got.info[i, 0]), got.bits[i].tolist()) == (st, words), s
    assert got.bits[0].tolist() == got.bits[1].tolist() == got.bits[2].tolist() and int(got.info[5, 1]) == 0
    ids = [ids_of(s, VOCAB31) + [sp.eos_id] for s in smiles]
    W = max(len(r) for r in ids) + 3
    rows = torch.tensor([[sp.sos_id] * 2 + r + [sp.pad_id] * (W - 2 - len(r)) for r in ids]).cuda()
    same(sp.fingerprints((rows, torch.full((9,), 2))), FpRows(got.bits.cpu(), got.info.cpu()))
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
    want_fps = fs.fp_reference(rows.ys.cpu(), rows.prefix_lens)
    same(sp.fingerprints(rows), want_fps)
    train = ["OCC", "NCC", "C1CC1", "C/C=C/C", "CC(", "CC(=O)O"]
    index = FingerprintIndex.from_smiles(sp, train, chunk=2)
    W = max(len(ids_of(s, VOCAB31)) for s in train) + 1
    host_rows = torch.tensor([ids_of(s, VOCAB31) + [sp.eos_id] + [sp.pad_id] * (W - 1 - len(ids_of(s, VOCAB31))) for s in train])
    want_index = FingerprintIndex.from_rows(fs, [(host_rows, [0] * len(train))])
    assert index.bits.is_cuda and len(index) == 4
    assert torch.equal(index.bits.cpu(), want_index.bits) and torch.equal(index.counts.cpu(), want_index.counts)
    on_dev = FingerprintIndex.from_rows(fs, [(host_rows.cuda(), [0] * len(train))])
    assert torch.equal(on_dev.bits.cpu(), want_index.bits)
    # basic_metrics: intDiv over the valid rows against the oracle, the other keys as without int_div
    key_index = MolKeyIndex.from_smiles(sp, train, chunk=2)
    plain = sp.basic_metrics(rows, key_index)
    full = sp.basic_metrics(rows, key_index, int_div=True)
    assert list(full) == list(plain) + ["intDiv", "n_fp"] and {k: full[k] for k in plain} == plain
    ok = (sp.chemistry.check_reference(rows.ys.cpu(), rows.prefix_lens).status == _ops.CHEM_OK).tolist()
    strings = [[VOCAB31[t] for t in row[t0:row.index(sp.eos_id, t0)]] if sp.eos_id in row[t0:] else None
               for row, t0 in zip(rows.ys.cpu().tolist(), [int(t) for t in rows.prefix_lens])]
    xs = [ref.fingerprint(s)[1] if s is not None else 0 for s in strings]
    assert [ref.words(x) for x in xs] == want_fps.bits.tolist()
    kept = [x for x, v in zip(xs, ok) if v and x]
    assert full["n_fp"] == len(kept) >= 8 and full["intDiv"] == pytest.approx(ref.int_div(kept), abs=1e-12)
    assert 0.0 < full["intDiv"] < 1.0
    ys_ = [big for big in (ref.fingerprint(PATTERN.findall(s))[1] for s in train) if big]
    assert sp.snn(rows, index) == pytest.approx(ref.snn(xs, ys_), abs=1e-12)
    assert sp.snn(rows, want_index) == sp.snn(sp.fingerprints(rows), index) == sp.snn(rows, sp.fingerprints(train))
