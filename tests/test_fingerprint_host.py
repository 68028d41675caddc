"""Circular fingerprints and Tanimoto metrics on the host (no GPU): SmilesFingerprints.fingerprint -- THE statement --
against the independent oracle of tests/fingerprint_ref.py bit for bit; fingerprints under SmilesRandomizer's spellings;
the pinned limit of radius 2; fp_reference's spans; tanimoto_reference, internal_diversity and snn against the oracle;
FingerprintIndex; similarity_reward; and basic_metrics with and without fingerprints."""
import itertools
import os
import re

import pytest
import torch

from gct_plus_amd import ops
from gct_plus_amd.fingerprint import (FingerprintIndex, FpRows, SmilesFingerprints, TanimotoAgg, internal_diversity, snn,
                                      tanimoto_reference)
from gct_plus_amd.molkey import MolKeyIndex, basic_metrics
from gct_plus_amd.randomize import stream
from gct_plus_amd.Train.finetune import similarity_reward
from tests import fingerprint_ref as ref
from tests import molkey_ref
from tests.test_molkey_host import CORPUS, KEYS, RZ, WL_HARD, report_of, row_of, strings
from tests.test_randomize_gpu import KEPT_ROWS
from tests.test_randomize_host import EOS, PAD, SEP, VOCAB, ids_of

FPS = SmilesFingerprints(VOCAB, PAD, EOS, SEP)
NO_GRAPH = [s for s in KEPT_ROWS if s != "S(C)(C)(C)(C)(C)(C)(C)C"] + ["C\\C=C\\C", "C()C", "CC.O"]
# non-isomorphic pairs of the corpus that radius 2 cannot separate: the two WL_HARD pairs, and two more
MERGED = WL_HARD + [("C12C3C4C1C5C2C3C45", "C12C3C1C23"), ("C1CC2CCC1C2", "C1CC1CC1CC1")]


def big(words):
    x = 0
    for w, v in enumerate(words):
        x |= (int(v) & (2 ** 64 - 1)) << (64 * w)
    return x


def fp_of(s):
    return FPS.fingerprint(ids_of(s))


def rows_of(smiles):
    """An FpRows of SMILES strings through fp_reference."""
    ids = [ids_of(s) for s in smiles]
    W = max(len(t) for t in ids) + 1
    return FPS.fp_reference(torch.tensor([row_of(t, W) for t in ids]), [0] * len(ids))


def synthetic(words_and_counts):
    """An FpRows of hand-made rows: (16 words or a dict word -> value, count)."""
    bits = torch.zeros(len(words_and_counts), ops.FP_WORDS, dtype=torch.int64)
    info = torch.zeros(len(words_and_counts), 4, dtype=torch.int32)
    for r, (words, count) in enumerate(words_and_counts):
        for w, v in words.items():
            bits[r, w] = v
        info[r, 1] = count
    return FpRows(bits, info)


# ------------------------------------------------------------------------------------------ 1. the rule
def test_constants_are_shared():
    """Radius, width and status codes are one set of constants: the header's, ops' and the oracle's."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gctplus_hip.h")).read()
    assert int(re.search(r"#define GCT_FP_RADIUS (\d+)", header).group(1)) == ops.FP_RADIUS == ref.RADIUS == 2
    assert int(re.search(r"#define GCT_FP_BITS (\d+)", header).group(1)) == ops.FP_BITS == ref.BITS == 1024
    assert ops.FP_WORDS * 64 == ops.FP_BITS and ops.FP_MAX_SPAN == ops.KEY_MAX_SPAN
    for name in ("GRAPH", "SYNTAX", "UNSUPPORTED"):
        assert int(re.search(rf"#define GCT_FP_{name} (\d+)", header).group(1)) == getattr(ops, f"FP_{name}") == getattr(ref, name)
    assert FPS.labels is KEYS.labels or FPS.labels == KEYS.labels
    assert FPS.words == KEYS.words and FPS.keys.randomizer is FPS.randomizer


def test_fingerprint_equals_the_oracle_bit_for_bit():
    counts = []
    for s in CORPUS + KEPT_ROWS + NO_GRAPH:
        status, words = fp_of(s)
        want = ref.fingerprint(strings(s))
        assert (status, words) == (want[0], ref.words(want[1])), s
        assert len(words) == 16 and all(-2 ** 63 <= w < 2 ** 63 for w in words)
        if s in CORPUS:
            assert status == ops.FP_GRAPH
            counts.append(ref.popcount(want[1]))
    assert min(counts) == 3 and max(counts) == 54                    # (3: CC, one environment per round)


def test_rows_without_a_graph_have_no_bit():
    seen = set()
    for s in NO_GRAPH:
        status, words = fp_of(s)
        want = ops.FP_SYNTAX if RZ.parse(ids_of(s)) is None else ops.FP_UNSUPPORTED
        assert status == want and words == [0] * 16, s
        seen.add(status)
    assert seen == {ops.FP_SYNTAX, ops.FP_UNSUPPORTED}
    V = len(VOCAB)
    for t in (-1, V, 2 ** 40):
        assert FPS.fingerprint([ids_of("C")[0], t]) == (ops.FP_SYNTAX, [0] * 16)


def test_randomised_spellings_keep_the_fingerprint():
    checked = changed = 0
    for m, s in enumerate(CORPUS):
        toks = ids_of(s)
        want = FPS.fingerprint(toks)
        for k in range(50):
            status, out, _ = RZ.randomize(toks, stream(5, k | m << 32, 0))
            assert status == ops.RAND_OK, s
            assert FPS.fingerprint(out) == want, (s, "".join(VOCAB[t] for t in out))
            checked += 1
            changed += out != toks
    assert checked >= 3000 and changed >= checked // 2


def test_identities_and_the_pinned_limit_of_radius_two():
    """CC is C-C; T(x, x) = 1; T is symmetric; labels are strings, not ids.  The limit: a fingerprint is not identity
    -- the two WL_HARD pairs (and two more pairs of the corpus) share a fingerprint although their keys differ, and
    those four are ALL the non-isomorphic pairs of the corpus that merge."""
    assert fp_of("CC") == fp_of("C-C") and fp_of("c1ccccc1") == fp_of("c:1:c:c:c:c:c1")
    assert fp_of("C1CCCCC1") != fp_of("c1ccccc1") and fp_of("CC=O") != fp_of("C=CO")
    bits = {s: ref.fingerprint(strings(s))[1] for s in CORPUS}
    for a, b in itertools.combinations(CORPUS[::3], 2):
        assert ref.tanimoto(bits[a], bits[b]) == ref.tanimoto(bits[b], bits[a])
    assert all(ref.tanimoto(x, x) == 1.0 for x in bits.values())
    for a, b in WL_HARD:
        assert fp_of(a) == fp_of(b) and KEYS.key(ids_of(a)) != KEYS.key(ids_of(b)), (a, b)
    graphs = {s: molkey_ref.graph(strings(s)) for s in CORPUS}
    merged = {(a, b) for a, b in itertools.combinations(CORPUS, 2)
              if bits[a] == bits[b] and not molkey_ref.isomorphic(graphs[a], graphs[b])}
    assert merged == {tuple(sorted(p, key=CORPUS.index)) for p in MERGED}
    for a, b in itertools.combinations(CORPUS, 2):                   # the other direction has no exception
        if molkey_ref.isomorphic(graphs[a], graphs[b]):
            assert bits[a] == bits[b], (a, b)
    other = VOCAB[:5] + VOCAB[5:][::-1]
    f2 = SmilesFingerprints(other, PAD, EOS, SEP)
    for s in CORPUS[::4]:
        assert f2.fingerprint(ids_of(s, other)) == fp_of(s), s


# ------------------------------------------------------------------------------------------ 2. the batch rule
def test_fp_reference_spans_sep_and_rows_without_eos():
    mol, sca, bad = ids_of("CC(=O)Oc1ccccc1"), ids_of("c1ccccc1"), ids_of("C/C=C/C")
    W = 48
    rows = [row_of(sca + [SEP] + mol, W, 1, 2), row_of(mol, W, 3, ids_of("N")[0]), row_of(bad + [SEP] + mol, W),
            row_of(mol + [SEP] + ids_of("C(C"), W), row_of(mol + [SEP] + bad, W), row_of(sca + [SEP] + mol + [SEP] + mol, W),
            [ids_of("C")[0]] * W, [PAD] * W, row_of([], W), row_of(mol, W), row_of([ids_of("C")[0], len(VOCAB) + 2], W)]
    starts = [1, 3, 0, 0, 0, 0, 0, 0, 0, W, 0]
    got = FPS.fp_reference(torch.tensor(rows), starts)
    assert got.bits.dtype == torch.int64 and tuple(got.bits.shape) == (11, 16)
    assert got.info.dtype == torch.int32 and tuple(got.info.shape) == (11, 4)
    st, wm = FPS.fingerprint(mol)
    pop = ref.popcount(big(wm))
    G, SY, UN = ops.FP_GRAPH, ops.FP_SYNTAX, ops.FP_UNSUPPORTED
    for r in (0, 1, 2):                                              # the molecule behind <sep>; the scaffold is not read
        assert got.bits[r].tolist() == wm and got.info[r].tolist() == [G, pop, 10, 10], r
    assert got.info[3].tolist() == [SY, 0, 0, 0] and got.info[4].tolist() == [UN, 0, 4, 3]
    assert got.info[5].tolist() == [SY, 0, 0, 0]                     # a second <sep> is no SMILES token
    for r in (6, 7, 9):                                              # no <eos> in the span (row 9: an empty span)
        assert got.info[r].tolist() == [-1, 0, 0, 0]
    assert got.info[8].tolist() == [SY, 0, 0, 0] and got.info[10].tolist() == [SY, 0, 0, 0]
    assert not bool(got.bits[3:].any())
    assert FPS.fp_reference(torch.tensor(rows[:2]), [-1, W + 1]).info.tolist() == [[-1, 0, 0, 0]] * 2
    assert FPS.fp_reference(torch.tensor([[PAD] * 300]), [0]).info.tolist() == [[-1, 0, 0, 0]]
    nosep = SmilesFingerprints(VOCAB, PAD, EOS).fp_reference(torch.tensor(rows[:1]), [1])
    assert nosep.info[0].tolist() == [SY, 0, 0, 0]
    keys = KEYS.key_reference(torch.tensor(rows), starts)            # the same spans as the keys: status, atoms, bonds
    assert got.info[:, [0, 2, 3]].tolist() == keys.info[:, [0, 2, 3]].tolist()
    with pytest.raises(ValueError):
        FPS.fp_reference(torch.tensor(rows), starts[:3])


# ------------------------------------------------------------------------------------------ 3. Tanimoto and its figures
def test_tanimoto_reference_against_the_oracle():
    smiles = CORPUS[:20] + ["C/C=C/C", "CC", "C-C", "C("]
    fps = rows_of(smiles)
    xs = [big(r) for r in fps.bits.tolist()]
    assert xs == [ref.fingerprint(strings(s))[1] for s in smiles]
    for p in (1, 2):
        got = tanimoto_reference(fps, FpRows(fps.bits[5:], fps.info[5:]), p)
        want = ref.aggregate(xs, xs[5:], p)
        assert isinstance(got, TanimotoAgg) and got.best.dtype == torch.float32 and got.arg.dtype == torch.int32
        assert got.total.dtype == torch.float64 and int(got.present) == len(smiles) - 5 - 2
        assert got.best.tolist() == [w[0] for w in want] and got.arg.tolist() == [w[1] for w in want]
        assert got.total.tolist() == pytest.approx([w[2] for w in want], rel=1e-13, abs=0)
    assert got.arg[20].item() == -1 and got.arg[23].item() == -1     # absent rows of a
    assert got.arg[22].item() == 21 - 5                              # C-C: the lowest copy in b is CC's
    none = tanimoto_reference(fps, FpRows(fps.bits[20:21], fps.info[20:21]))
    assert none.best.tolist() == [0.0] * 24 and none.arg.tolist() == [-1] * 24 and none.total.tolist() == [0.0] * 24
    empty = tanimoto_reference(fps, FpRows(fps.bits[:0], fps.info[:0]))
    assert empty.arg.tolist() == [-1] * 24 and int(empty.present) == 0
    with pytest.raises(ValueError):
        tanimoto_reference(fps, fps, p=3)
    with pytest.raises(ValueError):
        tanimoto_reference(fps, fps.bits)


def test_a_zero_similarity_still_names_its_row():
    """The maximum is attained, also when it is 0: arg is the lowest present row, not -1."""
    a = synthetic([({0: 0xFF}, 8)])
    b = synthetic([({}, 0), ({1: 0xFF}, 8), ({2: 0xF}, 4)])
    got = tanimoto_reference(a, b)
    assert (got.best.tolist(), got.arg.tolist(), got.total.tolist()) == ([0.0], [1], [0.0])


def test_internal_diversity():
    one = rows_of(["CC(=O)Oc1ccccc1"] * 5)
    assert internal_diversity(one) == 0.0 and internal_diversity(one, p=2) == 0.0
    halves = synthetic([({0: 0xFF}, 8), ({1: 0xFF}, 8)] * 3)        # disjoint bits, equal shares: self pairs count
    assert internal_diversity(halves) == 0.5
    smiles = CORPUS[:24] + ["C/C=C/C", "C("]
    fps = rows_of(smiles)
    xs = [ref.fingerprint(strings(s))[1] for s in smiles]
    assert internal_diversity(fps) == pytest.approx(ref.int_div(xs), abs=1e-12)
    assert internal_diversity(fps, p=2) == pytest.approx(ref.int_div(xs, 2), abs=1e-12)
    valid = torch.tensor([i % 3 != 0 for i in range(len(smiles))])
    kept = [x for x, v in zip(xs, valid.tolist()) if v]
    assert internal_diversity(fps, valid) == pytest.approx(ref.int_div(kept), abs=1e-12)
    assert internal_diversity(fps, valid) != pytest.approx(ref.int_div(xs), abs=1e-6)
    assert internal_diversity(fps, torch.zeros(len(smiles), dtype=torch.bool)) == 0.0
    assert internal_diversity(rows_of(["C(", "C/C=C/C"])) == 0.0
    assert internal_diversity(FpRows(fps.bits[:0], fps.info[:0])) == 0.0
    assert 0.85 < internal_diversity(rows_of(CORPUS)) < 0.95
    with pytest.raises(ValueError):
        internal_diversity(fps, valid[:3])


def test_snn_against_the_oracle():
    gen, train = CORPUS[:12] + ["C(", "CCO"], CORPUS[8:30] + ["C/C=C/C"]
    g, t = rows_of(gen), rows_of(train)
    xs, ys = [ref.fingerprint(strings(s))[1] for s in gen], [ref.fingerprint(strings(s))[1] for s in train]
    assert snn(g, t) == pytest.approx(ref.snn(xs, ys), abs=1e-12)
    assert 0.0 < ref.snn(xs, ys) < 1.0
    index = FingerprintIndex.from_rows(FPS, [(torch.tensor([row_of(ids_of(s), 64) for s in train]), [0] * len(train))])
    assert len(index) == len(train) - 1 and snn(g, index) == pytest.approx(ref.snn(xs, ys), abs=1e-12)
    assert snn(g, FpRows(t.bits[:0], t.info[:0])) == 0.0 and snn(FpRows(g.bits[12:13], g.info[12:13]), t) == 0.0
    assert snn(g, g) == 1.0


def test_index_round_trip_mismatch_and_nearest_across_chunks(tmp_path):
    train = ["CCO", "c1ccccc1", "C/C=C/C", "CC(=O)O", "OCC", "C(C", "c1ccccc1", "CCN"]
    W = 12
    ys = torch.tensor([row_of(ids_of(s), W) for s in train])
    index = FingerprintIndex.from_rows(FPS, [(ys[:3], [0] * 3), (ys[3:], [0] * 5)])
    kept = [s for s in train if s not in ("C/C=C/C", "C(C")]          # CCO benzene CC(=O)O OCC benzene CCN
    assert len(index) == 6 and index.shape == (ops.FP_BITS, ops.FP_RADIUS)
    assert index.bits.tolist() == [fp_of(s)[1] for s in kept]
    assert index.counts.dtype == torch.int32 and index.counts.tolist() == [ref.popcount(big(fp_of(s)[1])) for s in kept]
    assert len(FingerprintIndex.from_rows(FPS, [])) == 0
    probe = rows_of(["OCC", "c1ccccc1", "C(", "CCCN", "C1CC1"])
    xs, ys_ = [big(r) for r in probe.bits.tolist()], [big(r) for r in index.bits.tolist()]
    want = ref.aggregate(xs, ys_)
    for chunk in (1, 2, 3, 4, 6, 1 << 20):                           # CCO at 0 and 3, benzene at 1 and 4: ties across chunks
        best, arg = index.nearest(probe, chunk=chunk)
        assert best.dtype == torch.float32 and arg.dtype == torch.int32
        assert best.tolist() == [w[0] for w in want] and arg.tolist() == [w[1] for w in want], chunk
    assert arg.tolist()[:3] == [0, 1, -1] and best.tolist()[:3] == [1.0, 1.0, 0.0]
    none = FingerprintIndex.from_rows(FPS, []).nearest(probe)
    assert none[0].tolist() == [0.0] * 5 and none[1].tolist() == [-1] * 5
    path = str(tmp_path / "train.fps")
    index.save(path)
    again = FingerprintIndex.load(path)
    assert torch.equal(again.bits, index.bits) and torch.equal(again.counts, index.counts) and again.shape == index.shape
    assert torch.load(path, weights_only=True).keys() == {"bits", "counts", "fp_bits", "fp_radius"}
    for key, value in (("fp_bits", 2048), ("fp_radius", 3)):
        blob = torch.load(path, weights_only=True)
        blob[key] = value
        other = str(tmp_path / f"other_{key}.fps")
        torch.save(blob, other)
        with pytest.raises(ValueError, match="build the index again"):
            FingerprintIndex.load(other)
    with pytest.raises(ValueError):
        FingerprintIndex(index.bits[:, :8], index.counts)
    with pytest.raises(ValueError):
        index.nearest(probe, chunk=0)


def test_similarity_reward():
    best = torch.tensor([0.0, 0.2, 0.4, 0.5, 0.8, 1.0])
    assert similarity_reward(best).tolist() == best.tolist() and similarity_reward(best).dtype == torch.float32
    got = similarity_reward(best, lo=0.4, hi=0.8)
    assert got.tolist() == pytest.approx([0.0, 0.0, 0.0, 0.25, 1.0, 1.0], abs=1e-6)
    agg = TanimotoAgg(best, torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.float64), torch.tensor(1))
    assert torch.equal(similarity_reward(agg, 0.4, 0.8), got)
    assert not similarity_reward(best.double().requires_grad_()).requires_grad
    for lo, hi in ((0.5, 0.5), (-0.1, 1.0), (0.0, 1.5), (0.8, 0.4)):
        with pytest.raises(ValueError):
            similarity_reward(best, lo, hi)
    with pytest.raises(ValueError):
        similarity_reward(torch.zeros(3, dtype=torch.int32))


def test_basic_metrics_dict_is_unchanged_without_fingerprints():
    rows = ["CCO", "OCC", "CCN", "c1ccccc1", "C(C)O", "CC", "C-C", "C/C=C/C"]
    keys = torch.tensor([KEYS.key(ids_of(s))[1] for s in rows])
    OK, BAD = ops.CHEM_OK, ops.CHEM_VALENCE
    report = report_of([BAD, OK, OK, OK, OK, BAD, OK, OK])
    index = MolKeyIndex(torch.tensor([keys[0].item(), keys[5].item()]))
    plain = basic_metrics(report, keys, index)
    assert list(plain) == ["valid", "unique", "novel", "n", "n_valid", "n_unique", "n_novel"]
    assert list(basic_metrics(report, keys)) == ["valid", "unique", "n", "n_valid", "n_unique"]
    fps = rows_of(rows)
    full = basic_metrics(report, keys, index, fps)
    assert list(full) == list(plain) + ["intDiv", "n_fp"] and {k: full[k] for k in plain} == plain
    valid = [s for s, st in zip(rows, report.status.tolist()) if st == OK]
    xs = [ref.fingerprint(strings(s))[1] for s in valid]
    assert full["n_fp"] == 5 and full["intDiv"] == pytest.approx(ref.int_div(xs), abs=1e-12)
    none = basic_metrics(report_of([BAD] * 8), keys, None, fps)
    assert none["intDiv"] == 0.0 and none["n_fp"] == 0
    with pytest.raises(ValueError):
        basic_metrics(report, keys, None, FpRows(fps.bits[:3], fps.info[:3]))
