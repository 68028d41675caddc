"""Molecule identity keys on the host (no GPU): SmilesKeys.key -- THE statement -- against the independent oracle of
tests/molkey_ref.py bit for bit; key equality against the oracle's backtracking isomorphism test over every pair of a
corpus of 63 graphs; keys under SmilesRandomizer's spellings; string keys of rows without a graph; scaffold rows; rows
without <eos>; and what the keys are for: first_occurrence, MolKeyIndex, basic_metrics, uniqueness_reward."""
import itertools
import os
import re

import pytest
import torch

from gct_plus_amd import ops
from gct_plus_amd.smiles import ChemReport
from gct_plus_amd.molkey import (MolKeyIndex, MolKeys, SmilesKeys, as_int64, basic_metrics, first_occurrence, mix,
                                 mix_tensor)
from gct_plus_amd.randomize import SmilesRandomizer, stream
from gct_plus_amd.Train.finetune import uniqueness_reward
from tests import molkey_ref as ref
from tests.test_randomize_gpu import KEPT_ROWS
from tests.test_randomize_host import EOS, MOLECULES, PAD, PATTERN, SEP, VOCAB, ids_of

WL_HARD = [("C1CCC2CCCCC2C1", "C1CCCC1C1CCCC1"), ("C1CCCCC1C1CCCCC1", "C1CCC2CCCCCC2CC1")]
EXTRA = [s for pair in WL_HARD for s in pair] + [
    "Cc1ccccc1C", "Cc1cccc(C)c1", "Cc1ccc(C)cc1", "CC=O", "C=CO", "C1CCCCC1", "c1ccccc1", "C=1CCCCC1", "CC", "C-C",
    "C1CC1C1CC1", "C1CCC1C1CCC1", "C1CC2CC1C2", "C1CC2CCC1C2", "C1CC2CC2C1", "C1CCC2CC2C1", "C1CC1CC1CC1",
    "c:1:c:c:c:c:c1", "C1=CCCCC1", "OC=C"]
CORPUS = MOLECULES + EXTRA
KEYS = SmilesKeys(VOCAB, PAD, EOS, SEP)
RZ = SmilesRandomizer(VOCAB, PAD, EOS, SEP)
RESPELLED = {"C/C=C/C": "CC=CC", "C[C@@H](N)O": "CC(N)O", "CC.O": "CCO", "C(C": "CC", "C1CC": "CCC", "C?C": "CC"}


def strings(s):
    return PATTERN.findall(s)


def row_of(ids, width, start=0, fill=PAD):
    return [fill] * start + ids + [EOS] + [PAD] * (width - start - len(ids) - 1)


# ------------------------------------------------------------------------------------------ 1. the rule
def test_constants_are_shared():
    """R is one constant: the header's, ops' and the oracle's; mix on tensors is mix on ints."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gctplus_hip.h")).read()
    assert int(re.search(r"#define GCT_KEY_ROUNDS (\d+)", header).group(1)) == ops.KEY_ROUNDS == ref.ROUNDS == 3
    for name in ("GRAPH", "STRING_SYNTAX", "STRING_UNSUPPORTED"):
        assert int(re.search(rf"#define GCT_KEY_{name} (\d+)", header).group(1)) == getattr(ops, f"KEY_{name}") == getattr(ref, name)
    xs = [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 0x123456789ABCDEF, -987654321987654321]
    assert mix_tensor(torch.tensor(xs)).tolist() == [as_int64(mix(x)) for x in xs]
    assert [mix(x) for x in xs] == [ref.mix(x) for x in xs]


def test_key_equals_the_oracle_bit_for_bit():
    assert len(MOLECULES) == 39 and len(EXTRA) == 24
    for s in CORPUS + KEPT_ROWS:
        status, key = KEYS.key(ids_of(s))
        want = ref.key(strings(s))
        assert (status, key) == (want[0], ref.signed(want[1])), s
        assert -2 ** 63 <= key < 2 ** 63


def test_key_equality_is_isomorphism_on_the_corpus():
    """Every pair of the 63 graphs: equal keys <=> the backtracking test finds an isomorphism.  Neither direction is
    vacuous: the corpus holds isomorphic pairs (CC / C-C, benzene twice and with its bonds written, ...) and the pairs
    that plain refinement merges."""
    graphs = [ref.graph(strings(s)) for s in CORPUS]
    keys = []
    for s in CORPUS:
        status, key = KEYS.key(ids_of(s))
        assert status == ops.KEY_GRAPH, s
        keys.append(key)
    assert len(graphs) >= 60 and all(g is not None for g in graphs)
    same = 0
    for i, j in itertools.combinations(range(len(CORPUS)), 2):
        iso = ref.isomorphic(graphs[i], graphs[j])
        assert (keys[i] == keys[j]) == iso, (CORPUS[i], CORPUS[j], iso)
        same += iso
    assert same >= 2
    by_name = dict(zip(CORPUS, keys))
    assert by_name["CC"] == by_name["C-C"] and by_name["c1ccccc1"] == by_name["c:1:c:c:c:c:c1"]
    assert by_name["C=1CCCCC1"] == by_name["C1=CCCCC1"] and by_name["C=CO"] == by_name["OC=C"]
    assert len({by_name[s] for s in ("C1CCCCC1", "c1ccccc1", "C=1CCCCC1")}) == 3
    assert len({by_name[s] for s in ("Cc1ccccc1C", "Cc1cccc(C)c1", "Cc1ccc(C)cc1")}) == 3


def test_what_each_step_of_the_rule_is_for():
    """Without the distance profile the two WL-hard pairs merge, at any number of rounds; with it and no round, bond
    orders are not seen (CC=O / C=CO merge); the rule as stated separates both."""
    for a, b in WL_HARD:
        ga, gb = ref.graph(strings(a)), ref.graph(strings(b))
        assert not ref.isomorphic(ga, gb)
        assert ref.graph_key(*ga, rounds=8, profile=False) == ref.graph_key(*gb, rounds=8, profile=False)
        assert ref.graph_key(*ga) != ref.graph_key(*gb)
    ga, gb = ref.graph(strings("CC=O")), ref.graph(strings("C=CO"))
    assert ref.graph_key(*ga, rounds=0) == ref.graph_key(*gb, rounds=0) and ref.graph_key(*ga, rounds=1) != ref.graph_key(*gb, rounds=1)


def test_randomised_spellings_keep_the_key():
    checked = changed = 0
    for m, s in enumerate(CORPUS):
        toks = ids_of(s)
        want = KEYS.key(toks)
        for k in range(50):
            status, out, _ = RZ.randomize(toks, stream(5, k | m << 32, 0))
            assert status == ops.RAND_OK, s
            assert KEYS.key(out) == want, (s, "".join(VOCAB[t] for t in out))
            checked += 1
            changed += out != toks
    assert checked >= 3000 and changed >= checked // 2


# ------------------------------------------------------------------------------------------ 2. parts without a graph
def test_rows_without_a_graph_get_string_keys():
    eight = "S(C)(C)(C)(C)(C)(C)(C)C"                                # (the one row of KEPT_ROWS with a graph: 8 bonds)
    assert eight in KEPT_ROWS and KEYS.key(ids_of(eight))[0] == ops.KEY_GRAPH
    rows = [s for s in KEPT_ROWS if s != eight] + ["C\\C=C\\C", "C()C", "CC.O"]
    got = [KEYS.key(ids_of(s)) for s in rows]
    for s, (status, key) in zip(rows, got):
        want = ops.KEY_STRING_SYNTAX if RZ.parse(ids_of(s)) is None else ops.KEY_STRING_UNSUPPORTED
        assert status == want, s
        assert key == as_int64(KEYS.string_key(ids_of(s))) == ref.signed(ref.string_key(strings(s)))
    assert {st for st, _ in got} == {ops.KEY_STRING_SYNTAX, ops.KEY_STRING_UNSUPPORTED}
    for (a, (_, ka)), (b, (_, kb)) in itertools.combinations(zip(rows, got), 2):
        assert (ka == kb) == (ids_of(a) == ids_of(b)), (a, b)
    assert "CC.O" in KEPT_ROWS                                        # (so one pair above is equal)
    for s, plain in RESPELLED.items():
        status, key = KEYS.key(ids_of(plain))
        assert status == ops.KEY_GRAPH and key != KEYS.key(ids_of(s))[1]
        assert key != as_int64(KEYS.string_key(ids_of(plain)))      # another domain: the same tokens, another key
    V = len(VOCAB)                                                   # ids outside the vocabulary: SYNTAX, told apart
    odd = [KEYS.key([ids_of("C")[0], t]) for t in (-1, V, V + 1, 2 ** 40)]
    assert {st for st, _ in odd} == {ops.KEY_STRING_SYNTAX} and len({k for _, k in odd}) == 4


def test_labels_do_not_depend_on_the_vocabulary():
    """The atom label is the token's string, not its id: another vocabulary order gives the same keys."""
    other = VOCAB[:5] + VOCAB[5:][::-1]
    k2 = SmilesKeys(other, PAD, EOS, SEP)
    for s in CORPUS[::4] + KEPT_ROWS:
        assert k2.key(ids_of(s, other)) == KEYS.key(ids_of(s)), s


# ------------------------------------------------------------------------------------------ 3. the batch rule
def test_scaffold_part_is_keyed_on_its_own_and_rows_without_eos_have_no_key():
    mol, sca, sca2, bad = ids_of("CC(=O)Oc1ccccc1"), ids_of("c1ccccc1"), ids_of("c1ccccc"), ids_of("C/C=C/C")
    W = 48
    rows = [row_of(sca + [SEP] + mol, W, 1, 2), row_of(sca2 + [SEP] + mol, W), row_of(mol, W, 3, ids_of("N")[0]),
            row_of(bad + [SEP] + mol, W), row_of(mol + [SEP] + ids_of("C(C"), W), row_of(sca + [SEP] + mol + [SEP] + mol, W),
            [ids_of("C")[0]] * W, [PAD] * W, row_of([], W), row_of(mol, W)]
    starts = [1, 0, 3, 0, 0, 0, 0, 0, 0, W]
    got = KEYS.key_reference(torch.tensor(rows), starts)
    assert got.key.dtype == torch.int64 and got.info.dtype == torch.int32
    km, ks = KEYS.key(mol), KEYS.key(sca)
    assert KEYS.key(sca2) != ks                                      # (c1ccccc does not parse: an open ring)
    G, SY, UN = ops.KEY_GRAPH, ops.KEY_STRING_SYNTAX, ops.KEY_STRING_UNSUPPORTED
    assert got.key[0].tolist() == [km[1], ks[1]] and got.info[0].tolist() == [G, G, 10, 10]
    assert got.key[1].tolist() == [km[1], KEYS.key(sca2)[1]] and got.info[1].tolist() == [G, SY, 10, 10]
    assert got.key[2].tolist() == [km[1], 0] and got.info[2].tolist() == [G, -1, 10, 10]
    assert got.key[3].tolist() == [km[1], KEYS.key(bad)[1]] and got.info[3].tolist() == [G, UN, 10, 10]
    assert got.key[4].tolist() == [KEYS.key(ids_of("C(C"))[1], km[1]] and got.info[4].tolist() == [SY, G, 0, 0]
    assert got.info[5].tolist()[:2] == [SY, G]                       # the first <sep> splits; a second one is no SMILES token
    for r in (6, 7, 9):                                              # no <eos> in the span (row 9: an empty span)
        assert got.key[r].tolist() == [0, 0] and got.info[r].tolist() == [-1, -1, 0, 0]
    assert got.info[8].tolist() == [SY, -1, 0, 0] and got.key[8, 0] == KEYS.key([])[1]
    respelled = KEYS.key_reference(torch.tensor([row_of(ids_of("c1ccccc1OC(C)=O"), W)]), [0])
    assert respelled.key[0, 0] == km[1]
    out_of_range = KEYS.key_reference(torch.tensor(rows[:2]), [-1, W + 1])
    assert out_of_range.info.tolist() == [[-1, -1, 0, 0]] * 2
    nosep = SmilesKeys(VOCAB, PAD, EOS).key_reference(torch.tensor(rows[:1]), [1])
    assert nosep.info[0].tolist() == [SY, -1, 0, 0]


# ------------------------------------------------------------------------------------------ 4. what the keys are for
def test_first_occurrence_against_a_dict():
    g = torch.Generator().manual_seed(3)
    keys = torch.randint(-4, 5, (200,), generator=g) * 0x1234567890ABCDE
    group = torch.randint(0, 3, (200,), generator=g)
    valid = torch.rand(200, generator=g) < 0.7
    for grp, val in ((None, None), (group, None), (None, valid), (group, valid)):
        seen, want = set(), []
        for r in range(200):
            k = (int(keys[r]), None if grp is None else int(grp[r]))
            new = (val is None or bool(val[r])) and k not in seen
            want.append(new)
            if new:
                seen.add(k)
        got = first_occurrence(keys, grp, val)
        assert got.dtype == torch.bool and got.tolist() == want
    both = torch.stack([keys, keys * 0], 1)                          # [n, 2]: the molecule column; a MolKeys: its key
    assert torch.equal(first_occurrence(both), first_occurrence(keys))
    assert torch.equal(first_occurrence(MolKeys(both, torch.zeros(200, 4, dtype=torch.int32))), first_occurrence(keys))
    assert first_occurrence(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError):
        first_occurrence(keys, group[:5])
    with pytest.raises(ValueError):
        first_occurrence(keys.float())


def test_index_round_trip_contains_and_rounds(tmp_path):
    train = ["CCO", "OCC", "c1ccccc1", "C/C=C/C", "C(C", "CC(=O)O"]
    W = 12
    ys = torch.tensor([row_of(ids_of(s), W) for s in train])
    index = MolKeyIndex.from_rows(KEYS, [(ys[:4], [0] * 4), (ys[4:], [0] * 2)])
    graph_keys = sorted({KEYS.key(ids_of(s))[1] for s in ("CCO", "c1ccccc1", "CC(=O)O")})
    assert index.keys.tolist() == graph_keys and len(index) == 3 and index.rounds == ops.KEY_ROUNDS
    every = MolKeyIndex.from_rows(KEYS, [(ys, [0] * 6)], graph_only=False)
    assert len(every) == 5
    probe = torch.tensor([KEYS.key(ids_of(s))[1] for s in ("C(C)O", "CCN", "C1=CC=CC=C1", "c1ccccc1", "C/C=C/C")])
    assert index.contains(probe).tolist() == [True, False, False, True, False]
    assert every.contains(probe).tolist() == [True, False, False, True, True]
    assert MolKeyIndex(torch.zeros(0, dtype=torch.int64)).contains(probe).tolist() == [False] * 5
    assert len(MolKeyIndex.from_rows(KEYS, [])) == 0
    path = str(tmp_path / "train.keys")
    index.save(path)
    again = MolKeyIndex.load(path)
    assert torch.equal(again.keys, index.keys) and again.rounds == index.rounds
    assert torch.load(path, weights_only=True).keys() == {"keys", "rounds"}
    torch.save({"keys": index.keys, "rounds": ops.KEY_ROUNDS + 1}, path)
    with pytest.raises(ValueError, match="rounds"):
        MolKeyIndex.load(path)


def report_of(status):
    s = torch.tensor(status, dtype=torch.int32)
    return ChemReport(s, torch.full_like(s, -1), torch.zeros_like(s), torch.zeros_like(s))


def test_basic_metrics_against_hand_counted_rows():
    k = {s: KEYS.key(ids_of(s))[1] for s in ("CCO", "OCC", "C(C)O", "CCN", "c1ccccc1", "CC", "C-C")}
    assert k["CCO"] == k["OCC"] == k["C(C)O"] and k["CC"] == k["C-C"]
    rows = ["CCO", "OCC", "CCN", "c1ccccc1", "C(C)O", "CC", "C-C", "CCN"]
    keys = torch.tensor([k[s] for s in rows])
    OK, BAD = ops.CHEM_OK, ops.CHEM_VALENCE
    index = MolKeyIndex(torch.tensor([k["CCO"], k["CC"]]))
    # valid rows: OCC CCN c1ccccc1 C(C)O C-C CCN -> 6 of 8; distinct among them: CCO CCN benzene CC -> 4; not in the index: 2
    got = basic_metrics(report_of([BAD, OK, OK, OK, OK, BAD, OK, OK]), keys, index)
    assert got == {"valid": 6 / 8, "unique": 4 / 6, "novel": 2 / 4, "n": 8, "n_valid": 6, "n_unique": 4, "n_novel": 2}
    got = basic_metrics(report_of([OK] * 8), MolKeys(torch.stack([keys, keys], 1), torch.zeros(8, 4, dtype=torch.int32)))
    assert got == {"valid": 1.0, "unique": 4 / 8, "n": 8, "n_valid": 8, "n_unique": 4}
    got = basic_metrics(report_of([BAD] * 8), keys, index)
    assert got == {"valid": 0.0, "unique": 0.0, "novel": 0.0, "n": 8, "n_valid": 0, "n_unique": 0, "n_novel": 0}
    got = basic_metrics(report_of([]), torch.zeros(0, dtype=torch.int64), index)
    assert got == {"valid": 0.0, "unique": 0.0, "novel": 0.0, "n": 0, "n_valid": 0, "n_unique": 0, "n_novel": 0}
    with pytest.raises(ValueError):
        basic_metrics(report_of([OK] * 3), keys)


def test_uniqueness_reward():
    k = {s: KEYS.key(ids_of(s))[1] for s in ("CCO", "CCN", "CC")}
    keys = torch.tensor([k["CCO"], k["CCN"], k["CCO"], k["CC"], k["CCN"], k["CCO"]])
    assert uniqueness_reward(keys).tolist() == [1.0, 1.0, 0.0, 1.0, 0.0, 0.0]
    assert uniqueness_reward(keys).dtype == torch.float32
    index = MolKeyIndex(torch.tensor([k["CCN"]]))
    assert uniqueness_reward(keys, index).tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    group = torch.tensor([0, 0, 1, 1, 0, 1])
    assert uniqueness_reward(keys, group=group).tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert uniqueness_reward(keys, index, group).tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 0.0]
