"""Murcko scaffolds on the host (no GPU): SmilesScaffolds.scaffold -- THE statement -- against a hand-written table,
against the independent oracle of tests/scaffold_ref.py (membership, kept tokens and key) over the molkey corpus, and by
the properties of its spelling (it parses back to the key; the scaffold of a scaffold is itself; the key does not depend
on how the molecule was spelled); a vocabulary without [nH]; the batch rule's spans; and the front ends that need no
GPU: scaffold_match / scaffold_reward / scaffold_metrics on hand-made keys, tools/add_scaffolds.py's columns."""
import importlib.util
import os
import re

import pandas as pd
import pytest
import torch

from gct_plus_amd import ops
from gct_plus_amd.smiles import ChemReport
from gct_plus_amd.molkey import scaffold_metrics
from gct_plus_amd.randomize import stream
from gct_plus_amd.scaffold import ScaffoldRows, SmilesScaffolds, scaffold_match
from gct_plus_amd.Train.finetune import scaffold_reward
from tests import scaffold_ref as ref
from tests.test_molkey_host import CORPUS
from tests.test_randomize_host import EOS, PAD, PATTERN, SEP, VOCAB, ids_of, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCA = SmilesScaffolds(VOCAB, PAD, EOS, SEP)
OK, ACYCLIC, SYNTAX, UNSUPPORTED = ops.SCA_OK, ops.SCA_ACYCLIC, ops.SCA_SYNTAX, ops.SCA_UNSUPPORTED

# (molecule, status, the scaffold as the rule spells it, atoms kept) -- written by hand from the rule's text
TABLE = [
    ("O=C1CCCCC1C", OK, "O=C1CCCCC1", 7),                          # the rule's examples
    ("CC(C)=C1CCCC1", OK, "C=C1CCCC1", 6),
    ("c1ccccc1C(=O)c1ccccc1", OK, "c1ccccc1C(=O)c1ccccc1", 14),
    ("O=C(c1ccccc1)c1ccccc1", OK, "O=C(c1ccccc1)c1ccccc1", 14),
    ("CC(=O)c1ccccc1", OK, "c1ccccc1", 6),
    ("Cn1cccc1", OK, "[nH]1cccc1", 5),
    ("c1ccn(-c2ccccc2)c1", OK, "c1ccn(-c2ccccc2)c1", 11),
    ("c1ccccc1-c1ccccc1", OK, "c1ccccc1-c1ccccc1", 12),            # ring systems and linkers
    ("c1ccc2ccccc2c1", OK, "c1ccc2ccccc2c1", 10),
    ("C1CCC2(CC1)CCCC2", OK, "C1CCC2(CC1)CCCC2", 10),
    ("C12C3C4C1C5C2C3C45", OK, "C12C3C4C1C1C2C3C41", 8),           # (a ring takes the lowest free number)
    ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", OK, "[nH]1cnc2c1c(=O)[nH]c(=O)[nH]2", 11),
    ("c1ccccc1S(=O)(=O)c1ccccc1", OK, "c1ccccc1S(=O)(=O)c1ccccc1", 15),
    ("OS(=O)(=O)c1ccccc1", OK, "c1ccccc1", 6),
    ("c1ccccc1C(C)Cc1ccccc1", OK, "c1ccccc1CCc1ccccc1", 14),
    ("Cc1ccccc1", OK, "c1ccccc1", 6),                              # substituents go
    ("CC(C)(C)c1ccc(O)cc1", OK, "c1ccccc1", 6),
    ("N#Cc1ccc(Br)cc1", OK, "c1ccccc1", 6),
    ("C1C2CC3CC1CC(C2)C3", OK, "C1C2CC3CC1CC(C2)C3", 10),
    ("c1ccc2[nH]ccc2c1", OK, "c1ccc2[nH]ccc2c1", 9),
    ("C1CC11CC1", OK, "C1CC12CC2", 5),
    ("C=1CCCCC1", OK, "C=1CCCCC1", 6),
    ("CCO", ACYCLIC, "", 0),                                       # rows without a scaffold
    ("CC(=O)O", ACYCLIC, "", 0),
    ("FC(F)(F)C(F)(F)F", ACYCLIC, "", 0),
    ("C", ACYCLIC, "", 0),
    ("C[C@@H](N)O", UNSUPPORTED, "", 0),
    ("CC.O", UNSUPPORTED, "", 0),
    ("C(C", SYNTAX, "", 0),
]


def row_of(ids, width, start=0, fill=PAD):
    return [fill] * start + ids + [EOS] + [PAD] * (width - start - len(ids) - 1)


# ------------------------------------------------------------------------------------------ 1. the rule
def test_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "gctplus_hip.h")).read()
    names = ("OK", "ACYCLIC", "SYNTAX", "UNSUPPORTED", "NO_TOKEN", "NO_RING", "TOO_LONG")
    for k, name in enumerate(names):
        assert int(re.search(rf"#define GCT_SCA_{name} (\d+)", header).group(1)) == getattr(ops, f"SCA_{name}") == k
    assert "gct_smiles_scaffold" in header


@pytest.mark.parametrize("smiles, status, want, kept", TABLE, ids=[t[0] for t in TABLE])
def test_the_hand_written_table(smiles, status, want, kept):
    got_status, tokens, member, key = SCA.scaffold(ids_of(smiles))
    assert (got_status, text(tokens), sum(1 for m in member if m)) == (status, want, kept)
    atoms = sum(1 for t in ids_of(smiles) if SCA.randomizer.words[t] & 0xFF == ops.GRAMMAR_ATOM)
    assert len(member) == (atoms if status in (OK, ACYCLIC) else 0)
    if status == OK:
        assert (ops.KEY_GRAPH, key) == SCA.keys.key(ids_of(want)) and key != 0
    else:
        assert key == 0


def test_examples_of_the_rule_by_key():
    """The rule's examples as the rule's text writes them: another spelling of the same scaffold has the same key."""
    for mol, sca in (("Cn1cccc1", "c1cc[nH]c1"), ("CC(C)=C1CCCC1", "C1CCCC1=C"), ("O=C1CCCCC1C", "C1CCCCC1=O"),
                     ("c1ccccc1C(C)Cc1ccccc1", "c1ccc(CCc2ccccc2)cc1")):
        assert SCA.scaffold(ids_of(mol))[3] == SCA.keys.key(ids_of(sca))[1], mol
    same = lambda a, b: SCA.scaffold(ids_of(a))[3] == SCA.scaffold(ids_of(b))[3]        # noqa: E731
    assert same("Cc1ccccc1", "OS(=O)(=O)c1ccccc1") and not same("O=C1CCCCC1", "C1CCCCC1")
    assert not same("Cn1cccc1", "c1ccn(-c2ccccc2)c1") and not same("c1ccccc1", "C1CCCCC1")
    member = SCA.scaffold(ids_of("O=C1CCCCC1C"))[2]
    assert member == [2, 1, 1, 1, 1, 1, 1, 0]


def test_membership_tokens_and_key_equal_the_oracle_on_the_corpus():
    """Every distinct corpus entry: the peel's core and the oracle's brute-force ring bonds agree atom for atom, the kept
    tokens are the oracle's, and the key is the oracle's key of the induced subgraph."""
    distinct = sorted(set(CORPUS))
    with_core = 0
    for s in distinct:
        status, tokens, member, key = SCA.scaffold(ids_of(s))
        want = ref.scaffold(PATTERN.findall(s))
        assert want is not None and status in (OK, ACYCLIC), s
        assert member == want[0], s
        assert (status == OK) == bool(want[1]), s
        if status == OK:
            with_core += 1
            atoms = [VOCAB[t] for t in tokens if SCA.randomizer.words[t] & 0xFF == ops.GRAMMAR_ATOM]
            assert sorted(atoms) == sorted(want[1]), s
            assert key == ref.molkey_ref.signed(want[2]), s
    assert len(distinct) == 61 and with_core >= 40


def test_the_oracle_agrees_on_the_table_too():
    for smiles, status, want, kept in TABLE:
        got = ref.scaffold(PATTERN.findall(smiles))
        if status in (SYNTAX, UNSUPPORTED):
            assert got is None, smiles
        else:
            assert got[0] == SCA.scaffold(ids_of(smiles))[2] and len(got[1]) == kept, smiles


# ------------------------------------------------------------------------------------------ 2. the spelling's properties
def test_the_spelling_parses_back_and_is_a_fixed_point():
    """For every corpus and table molecule with a scaffold: SmilesKeys.key of the spelling is the returned key, every
    atom of the spelling is kept, and the scaffold of the scaffold has the same key and the same spelling."""
    seen = 0
    for s in sorted(set(CORPUS) | {t[0] for t in TABLE}):
        status, tokens, member, key = SCA.scaffold(ids_of(s))
        if status != OK:
            continue
        seen += 1
        assert SCA.keys.key(tokens) == (ops.KEY_GRAPH, key), s
        again = SCA.scaffold(tokens)
        assert again[0] == OK and again[1] == tokens and again[3] == key, (s, text(tokens), text(again[1]))
        assert all(m in (1, 2) for m in again[2]) and len(again[2]) == sum(1 for m in member if m)
    assert seen >= 55


def test_the_key_does_not_depend_on_the_spelling():
    """8 randomised spellings of every corpus molecule: the scaffold's key and the number of atoms kept are unchanged."""
    moved = 0
    for m, s in enumerate(sorted(set(CORPUS))):
        ids = ids_of(s)
        status, tokens, member, key = SCA.scaffold(ids)
        for k in range(8):
            st, new, _ = SCA.randomizer.randomize(ids, stream(5, k | m << 32, 0), 1.0)
            assert st == ops.RAND_OK
            got = SCA.scaffold(new)
            assert (got[0], got[3], sum(1 for x in got[2] if x)) == (status, key, sum(1 for x in member if x)), (s, text(new))
            moved += got[1] != tokens
    assert moved > 50                                              # (the spelling itself may differ: the key is the identity)


def test_a_vocabulary_without_nh():
    vocab = [t for t in VOCAB if t != "[nH]"]
    sc = SmilesScaffolds(vocab, vocab.index(VOCAB[PAD]), vocab.index(VOCAB[EOS]))
    assert sc.nh_id is None and sc.n_id is not None and SCA.nh_id is not None
    status, tokens, member, key = sc.scaffold(ids_of("Cn1cccc1", vocab))
    assert (status, tokens, member, key) == (ops.SCA_NO_TOKEN, [], [0, 1, 1, 1, 1, 1], 0)
    status, tokens, _, key = sc.scaffold(ids_of("c1ccn(-c2ccccc2)c1", vocab))
    assert status == OK and text(tokens, vocab) == "c1ccn(-c2ccccc2)c1" and key == SCA.scaffold(ids_of("c1ccn(-c2ccccc2)c1"))[3]
    assert ref.scaffold(PATTERN.findall("Cn1cccc1"), has_nh=False)[1] is None


def test_room_and_too_long():
    ids = ids_of("c1ccccc1-c1ccccc1")
    assert SCA.scaffold(ids, room=len(ids))[0] == OK
    status, tokens, member, key = SCA.scaffold(ids, room=len(ids) - 1)
    assert (status, tokens, sum(member)) == (ops.SCA_TOO_LONG, [], 12) and key == SCA.scaffold(ids)[3]


# ------------------------------------------------------------------------------------------ 3. the batch rule
def test_reference_rows_spans_and_given_parts():
    mol, sca, wrong = ids_of("Cc1ccccc1"), ids_of("c1ccccc1"), ids_of("C1CCCCC1")
    W = 24
    rows = [row_of(mol, W), row_of(sca + [SEP] + mol, W), row_of(wrong + [SEP] + mol, W), row_of(mol, W, start=3, fill=7),
            [PAD] * W, row_of(ids_of("CCO"), W), row_of(ids_of("C(C") + [SEP] + mol, W), row_of(ids_of("C(C"), W),
            row_of(mol, W)]
    starts = [0, 0, 0, 3, 0, 0, 0, 0, W + 1]
    got = SCA.scaffold_reference(torch.tensor(rows), starts)
    assert isinstance(got, ScaffoldRows) and got.tokens.dtype == got.key.dtype == torch.int64
    assert got.info.dtype == got.member.dtype == torch.int32
    assert tuple(got.tokens.shape) == (9, W) and tuple(got.member.shape) == (9, W) and tuple(got.key.shape) == (9, 2)
    key = SCA.keys.key(sca)[1]
    assert got.info.tolist() == [[OK, -1, 6, 8], [OK, ops.KEY_GRAPH, 6, 8], [OK, ops.KEY_GRAPH, 6, 8], [OK, -1, 6, 8],
                                 [-1, -1, 0, 0], [ACYCLIC, -1, 0, 0], [OK, ops.KEY_STRING_SYNTAX, 6, 8], [SYNTAX, -1, 0, 0],
                                 [-1, -1, 0, 0]]
    assert got.key[:, 0].tolist() == [key, key, key, key, 0, 0, key, 0, 0]
    assert got.key[:, 1].tolist() == [0, key, SCA.keys.key(wrong)[1], 0, 0, 0, SCA.keys.key(ids_of("C(C"))[1], 0, 0]
    assert got.tokens[0].tolist() == row_of(sca, W) and got.tokens[3].tolist() == row_of(sca, W)
    assert got.tokens[4].tolist() == [PAD] * W and got.tokens[5].tolist() == [EOS] + [PAD] * (W - 1)
    assert got.member[0].tolist() == [0] + [1] * 6 + [-1] * (W - 7) and got.member[5].tolist() == [0] * 3 + [-1] * (W - 3)
    assert got.member[7].tolist() == [-1] * W and got.member[4].tolist() == [-1] * W
    assert scaffold_match(got).tolist() == [False, True, False, False, False, False, False, False, False]
    narrow = SCA.scaffold_reference(torch.tensor(rows[:1]), [0], out_width=8)
    assert narrow.info.tolist() == [[ops.SCA_TOO_LONG, -1, 6, 0]] and narrow.tokens.tolist() == [[EOS] + [PAD] * 7]
    assert SCA.scaffold_reference(torch.tensor(rows[:1]), [0], out_width=9).tokens.tolist() == [sca + [EOS]]
    with pytest.raises(ValueError):
        SCA.scaffold_reference(torch.tensor(rows), starts[:3])
    with pytest.raises(ValueError):
        SCA.scaffold_reference(torch.tensor(rows), starts, out_width=0)


# ------------------------------------------------------------------------------------------ 4. the front ends
def hand_made(key, info):
    n = len(key)
    return ScaffoldRows(torch.zeros(n, 4, dtype=torch.int64), torch.tensor(key, dtype=torch.int64),
                        torch.tensor(info, dtype=torch.int32), torch.zeros(n, 4, dtype=torch.int32))


def test_reward_and_metrics_on_hand_made_keys():
    G, S = ops.KEY_GRAPH, ops.KEY_STRING_SYNTAX
    sca = hand_made([[5, 5], [5, 5], [6, 5], [5, 5], [0, 0], [7, 7], [5, 5], [9, 9]],
                    [[OK, G, 6, 8], [OK, G, 6, 8], [OK, G, 6, 8], [OK, S, 6, 8], [ACYCLIC, G, 0, 0], [OK, -1, 5, 5],
                     [OK, G, 6, 8], [ops.SCA_NO_RING, G, 3, 0]])
    match = [True, True, False, False, False, False, True, False]
    assert scaffold_match(sca).tolist() == match
    reward = scaffold_reward(sca)
    assert reward.dtype == torch.float32 and reward.tolist() == [float(m) for m in match] and not reward.requires_grad
    status = torch.tensor([0, 0, 0, 0, 0, 0, 1, 0], dtype=torch.int32)       # row 6 is not valid
    report = ChemReport(status, status, status, status)
    got = scaffold_metrics(report, sca)
    assert got == {"same_scaffold": 2 / 7, "n_scaffolds": 3, "n": 8, "n_valid": 7, "n_same": 2}
    mol = torch.tensor([11, 11, 11, 12, 13, 14, 11, 15])
    got = scaffold_metrics(report, sca, mol)
    assert got["unique_on_scaffold"] == 6 / 7 and got["n_scaffolds"] == 3       # (rows 0 and 1: one molecule on one scaffold)
    none = ChemReport(*(torch.ones(8, dtype=torch.int32),) * 4)
    assert scaffold_metrics(none, sca, mol)["same_scaffold"] == 0.0
    with pytest.raises(ValueError):
        scaffold_metrics(ChemReport(*(status[:3],) * 4), sca)


def test_add_scaffolds_columns_on_the_cpu(tmp_path):
    spec = importlib.util.spec_from_file_location("add_scaffolds", os.path.join(ROOT, "tools", "add_scaffolds.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    smiles = ["Cc1ccccc1", "CCO", "Cn1cccc1", "C[C@@H](N)O", "O=C1CCCCC1C", "C(C", "c1ccccc1-c1ccccc1"]
    want = ["c1ccccc1", "", "[nH]1cccc1", "", "O=C1CCCCC1", "", "c1ccccc1-c1ccccc1"]
    got, counts = tool.scaffold_column(smiles, chunk=3, device="cpu")
    assert got == want and dict(counts) == {"OK": 4, "ACYCLIC": 1, "UNSUPPORTED": 1, "SYNTAX": 1}
    frame = pd.DataFrame({"src": smiles, "src_logP": range(7), "trg": smiles, "trg_logP": range(7)})
    out, _ = tool.add_columns(frame, chunk=4, device="cpu")
    assert list(out.columns) == ["src", "src_scaffold", "src_logP", "trg", "trg_scaffold", "trg_logP"]
    assert out["src_scaffold"].tolist() == want and out["trg_scaffold"].tolist() == want
    assert list(frame.columns) == ["src", "src_logP", "trg", "trg_logP"]
    only = tool.add_columns(pd.DataFrame({"smiles": smiles[:2]}), smiles_col="smiles", device="cpu")[0]
    assert list(only.columns) == ["smiles", "src_scaffold"]
    src, dst = tmp_path / "in.csv", tmp_path / "out.csv"
    frame.to_csv(src, index=False)
    tool.main([str(src), str(dst), "--device", "cpu", "--chunk", "2"])
    back = pd.read_csv(dst, keep_default_na=False)
    assert back["src_scaffold"].tolist() == want and list(back.columns) == list(out.columns)
