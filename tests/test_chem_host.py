"""The chemistry check on the host: smiles.SmilesChemistry -- hand-written known answers over every status, the atom
entries of every kind of atom token, `check` against the independent oracle of tests/chem_ref.py on random walks through
the grammar and on single-token substitutions of valid molecules, validity_reward, and argument validation.  No GPU, no
native library."""
import random
import re

import pytest
import torch

from gct_plus_amd import ops, synthetic
from gct_plus_amd.smiles import ChemReport, SmilesChemistry, SmilesGrammar, chem_atom_entry
from gct_plus_amd.Train.finetune import validity_reward
from tests import chem_ref
from tests.test_grammar_host import EOS, PAD, VOCAB31, VOCAB70

CHEMV = synthetic.CHEM_VOCAB                          # VOCAB70 and what the molecules below need
assert CHEMV[:70] == VOCAB70 and len(set(CHEMV)) == len(CHEMV)
OK, SYNTAX, VALENCE, RING_BOND = ops.CHEM_OK, ops.CHEM_SYNTAX, ops.CHEM_VALENCE, ops.CHEM_RING_BOND
AROMATIC = ops.CHEM_AROMATIC
assert (OK, SYNTAX, VALENCE, RING_BOND, AROMATIC) == (chem_ref.OK, chem_ref.SYNTAX, chem_ref.VALENCE, chem_ref.RING_BOND,
                                                      chem_ref.AROMATIC) == (0, 1, 2, 3, 4)

# (SMILES, (status, position, atoms, ring_bonds)); positions count tokens, the <eos> stands behind the last one
VALID = [
    ("CCO", (OK, -1, 3, 0)),                                      # ethanol
    ("c1ccccc1", (OK, -1, 6, 1)),                                 # benzene
    ("CC(=O)O", (OK, -1, 4, 0)),                                  # acetic acid
    ("C1CC1", (OK, -1, 3, 1)),                                    # cyclopropane
    ("N#N", (OK, -1, 2, 0)),
    ("c1cc[nH]c1", (OK, -1, 5, 1)),                               # pyrrole
    ("CS(=O)(=O)C", (OK, -1, 5, 0)),                              # dimethyl sulfone
    ("C=1CCCCC=1", (OK, -1, 6, 1)),                               # both ends of the closure say `=`
    ("O=c1cccc[nH]1", (OK, -1, 7, 1)),                            # 2-pyridone
    ("CC(=O)Oc1ccccc1C(=O)O", (OK, -1, 13, 1)),                   # aspirin
    ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", (OK, -1, 14, 2)),              # caffeine
    ("c1ccc2ccccc2c1", (OK, -1, 10, 2)),                          # naphthalene
    ("c1ccncc1", (OK, -1, 6, 1)),                                 # pyridine
    ("C[N+](C)(C)C", (OK, -1, 5, 0)),
    ("CC(=O)[O-]", (OK, -1, 4, 0)),                               # acetate
    ("c1ccsc1", (OK, -1, 5, 1)),                                  # thiophene
    ("C1=CCCCC=1", (OK, -1, 6, 1)),                               # one end says `=`, the other nothing
    ("Cn1cccc1", (OK, -1, 6, 1)),
    ("c1ccoc1", (OK, -1, 5, 1)),                                  # furan
    ("FC(F)(F)c1ccccc1", (OK, -1, 10, 1)),
    ("C[n+]1ccccc1", (OK, -1, 7, 1)),
    ("CP(C)(C)=O", (OK, -1, 5, 0)),
    ("ClC(Cl)Cl.CO", (OK, -1, 6, 0)),
    ("C12CC1C2", (OK, -1, 4, 2)),                                 # bicyclobutane: two closures on one atom
    ("N[C@@H](C)C(=O)O", (OK, -1, 6, 0)),                         # alanine
    ("c1ccc(-c2ccccc2)cc1", (OK, -1, 12, 2)),                     # biphenyl
    ("[Na+].[O-]C", (OK, -1, 3, 0)),
    ("c1cc[nH+]cc1", (OK, -1, 6, 1)),                             # pyridinium
    ("BrCCBr", (OK, -1, 4, 0)),
    ("C%10CCCCC%10", (OK, -1, 6, 1)),
    ("C[Si](C)(C)C", (OK, -1, 5, 0)),
    ("O=S(=O)(O)O", (OK, -1, 5, 0)),
    ("C/C=C/C", (OK, -1, 4, 0)),
    ("[13C][2H]", (OK, -1, 2, 0)),
    ("*C*", (OK, -1, 3, 0)),
]
INVALID = [
    ("C(C)(C)(C)(C)C", (VALENCE, 0, 6, 0)),
    ("O=O=O", (VALENCE, 2, 3, 0)),
    ("F=C", (VALENCE, 0, 2, 0)),
    ("CN(C)(C)C", (VALENCE, 1, 5, 0)),
    ("C#C#C", (VALENCE, 2, 3, 0)),
    ("CO(C)C", (VALENCE, 1, 4, 0)),
    ("C[O-](C)C", (VALENCE, 1, 4, 0)),
    ("ClC(Cl)(Cl)(Cl)Cl", (VALENCE, 1, 6, 0)),
    ("c1(C)(C)cccc1", (VALENCE, 0, 7, 1)),                        # an aromatic carbon without a double bond: 1 + 4
    ("C[N+](C)(C)(C)C", (VALENCE, 1, 6, 0)),
    ("B(C)(C)(C)C", (VALENCE, 0, 5, 0)),
    ("C[nH]1cccc1", (VALENCE, 1, 6, 1)),                          # three bonds and a hydrogen on an aromatic N
    ("C=1CCCCC#1", (RING_BOND, 9, 6, 1)),                         # `=` at one end, `#` at the other
    ("C1C1", (RING_BOND, 3, 2, 1)),                               # doubles the chain bond
    ("C12CCC12", (RING_BOND, 7, 4, 2)),                           # doubles the closure in front of it
    ("C1CC1C=1CC#1", (RING_BOND, 11, 6, 2)),
    ("cc", (AROMATIC, 0, 2, 0)),
    ("cO", (AROMATIC, 0, 2, 0)),
    ("Cc", (AROMATIC, 1, 2, 0)),
    ("c1ccccc1c", (AROMATIC, 8, 7, 1)),
    ("C1CC(", (SYNTAX, 5, 0, 0)),                                 # the <eos> at index 5 finds a branch and a ring open
    ("C)C", (SYNTAX, 1, 0, 0)),
    ("C==C", (SYNTAX, 2, 0, 0)),
    ("CC%70", (SYNTAX, 2, 0, 0)),                                 # ring numbers end at 63
]
CHEM = SmilesChemistry(CHEMV, PAD, EOS)


_TOKEN = re.compile(r"\[[^\]]+\]|Br|Cl|%\d\d|.")     # the test's own reading of a SMILES string: no native scanner


def ids_of(smiles, vocab=CHEMV):
    return [vocab.index(t) for t in _TOKEN.findall(smiles)]


def strings(vocab, ids):
    """What the oracle reads: "<pad>" / "<eos>" for the two special ids, None for an id outside the vocabulary."""
    return ["<pad>" if t == PAD else "<eos>" if t == EOS else vocab[t] if 0 <= t < len(vocab) else None for t in ids]


def walk(gr, G, rng, length, p_eos):
    """`length` tokens of a random walk through gr.allowed under the budget G; <eos> is taken only when nothing else is
    allowed or with probability p_eos; behind the end of the walk the row writes pad."""
    toks = []
    while len(toks) < length:
        ok = gr.allowed(toks, G - len(toks))
        if len(ok) > 1 and rng.random() >= p_eos:
            ok = [t for t in ok if t != EOS]
        toks.append(rng.choice(ok))
    return toks


def walks(vocab, budget, count, seed):
    gr = SmilesGrammar(vocab, PAD, EOS)
    rng = random.Random(seed)
    return [walk(gr, budget, rng, budget + 1, 0.3) for _ in range(count)]


def substitutions(vocab, seed, per_token=6):
    """Every single-token substitution of the valid known answers by `per_token` random tokens each (ids 5 and up: every
    token but the five special ones), with <eos> and one <pad> behind."""
    rng = random.Random(seed)
    out = []
    for s, _ in VALID:
        ids = ids_of(s, vocab)
        for k in range(len(ids)):
            for _ in range(per_token):
                m = list(ids)
                m[k] = rng.randrange(5, len(vocab))
                out.append(m + [EOS, PAD])
    return out


def mixed_set():
    """[(vocabulary, generated ids)]: walks over V31 and V70 at budgets 8 and 14, and the substitutions."""
    rows = []
    for vocab, seed in ((VOCAB31, 31), (VOCAB70, 70)):
        for budget in (8, 14):
            rows += [(vocab, w) for w in walks(vocab, budget, 120, seed + budget)]
    rows += [(CHEMV, m) for m in substitutions(CHEMV, 1)]
    return rows


# ---------------------------------------------------------------------------------------------- known answers
def test_known_answers_cover_every_status():
    assert len(VALID) >= 25 and len(INVALID) >= 15
    assert {a[0] for _, a in INVALID} == {SYNTAX, VALENCE, RING_BOND, AROMATIC}


@pytest.mark.parametrize("smiles,want", VALID + INVALID, ids=[s for s, _ in VALID + INVALID])
def test_known_answer(smiles, want):
    ids = ids_of(smiles) + [EOS, PAD, PAD]
    assert tuple(CHEM.check(ids)) == want
    assert CHEM.valid(ids) == (want[0] == OK)
    assert chem_ref.verdict(strings(CHEMV, ids)) == want          # the oracle agrees with the hand-written answer


def test_degenerate_spans():
    C = CHEMV.index("C")
    assert tuple(CHEM.check([])) == (SYNTAX, 0, 0, 0)                               # an empty span
    assert tuple(CHEM.check([EOS])) == (SYNTAX, 0, 0, 0)                            # <eos> alone
    assert tuple(CHEM.check([C, C])) == (SYNTAX, 2, 0, 0)                           # no <eos>: the span's length
    assert tuple(CHEM.check([C, -1, EOS])) == (SYNTAX, 1, 0, 0)
    assert tuple(CHEM.check([C, len(CHEMV), EOS])) == (SYNTAX, 1, 0, 0)
    assert tuple(CHEM.check([C, EOS, PAD, C, PAD])) == (SYNTAX, 3, 0, 0)            # junk behind the <eos>
    assert tuple(CHEM.check([C, EOS, PAD, PAD])) == (OK, -1, 1, 0)
    for ids in ([], [EOS], [C, C], [C, -1, EOS], [C, len(CHEMV), EOS], [C, EOS, PAD, C, PAD]):
        assert chem_ref.verdict(strings(CHEMV, ids)) == tuple(CHEM.check(ids))


# ------------------------------------------------------------------------------------------------ atom entries
ENTRIES = {   # token: (cap, H, aromatic, carbon-like)
    "B": (3, 0, False, False), "C": (4, 0, False, True), "N": (3, 0, False, False), "O": (2, 0, False, False),
    "F": (1, 0, False, False), "P": (5, 0, False, False), "S": (6, 0, False, False), "Cl": (1, 0, False, False),
    "Br": (1, 0, False, False), "I": (5, 0, False, False), "b": (3, 0, True, False), "c": (4, 0, True, True),
    "n": (3, 0, True, False), "o": (2, 0, True, False), "s": (6, 0, True, False), "p": (5, 0, True, False),
    "*": (None, 0, False, False),
    "[nH]": (3, 1, True, False), "[N+]": (4, 0, False, True), "[O-]": (1, 0, False, False), "[n+]": (4, 0, True, True),
    "[nH+]": (4, 1, True, True), "[c-]": (3, 0, True, False), "[B-]": (4, 0, False, True),
    "[C@@H]": (4, 1, False, True), "[13C]": (4, 0, False, True), "[2H]": (None, 0, False, False),
    "[Na+]": (None, 0, False, False), "[Si]": (4, 0, False, False), "[se]": (None, 0, True, False),
    "[S@]": (6, 0, False, False), "[I+]": (None, 0, False, False),
    "[C@@@H]": (None, 0, False, False),                           # unreadable: three chirality marks
    "[NH4+]": (4, 4, False, True), "[O-2]": (None, 0, False, False), "[Cl+]": (6, 0, False, False),
    "[Al]": (None, 0, False, False), "[P+]": (4, 0, False, False), "[N++]": (3, 0, False, False),
    "[N+-]": (None, 0, False, False), "[Br]": (1, 0, False, False), "[Br-]": (None, 0, False, False),
}


@pytest.mark.parametrize("token", list(ENTRIES))
def test_atom_entry(token):
    want = ENTRIES[token]
    got = chem_atom_entry(token)
    assert (got[0], got[1], bool(got[2]), bool(got[3])) == want
    assert chem_ref.atom_reading(token) == want
    if token in CHEMV:                                            # and the table word holds the same
        w = CHEM.words[CHEMV.index(token)]
        cap = None if w & 15 == ops.CHEM_NO_CAP else w & 15
        assert (cap, (w >> 4) & 15, bool((w >> 8) & 1), bool((w >> 9) & 1), (w >> 12) & 7) == want + (0,)


def test_table_words_of_the_other_tokens():
    for tok, order in (("-", 1), ("=", 2), ("#", 3), ("$", 4), (":", 1), ("/", 1), ("\\", 1), ("~", 1)):
        assert CHEM.words[CHEMV.index(tok)] == ops.CHEM_NO_CAP | (order << 12), tok
    for tok in ("(", ")", "1", "%12", ".", "<eos>", "<pad>", "<unk>", "%70", "?"):
        assert CHEM.words[CHEMV.index(tok)] == ops.CHEM_NO_CAP, tok
    assert CHEM.chem.dtype == torch.int32 and CHEM.chem.tolist() == CHEM.words and len(CHEM) == len(CHEMV)
    table, chem = CHEM.device_tables("cpu")
    assert table is CHEM.device_tables("cpu")[0] and chem is CHEM.device_tables("cpu")[1]   # copied once
    assert torch.equal(table, CHEM.grammar.table) and torch.equal(chem, CHEM.chem)


# --------------------------------------------------------------------------------------- check against the oracle
def test_check_equals_the_oracle_on_the_mixed_set():
    rows = mixed_set()
    count = {}
    checkers = {}
    for vocab, ids in rows:
        ch = checkers.setdefault(len(vocab), SmilesChemistry(vocab, PAD, EOS))
        want = chem_ref.verdict(strings(vocab, ids))
        assert tuple(ch.check(ids)) == want, [vocab[t] for t in ids]
        count[want[0]] = count.get(want[0], 0) + 1
    print(f"{len(rows)} rows; the oracle's statuses: {dict(sorted(count.items()))}")
    for status in (OK, SYNTAX, VALENCE, RING_BOND, AROMATIC):     # no branch hides: the REFERENCE finds every status
        assert count.get(status, 0) >= 5, (status, count)
    assert count[OK] >= 0.1 * len(rows), count


def test_check_reference_is_check_per_row():
    rng = random.Random(4)
    rows = [m for _, m in mixed_set()[-40:]]
    W = 3 + max(len(m) for m in rows)
    ys = torch.randint(0, len(CHEMV), (len(rows), W), generator=torch.Generator().manual_seed(4))
    lens = []
    for r, m in enumerate(rows):
        t0 = rng.randint(0, W - len(m))
        ys[r, t0:] = PAD
        ys[r, t0:t0 + len(m)] = torch.tensor(m)
        lens.append(t0)
    rep = CHEM.check_reference(ys, lens)
    assert isinstance(rep, ChemReport) and all(t.dtype == torch.int32 and t.shape == (len(rows),) for t in rep)
    for r, m in enumerate(rows):
        assert tuple(int(t[r]) for t in rep) == tuple(CHEM.check(ys[r, lens[r]:].tolist()))
    empty = CHEM.check_reference(ys, [W] * len(rows))                               # start == W: an empty span
    assert empty.status.tolist() == [SYNTAX] * len(rows) and empty.position.tolist() == [0] * len(rows)


# ------------------------------------------------------------------------------------------------ the reward
def test_validity_reward_plain_and_shaped():
    rep = ChemReport(torch.tensor([OK, SYNTAX, VALENCE, RING_BOND, AROMATIC, OK], dtype=torch.int32),
                     torch.tensor([-1, 10, 0, 3, 5, -1], dtype=torch.int32),
                     torch.tensor([3, 0, 6, 2, 7, 1], dtype=torch.int32), torch.tensor([0, 0, 0, 1, 1, 0], dtype=torch.int32))
    plain = validity_reward(rep)
    assert plain.dtype == torch.float32 and plain.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    shaped = validity_reward(rep, shaped=True, lengths=[10, 10, 8, 4, 20, 5])
    assert shaped.dtype == torch.float32 and shaped.tolist() == [1.0, 1.0, 0.0, 0.75, 0.25, 1.0]
    assert validity_reward(rep, shaped=True, lengths=20).tolist() == [1.0, 0.5, 0.0, 0.15000000596046448, 0.25, 1.0]
    with pytest.raises(ValueError):
        validity_reward(rep, shaped=True)
    with pytest.raises(ValueError):
        validity_reward(rep, shaped=True, lengths=[10, 10])
    with pytest.raises(ValueError):
        validity_reward(rep, shaped=True, lengths=[10, 10, 8, 0, 20, 5])


# ------------------------------------------------------------------------------------------------ validation
def test_value_errors():
    with pytest.raises(ValueError):
        SmilesChemistry(["<unk>", "<pad>", "<sos>", "<eos>", "(", ")"], 1, 3)       # no atom token
    with pytest.raises(ValueError):
        SmilesChemistry(CHEMV, PAD, len(CHEMV))                                     # no <eos> inside the vocabulary
    ys = torch.full((3, 300), PAD)
    for call in (CHEM.check_reference, CHEM.check_rows):          # (check_rows raises before it reaches the device)
        with pytest.raises(ValueError):
            call(ys, [43, 44, 45])                                                  # a span of 257 columns
        with pytest.raises(ValueError):
            call(ys, [301, 44, 44])                                                 # past the row
        with pytest.raises(ValueError):
            call(ys, [-1, 44, 44])
        with pytest.raises(ValueError):
            call(ys, [44, 44])                                                      # one per row
        with pytest.raises(ValueError):
            call(ys.float(), [44, 44, 44])
        with pytest.raises(ValueError):
            call(ys[0], [44])
    assert CHEM.check_reference(ys, [44, 300, 44]).status.tolist() == [SYNTAX] * 3  # 256 columns are fine
