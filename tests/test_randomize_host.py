"""SMILES randomisation on the host (no GPU): SmilesRandomizer.randomize -- THE statement -- against hand-written
spellings, against the independent oracle of tests/randomize_ref.py (graph equality under perm, and the oracle's own
recursive spelling token for token) and against SmilesChemistry.check; every status that keeps a part; the coin; the
distribution over spellings; the loader on "cpu"; train1's refusal of -synthetic."""
import collections
import re

import pandas as pd
import pytest
import torch

from gct_plus_amd import data, ops, synthetic
from gct_plus_amd.smiles import SmilesChemistry
from gct_plus_amd.randomize import SmilesRandomizer, stream
from tests import randomize_ref as ref
from tests.test_data_pipeline import SMILES as PIPELINE_SMILES

PATTERN = re.compile(r"(\[[^\]]+]|Br?|Cl?|N|O|S|P|F|I|b|c|n|o|s|p|\(|\)|\.|=|#|-|\+|\\|\/|:|~|@|\?|>|\*|\$|\%[0-9]{2}|[0-9])")
PAD, EOS, SEP = synthetic.PAD_ID, synthetic.EOS_ID, synthetic.SEP_ID
MOLECULES = PIPELINE_SMILES + [
    "CCO", "c1ccccc1", "Cc1ccccc1", "CC(=O)O", "C#N", "C12C3C4C1C5C2C3C45", "C1CC12CC2", "C1CCC2(CC1)CCCC2", "c1cc[nH]c1",
    "c1ccc2[nH]ccc2c1", "C[N+](=O)[O-]", "[NH3+]CC(=O)[O-]", "c1ccccc1-c1ccccc1", "C=1CCCCC1", "c1ccc2ccccc2c1",
    "C1C2CC3CC1CC(C2)C3", "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccsc1", "C12C3C1C23", "CC(C)(C)c1ccc(O)cc1", "C1CC11CC1",
    "OS(=O)(=O)c1ccccc1", "FC(F)(F)C(F)(F)F", "N#Cc1ccc(Br)cc1", "C" * 40]
VOCAB = list(synthetic.CHEM_VOCAB)
VOCAB += sorted({t for s in MOLECULES for t in PATTERN.findall(s)} - set(VOCAB))
RZ = SmilesRandomizer(VOCAB, PAD, EOS, SEP)
CHEM = SmilesChemistry(VOCAB, PAD, EOS)
RING_TOKENS = [VOCAB[i] for i in RZ.ring_ids]
STAY = 0xFFFFFFFF                                             # a shuffle word that swaps nothing: floor(w (i + 1) / 2^32) = i


def ids_of(s, vocab=VOCAB):
    return [vocab.index(t) for t in PATTERN.findall(s)]


def text(ids, vocab=VOCAB):
    return "".join(vocab[i] for i in ids)


def injected(root, atoms, swaps=()):
    """A stream that picks `root` of `atoms`, and swaps the last two list entries of the atoms in `swaps` only (their
    word 0: step i = 1 of an atom with two bonds)."""
    y = -(-root * 2 ** 32 // atoms)                           # the smallest word with floor(y * atoms / 2^32) = root
    table = {0: (0, y, 0, 0)}
    table.update({1 + 2 * a: (0, STAY, STAY, STAY) for a in swaps})
    return lambda i: table.get(i, (STAY,) * 4)


# ------------------------------------------------------------------------------------------ 1. hand-written spellings
@pytest.mark.parametrize("smiles, root, swaps, want, perm", [
    ("CCO", 0, (), "CCO", [0, 1, 2]),
    ("CCO", 2, (), "OCC", [2, 1, 0]),
    ("CCO", 1, (), "C(C)O", [1, 0, 2]),
    ("CCO", 1, (1,), "C(O)C", [1, 2, 0]),
    ("Cc1ccccc1", 0, (), "Cc1ccccc1", [0, 1, 2, 3, 4, 5, 6]),                       # rooted on the methyl
    ("Cc1ccccc1", 3, (), "c1cc(C)ccc1", [3, 2, 1, 0, 6, 5, 4]),                     # rooted in the ring
    ("C1CC12CC2", 2, (), "C12(CC1)CC2", [2, 1, 0, 3, 4]),                           # rooted at the spiro atom
    ("C1CC12CC2", 0, (), "C1CC12CC2", [0, 1, 2, 3, 4]),
    ("c1ccccc1-c1ccccc1", 6, (), "c1(-c2ccccc2)ccccc1", [6, 5, 4, 3, 2, 1, 0, 7, 8, 9, 10, 11]),
    ("C=1CCCCC1", 0, (), "C=1CCCCC1", [0, 1, 2, 3, 4, 5]),                          # the = stays with the ring closure
    ("C=1CCCCC1", 5, (), "C=1CCCCC1", [5, 4, 3, 2, 1, 0]),                          # ... written at the opening end
    ("C=1CCCCC1", 5, (5,), "C1=CCCCC1", [5, 0, 1, 2, 3, 4]),                        # ... or it becomes a chain bond
    ("C1CC11CC1", 0, (), "C1CC12CC2", [0, 1, 2, 3, 4]),                             # a number closed here is not reopened here
    ("C1CC11CC1", 4, (), "C1CC21CC2", [4, 3, 2, 1, 0]),
])
def test_injected_words_give_the_hand_written_spelling(smiles, root, swaps, want, perm):
    toks = ids_of(smiles)
    atoms = sum(1 for t in toks if RZ.words[t] & 0xFF == ops.GRAMMAR_ATOM)
    status, out, pm = RZ.randomize(toks, injected(root, atoms, swaps))
    assert (status, text(out), pm) == (ops.RAND_OK, want, perm)
    assert ref.same_graph(PATTERN.findall(smiles), PATTERN.findall(want), perm)


# ------------------------------------------------------------------------------------------ 2. many molecules, many keys
def test_every_spelling_is_the_same_graph():
    """39 molecules, 200 keys each: the output is well formed, the same labelled graph under perm (the oracle's reading),
    the oracle's own recursive spelling token for token, and SmilesChemistry.check sees what it saw before."""
    assert len(MOLECULES) >= 30
    distinct = 0
    for m, s in enumerate(MOLECULES):
        strings, toks = PATTERN.findall(s), ids_of(s)
        before = CHEM.check(toks + [EOS])
        seen = set()
        for k in range(200):
            status, out, perm = RZ.randomize(toks, stream(3, k | m << 32, 0))
            assert status == ops.RAND_OK, s
            new = [VOCAB[t] for t in out]
            assert RZ.grammar.well_formed(out + [EOS]), (s, "".join(new))
            assert ref.same_graph(strings, new, perm), (s, "".join(new), perm)
            assert ref.spell(strings, RING_TOKENS, 3, k | m << 32) == (ref.OK, new, perm), (s, "".join(new))
            after = CHEM.check(out + [EOS])
            assert (after[0], after[2], after[3]) == (before[0], before[2], before[3]), (s, "".join(new))
            seen.add(("".join(new), tuple(perm)))
        distinct += len(seen) > 1
    assert distinct == len(MOLECULES)                               # every molecule was written in more than one atom order


# ------------------------------------------------------------------------------------------ 3. parts that are kept
def row_of(ids, width, start=0, fill=PAD):
    return torch.tensor([[fill] * start + ids + [EOS] + [PAD] * (width - start - len(ids) - 1)])


@pytest.mark.parametrize("smiles, status", [
    ("C/C=C/C", ops.RAND_UNSUPPORTED), ("C[C@@H](N)O", ops.RAND_UNSUPPORTED), ("CC.O", ops.RAND_UNSUPPORTED),
    ("C1C1", ops.RAND_UNSUPPORTED), ("C=1CC#1", ops.RAND_UNSUPPORTED), ("S(C)(C)(C)(C)(C)(C)(C)(C)C", ops.RAND_UNSUPPORTED),
    ("C(C", ops.RAND_SYNTAX), ("C1CC", ops.RAND_SYNTAX), ("", ops.RAND_SYNTAX), ("C?C", ops.RAND_SYNTAX),
])
def test_unsupported_and_malformed_rows_stay_as_they_are(smiles, status):
    toks = ids_of(smiles)
    ys = row_of(toks, 20, start=2, fill=VOCAB.index("N"))
    for key in range(20):
        got = RZ.randomize_reference(ys, [2], [key], 1, p=1.0)
        assert torch.equal(got.tokens, ys)
        atoms = 0 if status == ops.RAND_SYNTAX else sum(1 for t in toks if RZ.words[t] & 0xFF == ops.GRAMMAR_ATOM)
        assert got.info.tolist() == [[status, -1, len(toks) + 1, atoms]]
        assert got.perm[0, :atoms].tolist() == list(range(atoms)) and bool((got.perm[0, atoms:] == -1).all())
    assert ref.spell(PATTERN.findall(smiles), RING_TOKENS, 1, 0)[0] == status


def test_no_ring_number_left():
    """Tetrahedrane needs three ring numbers at once whatever the root; written with 0, 1 and 2 it is a legal input of a
    vocabulary whose usable numbers (1 .. 63) are two: NO_RING for every key.  The spiro chain C1CC11CC11CC1 is written
    with one number and needs up to three: under the same vocabulary some keys spell it and some cannot."""
    vocab = ["<unk>", "<pad>", "<sos>", "<eos>", "C", "0", "1", "2", "(", ")"]
    rz = SmilesRandomizer(vocab, 1, 3)
    assert [vocab[i] for i in rz.ring_ids] == ["1", "2"]
    cage = ids_of("C01C2C0C12", vocab)
    assert SmilesChemistry(vocab, 1, 3).check(cage + [3])[0] == ops.CHEM_OK
    for key in range(50):
        got = rz.randomize_reference(row_of(cage, 12), [0], [key], 0)
        assert got.info.tolist() == [[ops.RAND_NO_RING, -1, len(cage) + 1, 4]] and got.tokens[0, :len(cage)].tolist() == cage
    chain, seen = ids_of("C1CC11CC11CC1", vocab), collections.Counter()
    for key in range(200):
        status, out, _ = rz.randomize(chain, stream(0, key, 0))
        want = ref.spell([vocab[t] for t in chain], ["1", "2"], 0, key)
        assert (status, [vocab[t] for t in out]) == want[:2]
        assert status == ops.RAND_OK or out == chain
        seen[status] += 1
    assert set(seen) == {ops.RAND_OK, ops.RAND_NO_RING} and min(seen.values()) >= 10


def test_too_long_keeps_the_part():
    """out_width one short of what the new spelling needs: TOO_LONG, the row unchanged; with one column more it fits.
    A scaffold row where only the scaffold has no room: the scaffold is kept and the molecule is still rewritten."""
    toks = ids_of("CCO")
    key = next(k for k in range(50) if len(RZ.randomize(toks, stream(0, k, 0))[1]) == 5)       # C(C)O or C(O)C
    ys = row_of(toks, 5, start=1, fill=2)
    got = RZ.randomize_reference(ys, [1], [key], 0, out_width=6)                    # <sos> + 5 tokens: no room for <eos>
    assert got.info.tolist() == [[ops.RAND_TOO_LONG, -1, 4, 3]] and got.tokens.tolist() == [ys[0].tolist() + [PAD]]
    got = RZ.randomize_reference(ys, [1], [key], 0, out_width=7)
    assert got.info.tolist() == [[ops.RAND_OK, -1, 6, 3]] and text(got.tokens[0, 1:6].tolist()) in ("C(C)O", "C(O)C")
    # scaffold CCO (grows by two for this key as part 1), molecule c1ccccc1 (never grows)
    key = next(k for k in range(200) if len(RZ.randomize(toks, stream(0, k, 1))[1]) == 5)
    mol = ids_of("c1ccccc1")
    ys = torch.tensor([toks + [SEP] + mol + [EOS]])
    got = RZ.randomize_reference(ys, [0], [key], 0, out_width=ys.shape[1] + 1)
    assert got.info[0].tolist() == [ops.RAND_OK, ops.RAND_TOO_LONG, ys.shape[1], 9]
    assert got.tokens[0, :4].tolist() == toks + [SEP]
    assert ref.same_graph(PATTERN.findall("c1ccccc1"), [VOCAB[t] for t in got.tokens[0, 4:12].tolist()],
                          [p - 3 for p in got.perm[0, 3:9].tolist()])
    got = RZ.randomize_reference(ys, [0], [key], 0, out_width=ys.shape[1] + 2)
    assert got.info[0].tolist() == [ops.RAND_OK, ops.RAND_OK, ys.shape[1] + 2, 9]
    assert text(got.tokens[0, :5].tolist()) in ("C(C)O", "C(O)C") and got.tokens[0, 5] == SEP


# ------------------------------------------------------------------------------------------ 4. the coin
def test_coin():
    n = len(MOLECULES)
    W = max(len(ids_of(s)) for s in MOLECULES) + 12
    ys = torch.cat([row_of(ids_of(s), W, start=1, fill=2) for s in MOLECULES])
    keys = torch.arange(n) + 1000
    kept = RZ.randomize_reference(ys, [1] * n, keys, 5, p=0.0)
    assert torch.equal(kept.tokens, ys) and kept.info[:, 0].tolist() == [ops.RAND_KEPT] * n
    every = RZ.randomize_reference(ys, [1] * n, keys, 5, p=1.0)
    assert every.info[:, 0].tolist() == [ops.RAND_OK] * n
    half = RZ.randomize_reference(ys, [1] * n, keys, 5, p=0.5)
    want = [ref.coin(5, int(k), 0, 0.5) for k in keys]
    assert [s == ops.RAND_OK for s in half.info[:, 0].tolist()] == want and 0 < sum(want) < n
    for r in range(n):
        assert torch.equal(half.tokens[r], (every if want[r] else kept).tokens[r])
    with pytest.raises(ValueError):
        RZ.randomize_reference(ys, [1] * n, keys, 5, p=1.5)


# ------------------------------------------------------------------------------------------ 5. the distribution
def test_cco_distribution():
    """CCO over keys 0 .. 5999 under seed 0: roots are uniform (1/3 each) and the middle atom's two orders are equally
    likely, so CCO, OCC, C(C)O, C(O)C have probabilities 1/3, 1/3, 1/6, 1/6; each count within 4 standard errors
    (36.5 and 28.9 counts).  Observed: 2045, 1959, 1009, 987 -- deviations of +1.23, -1.12, +0.31 and -0.45 standard
    errors."""
    toks, seen = ids_of("CCO"), collections.Counter()
    for key in range(6000):
        seen[text(RZ.randomize(toks, stream(0, key, 0))[1])] += 1
    print(dict(seen))
    assert set(seen) == {"CCO", "OCC", "C(C)O", "C(O)C"}
    for s, p in (("CCO", 1 / 3), ("OCC", 1 / 3), ("C(C)O", 1 / 6), ("C(O)C", 1 / 6)):
        se = (6000 * p * (1 - p)) ** 0.5
        print(s, seen[s], f"{(seen[s] - 6000 * p) / se:+.2f} se")
        assert abs(seen[s] - 6000 * p) <= 4 * se, (s, seen[s])


# ------------------------------------------------------------------------------------------ 6. the loader on "cpu"
def frames():
    rows = [{"src": s, "src_scaffold": "c1ccccc1", "src_logP": 0.1 * i, "trg_logP": 0.1 * i}
            for i, s in enumerate(PIPELINE_SMILES)]
    return pd.DataFrame(rows)


def loaders(model_type, **kw):
    f = frames()
    sep = model_type == "pscavaetf"
    strs = [("c1ccccc1<sep>" if sep else "") + s for s in PIPELINE_SMILES]
    SRC, TRG = data.Vocab.build(strs, False, sep), data.Vocab.build(strs, True, sep)
    mk = lambda bs=4, rank=0, world=1, **more: data.SmilesLoader(f, SRC, TRG, model_type, ["logP"], bs, rank, world, False, 11,
                                                                "cpu", **{**kw, **more})
    return mk, SRC, TRG


def spellings(loader, SRC, TRG, epoch):
    """{dataset item: (src string, trg string)} of one pass over a loader."""
    loader.set_epoch(epoch)
    out = {}
    idx = synthetic.shard_indices(len(PIPELINE_SMILES), loader.world, loader.rank, epoch, loader.seed, False)
    at = 0
    for b in loader:
        assert b["trg"].shape[1] == b["src"].shape[1] + 2
        for src, trg in zip(b["src"].tolist(), b["trg"].tolist()):
            s = "".join(SRC.itos[t] for t in src if t != SRC.stoi["<pad>"])
            t = "".join(TRG.itos[t] for t in trg[1:trg.index(TRG.stoi["<eos>"])])
            assert all(x == TRG.stoi["<pad>"] for x in trg[trg.index(TRG.stoi["<eos>"]) + 1:])
            out.setdefault(int(idx[at]), (s, t))
            at += 1
    return out


@pytest.mark.parametrize("model_type", ["pvaetf", "pscavaetf"])
def test_loader_randomizes_on_the_cpu(model_type):
    mk, SRC, TRG = loaders(model_type, randomize_prob=1.0)
    numbers = {int(t.lstrip("%")): t for t in sorted(TRG.itos, key=len, reverse=True)
               if re.fullmatch(r"[0-9]|%[0-9]{2}", t) and 1 <= int(t.lstrip("%")) <= 63}
    ring_tokens = [numbers[r] for r in sorted(numbers)]
    chem = SmilesChemistry(TRG.itos, TRG.stoi["<pad>"], TRG.stoi["<eos>"])
    base = spellings(mk(), SRC, TRG, 0)
    assert sorted(base) == list(range(len(PIPELINE_SMILES)))
    changed = 0
    for i, (s, t) in base.items():
        assert s == t                                                               # src and trg spell the same string
        olds = (["c1ccccc1"] if model_type == "pscavaetf" else []) + [PIPELINE_SMILES[i]]
        news = t.split("<sep>")
        assert len(news) == len(olds)
        for part, (old, new) in enumerate(zip(reversed(olds), reversed(news))):     # part 0: the molecule, 1: the scaffold
            a, b = PATTERN.findall(old), PATTERN.findall(new)
            status, want, perm = ref.spell(a, ring_tokens, 11, i, part)             # the loader's seed; epoch 0: key = i
            assert status == ref.OK and want == b, (old, new)
            assert ref.same_graph(a, b, perm)                                       # the frame's molecule, respelled
            assert chem.check([TRG.stoi[x] for x in b] + [TRG.stoi["<eos>"]])[0] == ops.CHEM_OK
            changed += a != b
    assert changed >= len(base) // 2
    other = spellings(mk(), SRC, TRG, 1)
    assert sum(other[i] != base[i] for i in base) >= len(base) // 2                 # set_epoch changes the spellings
    for bs, world in ((3, 1), (8, 1), (3, 2), (8, 2)):
        got = {}
        for rank in range(world):
            got.update(spellings(mk(bs=bs, rank=rank, world=world), SRC, TRG, 1))
        assert got == other, (bs, world)


@pytest.mark.parametrize("model_type", ["pvaetf", "pscavaetf"])
def test_loader_with_probability_zero_is_todays_loader(model_type):
    mk, SRC, TRG = loaders(model_type)
    for a, b in zip(mk(), mk(randomize_prob=0.0)):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    canon = spellings(mk(), SRC, TRG, 0)
    assert all(canon[i][1].split("<sep>")[-1] == s for i, s in enumerate(PIPELINE_SMILES))
    half = spellings(mk(randomize_prob=0.5), SRC, TRG, 0)                           # some rows rewritten, some kept
    assert 0 < sum(half[i] != canon[i] for i in canon) < len(canon)


def test_loader_refuses_a_target_token_without_a_source_id():
    mk, SRC, TRG = loaders("pvaetf")
    short = data.Vocab([t for t in SRC.itos if t != "F"])
    with pytest.raises(ValueError, match="source vocabulary"):
        data.SmilesLoader(frames(), short, TRG, "pvaetf", [], 4, 0, 1, False, 0, "cpu", randomize_prob=0.5)
    data.SmilesLoader(frames(), short, TRG, "pvaetf", [], 4, 0, 1, False, 0, "cpu")


# ------------------------------------------------------------------------------------------ 7. train1
def test_train1_refuses_synthetic_batches(tmp_path):
    from gct_plus_amd import train1
    with pytest.raises(ValueError, match="not SMILES"):
        train1.main(0, 1, ["-model_type", "vaetf", "-model_folder", str(tmp_path), "-synthetic", "64", "-randomize_prob",
                           "0.5"])
