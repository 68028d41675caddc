"""The shared host layer of the SMILES modules (no GPU): smiles.row_spans -- THE batch rule -- against a literal table;
the five *_reference methods agree on which rows are absent and on the atoms of a molecule; the launch prelude of the six
*_rows methods raises the same errors with each module's own wording, before anything reaches the device library; one
sampler holds one grammar, one randomiser and one SmilesKeys."""
import pytest
import torch

from gct_plus_amd import data, ops
from gct_plus_amd.descriptor import SmilesDescriptors
from gct_plus_amd.fingerprint import SmilesFingerprints
from gct_plus_amd.molkey import SmilesKeys
from gct_plus_amd.scaffold import SmilesScaffolds
from gct_plus_amd.smiles import SmilesChemistry, launch_rows, row_spans
from tests.test_randomize_host import EOS, PAD, RZ, SEP, VOCAB, ids_of

W = 12
KEYS = SmilesKeys(VOCAB, PAD, EOS, SEP, randomizer=RZ)
FPS, DESC = SmilesFingerprints(VOCAB, PAD, EOS, SEP, keys=KEYS), SmilesDescriptors(VOCAB, PAD, EOS, SEP, keys=KEYS)
SCA = SmilesScaffolds(VOCAB, PAD, EOS, SEP, keys=KEYS)
CHEM = SmilesChemistry(VOCAB, PAD, EOS, grammar=RZ.grammar)
C, O = ids_of("C")[0], ids_of("O")[0]

# (what, the row before padding, start, length, scaffold, molecule): molecule None is an absent row
CASES = [
    ("start 0", ids_of("CCO") + [EOS], 0, 12, None, ids_of("CCO")),
    ("start in the middle", [PAD] * 3 + ids_of("C1CC1") + [EOS], 3, 9, None, ids_of("C1CC1")),
    ("start = W: an empty span", ids_of("CCO") + [EOS], W, 0, None, None),
    ("start = W + 1", ids_of("CCO") + [EOS], W + 1, 0, None, None),
    ("start -1", ids_of("CCO") + [EOS], -1, 0, None, None),
    ("no <eos>", [C] * W, 2, 10, None, None),
    ("<eos> in the span's first column", [C] * 4 + [EOS], 4, 8, None, []),
    ("tokens behind <eos>", ids_of("CC") + [EOS, O, O], 0, 12, None, ids_of("CC")),
    ("one <sep>", [PAD] + ids_of("C1CC1") + [SEP] + ids_of("CC") + [EOS], 1, 11, ids_of("C1CC1"), ids_of("CC")),
    ("two <sep>", [C, SEP, C, SEP, O, EOS], 0, 12, [C], [C, SEP, O]),
    ("a <sep> behind <eos>", ids_of("CO") + [EOS, SEP, C], 0, 12, None, ids_of("CO")),
]
YS = torch.tensor([row + [PAD] * (W - len(row)) for _, row, *_ in CASES], dtype=torch.int64)
STARTS = [c[2] for c in CASES]
ABSENT = [c[5] is None for c in CASES]
IN_RANGE = [r for r, s in enumerate(STARTS) if 0 <= s <= W]


# -------------------------------------------------------------------------------------------------- 1. the span rule
def test_row_spans_against_the_table():
    got = row_spans(YS, STARTS, EOS, SEP)
    assert len(got) == len(CASES)
    for sp, (what, _, start, length, scaffold, molecule), row in zip(got, CASES, YS.tolist()):
        assert (sp.row, sp.start) == (row, start), what
        assert (sp.length, sp.scaffold, sp.molecule) == (length, scaffold, molecule), what
    for sp, (what, _, start, length, scaffold, molecule) in zip(row_spans(YS, STARTS, EOS, None), CASES):     # no <sep> id
        whole = None if molecule is None else ([] if scaffold is None else scaffold + [SEP]) + molecule
        assert (sp.length, sp.scaffold, sp.molecule) == (length, None, whole), what
    assert row_spans(YS.to(torch.int32), torch.tensor(STARTS), EOS, SEP) == got            # any integer dtype, any holder


def test_row_spans_width_limit():
    wide = torch.full((2, 300), C, dtype=torch.int64)
    wide[:, 299] = EOS
    at, over = row_spans(wide, [44, 43], EOS, SEP)
    assert (at.length, at.scaffold, at.molecule) == (256, None, [C] * 255)
    assert (over.length, over.scaffold, over.molecule) == (0, None, None)
    assert row_spans(wide, [44, 43], EOS, SEP, max_span=257)[1].length == 257


def test_row_spans_refuses_other_shapes():
    for bad in (YS.float(), YS[0], YS[:, :0], YS.bool()):
        with pytest.raises(ValueError, match="ys must"):
            row_spans(bad, STARTS, EOS, SEP)
    with pytest.raises(ValueError, match="start must be 11 integers"):
        row_spans(YS, STARTS[:-1], EOS, SEP)


# ------------------------------------------------------------------------------------- 2. the five references agree
def test_the_references_agree_on_absent_rows_and_atoms():
    n = len(CASES)
    keys, fps, desc, sca = (o(YS, STARTS) for o in (KEYS.key_reference, FPS.fp_reference, DESC.desc_reference,
                                                    SCA.scaffold_reference))
    rnd = RZ.randomize_reference(YS, STARTS, torch.arange(n), 0)
    want = torch.tensor(ABSENT)
    assert torch.equal(keys.info[:, 0] == -1, want) and torch.equal(fps.info[:, 0] == -1, want)
    assert torch.equal(desc.status == -1, want) and torch.equal(sca.info[:, 0] == -1, want)
    # the randomiser marks an absent row (SYNTAX, -1, ...), which a present molecule that does not parse and has no
    # scaffold shares (the `<eos>` first row: an empty molecule); the keys tell the two apart
    unparsed = (keys.info[:, 0] == ops.KEY_STRING_SYNTAX) & (keys.info[:, 1] == -1)
    assert unparsed.tolist() == [c[0].startswith("<eos> in") for c in CASES]
    assert torch.equal((rnd.info[:, 0] == ops.RAND_SYNTAX) & (rnd.info[:, 1] == -1), want | unparsed)
    assert rnd.info[:, 2][want].tolist() == [c[3] for c in CASES if c[5] is None]        # the span's length, or 0
    graph = keys.info[:, 0] == ops.KEY_GRAPH
    assert graph.tolist() == [c[5] is not None and len(c[5]) > 0 and SEP not in c[5] for c in CASES]
    atoms = keys.info[:, 2][graph]
    assert atoms.tolist() == [3, 3, 2, 2, 2]
    assert torch.equal(fps.info[:, 2][graph], atoms) and torch.equal(desc.heavy_atoms[graph], atoms)
    assert torch.equal((sca.member >= 0).sum(1).to(torch.int32)[graph], atoms)


# ------------------------------------------------------------------------------------------ 3. the launch prelude
LAUNCHES = [
    ("the keys take at most 256", "start", KEYS.key_rows),
    ("the fingerprints take at most 256", "start", FPS.fp_rows),
    ("the descriptors take at most 256", "start", DESC.desc_rows),
    ("the scaffolds take at most 256", "start", SCA.scaffold_rows),
    ("the randomiser takes at most 256", "start", lambda ys, st: RZ.randomize_rows(ys, st, torch.arange(ys.shape[0]), 0)),
    ("the check takes at most 256", "prefix_lens", CHEM.check_rows),
]


@pytest.mark.parametrize("noun, name, rows", LAUNCHES, ids=[noun.split()[1] for noun, _, _ in LAUNCHES])
def test_launch_checks_raise_on_the_host(noun, name, rows):
    wide = torch.full((2, 300), C, dtype=torch.int64)
    with pytest.raises(ValueError, match=f"a span of 257 columns: {noun}"):
        rows(wide, [44, 43])
    for bad in ([0, W + 1], [-1, 0]):
        with pytest.raises(ValueError, match=rf"{name} must lie in \[0, {W}\] \(the row width\)"):
            rows(YS[:2], bad)
    with pytest.raises(ValueError, match=rf"{name} must have shape \[2\]"):
        rows(YS[:2], [0, 0, 0])
    with pytest.raises(ValueError, match="ys must hold integer token ids"):
        rows(YS[:2].float(), [0, 0])
    with pytest.raises(ValueError, match=r"ys must be \[n, W >= 1\] token rows"):
        rows(YS[0], [0])
    with pytest.raises(ValueError, match="ys must"):                                  # ys is judged before start
        rows(YS[0], [W + 1])


def test_launch_rows_makes_int64_rows_with_unit_column_stride():
    wider = torch.arange(3 * 2 * W, dtype=torch.int32).view(3, 2 * W)
    view = wider[:, ::2]
    assert view.stride(1) == 2
    ys, st = launch_rows(view, [0, 5, W], "the keys take")
    assert ys.dtype == torch.int64 and ys.stride(1) == 1 and torch.equal(ys, view.to(torch.int64))
    assert st.dtype == torch.int32 and st.tolist() == [0, 5, W]
    ys, st = launch_rows(YS[IN_RANGE], torch.tensor(STARTS)[IN_RANGE], "the keys take")
    assert torch.equal(ys, YS[IN_RANGE]) and st.tolist() == [STARTS[r] for r in IN_RANGE]
    one = torch.zeros(4, 1, dtype=torch.int64)[:, ::3]                                 # one column: no stride to mend
    assert launch_rows(one, [0, 1, 0, 1], "the keys take")[0].shape == (4, 1)


# ------------------------------------------------------------------------------------- 4. one of each per vocabulary
def test_one_sampler_holds_one_grammar_one_randomiser_and_one_keys():
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    from tests.test_grammar_host import tiny_model
    SRC, TRG = data.Vocab(["<unk>", "<pad>"] + VOCAB[4:]), data.Vocab(VOCAB)
    sp = get_sampler("vaetf", tiny_model(VOCAB), SRC, TRG, latent_dim=8, max_strlen=12, device="cpu", well_formed=True)
    assert sp.scaffolds.keys is sp.keys and sp.fingerprinter.keys is sp.keys and sp.describer.keys is sp.keys
    assert sp.randomizer is sp.keys.randomizer and sp.scaffolds.randomizer is sp.randomizer
    assert sp.chemistry.grammar is sp.randomizer.grammar and sp.grammar is sp.chemistry.grammar
    plain = get_sampler("vaetf", tiny_model(VOCAB), SRC, TRG, latent_dim=8, max_strlen=12, device="cpu")
    assert plain.grammar is None and plain.chemistry.grammar is plain.keys.grammar
    # without the arguments every object builds its own, as before
    alone = SmilesScaffolds(VOCAB, PAD, EOS, SEP)
    assert alone.keys is not KEYS and alone.keys.randomizer is not RZ and alone.randomizer is alone.keys.randomizer
    assert SmilesChemistry(VOCAB, PAD, EOS).grammar is not RZ.grammar
