"""Grammar-constrained decoding on the host: smiles.SmilesGrammar -- the classification of a vocabulary, known answers of
`allowed`, the closed form of the length budget against a breadth-first search, random walks through `allowed` against an
independent recursive-descent parser of the token strings, and argument validation.  No GPU, no native library."""
import random

import pytest
import torch

from gct_plus_amd import data, ops, synthetic
from gct_plus_amd.decode import TOP_K_FLOOR, KVDecoder, sample_filter_reference
from gct_plus_amd.smiles import (G_END, GRAMMAR_START, SmilesGrammar, check_grammar, grammar_class, grammar_min_finish,
                                 grammar_step)

PAD, SOS, EOS, SEP = synthetic.PAD_ID, synthetic.SOS_ID, synthetic.EOS_ID, synthetic.SEP_ID
VOCAB31 = synthetic.GRAMMAR_VOCAB                     # one token of every class, the scaffold models' 31 target tokens
# 70 tokens: more than one wave's 64 lanes
VOCAB70 = VOCAB31 + ["[N+]", "[O-]", "P", "I", "B", "b", "s", "p", "*", "\\", ":", "~", "$", "0", "4", "5", "6", "7",
                     "8", "9", "%01", "%10", "%11", "%63", "%64", "%99", "?", ">", "[Na+]", "[se]", "[Si]", "[2H]",
                     "[13C]", "[S@]", "[P@@]", "[B-]", "[I+]", "[nH+]", "[c-]"]
assert len(VOCAB31) == 31 and len(VOCAB70) == 70 and len(set(VOCAB70)) == 70


def grammar(vocab=VOCAB31):
    return SmilesGrammar(vocab, PAD, EOS)


def ids(gr, text):
    """Token ids of a space-separated token string."""
    return [gr.itos.index(t) for t in text.split()]


def names(gr, tokens):
    return sorted(gr.itos[t] for t in tokens)


# ------------------------------------------------------------------------------- the independent checker
_CHK_ATOMS = {"B", "Br", "C", "Cl", "N", "O", "S", "P", "F", "I", "b", "c", "n", "o", "s", "p", "*"}
_CHK_BONDS = {"=", "#", "-", "/", "\\", ":", "~", "$"}


def _kind(tok):
    """atom / bond / open / close / ring / dot / eos / pad / other of a token STRING (the checker's own reading)."""
    if tok is None:
        return "end"
    if tok.startswith("[") and tok.endswith("]") and len(tok) > 2 or tok in _CHK_ATOMS:
        return "atom"
    if tok in _CHK_BONDS:
        return "bond"
    if tok.isdigit() and len(tok) == 1 or (len(tok) == 3 and tok[0] == "%" and tok[1:].isdigit()):
        return "ring" if int(tok.lstrip("%")) < 64 else "other"
    return {"(": "open", ")": "close", ".": "dot", "<eos>": "eos", "<pad>": "pad"}.get(tok, "other")


class _Reject(Exception):
    pass


class _Parser:
    """Recursive descent over token strings:
         line   := chain ('.' chain)* <eos> <pad>*           with no ring left open at <eos>
         chain  := unit (bond? unit)*
         unit   := atom (bond? ring)* branch*                a ring number does not open and close on one atom
         branch := '(' bond? chain ')'"""

    def __init__(self, toks):
        self.t, self.i, self.open = list(toks), 0, set()

    def peek(self, k=0):
        return _kind(self.t[self.i + k]) if self.i + k < len(self.t) else "end"

    def take(self, kind):
        if self.peek() != kind:
            raise _Reject(f"token {self.i}: {kind} expected, got {self.peek()}")
        self.i += 1
        return self.t[self.i - 1]

    def line(self):
        self.chain()
        while self.peek() == "dot":
            self.i += 1
            self.chain()
        self.take("eos")
        if self.open:
            raise _Reject(f"rings left open: {sorted(self.open)}")
        while self.i < len(self.t):
            self.take("pad")

    def chain(self):
        self.unit()
        while self.peek() == "atom" or (self.peek() == "bond" and self.peek(1) == "atom"):
            if self.peek() == "bond":
                self.i += 1
            self.unit()

    def unit(self):
        self.take("atom")
        opened = set()
        while self.peek() == "ring" or (self.peek() == "bond" and self.peek(1) == "ring"):
            if self.peek() == "bond":
                self.i += 1
            r = int(self.take("ring").lstrip("%"))
            if r in self.open:
                if r in opened:
                    raise _Reject(f"ring {r} closes on the atom that opened it")
                self.open.discard(r)
            else:
                self.open.add(r)
                opened.add(r)
        while self.peek() == "open":
            self.i += 1
            if self.peek() == "bond":
                self.i += 1
            self.chain()
            self.take("close")


def parses(token_strings):
    """True when the generated token strings (the <eos> and any <pad> behind it included) are a well-formed line."""
    try:
        _Parser(token_strings).line()
        return True
    except _Reject:
        return False


def test_the_checker_itself():
    good = ["C <eos>", "C C ( = O ) O <eos> <pad> <pad>", "c 1 c c c c c 1 <eos>", "C 1 C C 1 1 C C 1 <eos>",
            "C = 1 C C = 1 <eos>", "C ( C ) ( C ) C <eos>", "C . C <eos>", "C %12 C C %12 <eos>", "C ( - C ) C <eos>",
            "[nH] 1 c c c c 1 <eos>", "C 1 2 C C 1 C 2 <eos>", "C ( C ( C ) ) C <eos>"]
    bad = ["<eos>", "C", "C (", "C ( ) <eos>", "C ) <eos>", "C 1 1 <eos>", "C 1 C <eos>", "C = <eos>", "C = = C <eos>",
           "= C <eos>", "1 C <eos>", "C ( = 1 C ) <eos>", "C ( C . C ) <eos>", "C . <eos>", "C ( C <eos>",
           "C <eos> C", "C @ <eos>", "C %70 C %70 <eos>", "C ( C ) 1 C 1 <eos>", "C ( C ) = 1 C 1 <eos>", "C . . C <eos>",
           "C <sep> <eos>", "C ( 1 ) C 1 <eos>"]
    for s in good:
        assert parses(s.split()), s
    for s in bad:
        assert not parses(s.split()), s


# ---------------------------------------------------------------------------------------------- classification
def test_classification_of_a_vocabulary_with_every_class():
    gr = grammar()
    want = {"C": ops.GRAMMAR_ATOM, "c": ops.GRAMMAR_ATOM, "Br": ops.GRAMMAR_ATOM, "Cl": ops.GRAMMAR_ATOM,
            "[nH]": ops.GRAMMAR_ATOM, "[C@@H]": ops.GRAMMAR_ATOM, "=": ops.GRAMMAR_BOND, "#": ops.GRAMMAR_BOND,
            "-": ops.GRAMMAR_BOND, "/": ops.GRAMMAR_BOND, "(": ops.GRAMMAR_OPEN, ")": ops.GRAMMAR_CLOSE,
            "1": ops.GRAMMAR_RING, "3": ops.GRAMMAR_RING, "%12": ops.GRAMMAR_RING, "%70": ops.GRAMMAR_BANNED,
            ".": ops.GRAMMAR_DOT, "<eos>": ops.GRAMMAR_EOS, "<pad>": ops.GRAMMAR_PAD, "<unk>": ops.GRAMMAR_BANNED,
            "<sos>": ops.GRAMMAR_BANNED, "<sep>": ops.GRAMMAR_BANNED, "@": ops.GRAMMAR_BANNED, "+": ops.GRAMMAR_BANNED}
    for tok, cls in want.items():
        assert gr.classes[gr.itos.index(tok)] == cls, tok
    assert gr.rings[gr.itos.index("1")] == 1 and gr.rings[gr.itos.index("%12")] == 12
    assert len(gr) == 31 and gr.table.dtype == torch.int32 and gr.table.shape == (31,)
    assert int(gr.table[gr.itos.index("%12")]) == ops.GRAMMAR_RING | (12 << 8)
    g70 = grammar(VOCAB70)
    assert g70.rings[g70.itos.index("%01")] == 1 and g70.classes[g70.itos.index("%01")] == ops.GRAMMAR_RING
    assert g70.rings[g70.itos.index("%63")] == 63 and g70.classes[g70.itos.index("%64")] == ops.GRAMMAR_BANNED
    for tok in ("?", ">", "%99"):
        assert g70.classes[g70.itos.index(tok)] == ops.GRAMMAR_BANNED, tok
    for tok in ("\\", ":", "~", "$"):
        assert g70.classes[g70.itos.index(tok)] == ops.GRAMMAR_BOND, tok
    assert grammar_class("%123") == (ops.GRAMMAR_BANNED, 0) and grammar_class("[]") == (ops.GRAMMAR_BANNED, 0)
    # every token's class agrees with the checker's own reading of the string
    kinds = {ops.GRAMMAR_ATOM: "atom", ops.GRAMMAR_BOND: "bond", ops.GRAMMAR_OPEN: "open", ops.GRAMMAR_CLOSE: "close",
             ops.GRAMMAR_RING: "ring", ops.GRAMMAR_DOT: "dot", ops.GRAMMAR_EOS: "eos", ops.GRAMMAR_PAD: "pad",
             ops.GRAMMAR_BANNED: "other"}
    for tok, cls in zip(g70.itos, g70.classes):
        assert kinds[cls] == _kind(tok), tok


def test_open_is_banned_without_close():
    vocab = [t for t in VOCAB31 if t != ")"]
    gr = grammar(vocab)
    assert gr.classes[vocab.index("(")] == ops.GRAMMAR_BANNED
    assert "(" not in names(gr, gr.allowed(ids(gr, "C"), 9))


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers():
    gr = grammar()
    atoms = sorted(t for t in VOCAB31 if _kind(t) == "atom")
    bonds = sorted(t for t in VOCAB31 if _kind(t) == "bond")
    assert names(gr, gr.allowed([], 9)) == atoms                                   # START: an atom
    assert "1" not in names(gr, gr.allowed(ids(gr, "C 1"), 9))                       # no ring closed on its own atom
    assert {"2", "3", "%12"} <= set(names(gr, gr.allowed(ids(gr, "C 1"), 9)))
    assert names(gr, gr.allowed(ids(gr, "C ("), 9)) == sorted(atoms + bonds)         # after '(' an atom or a bond
    assert names(gr, gr.allowed(ids(gr, "C ( ="), 9)) == atoms                       # 'C ( = 1' is forbidden
    assert "<eos>" not in names(gr, gr.allowed(ids(gr, "C 1 C"), 9))                 # a ring is open
    assert "<eos>" not in names(gr, gr.allowed(ids(gr, "C ( C"), 9))                 # a branch is open
    assert "<eos>" in names(gr, gr.allowed(ids(gr, "C 1 C C 1"), 9)) and "<eos>" in names(gr, gr.allowed(
        ids(gr, "C ( C ) C"), 9))
    assert names(gr, gr.allowed(ids(gr, "C 1 C"), 2)) == ["1"]                       # two slots: close the ring, <eos>
    assert names(gr, gr.allowed(ids(gr, "C ( C"), 2)) == [")"]
    assert names(gr, gr.allowed(ids(gr, "C"), 1)) == ["<eos>"]
    assert names(gr, gr.allowed([], 2)) == atoms
    assert "." not in names(gr, gr.allowed(ids(gr, "C ( C"), 9)) and "." in names(gr, gr.allowed(ids(gr, "C"), 9))
    # close, then open the same number again on one atom: it is open and was opened here, so it cannot close now
    assert "1" in names(gr, gr.allowed(ids(gr, "C 1 C C 1"), 9))
    assert "1" not in names(gr, gr.allowed(ids(gr, "C 1 C C 1 1"), 9))
    assert gr.state(ids(gr, "C 1 C C 1 1")) == (2, 0, 2, 2)                          # RING, depth 0, open {1}, here {1}
    # finished, or past the budget: pad only
    assert names(gr, gr.allowed(ids(gr, "C <eos>"), 5)) == ["<pad>"]
    assert names(gr, gr.allowed(ids(gr, "C <eos> <pad>"), 5)) == ["<pad>"]
    assert names(gr, gr.allowed(ids(gr, "C C"), 0)) == ["<pad>"]
    with pytest.raises(ValueError):
        gr.allowed(ids(gr, "C ( = 1"), 9)
    assert gr.well_formed(ids(gr, "C 1 C C 1 <eos> <pad>")) and not gr.well_formed(ids(gr, "C 1 C C 1"))
    assert not gr.well_formed(ids(gr, "C 1 1 <eos>")) and not gr.well_formed(ids(gr, "C <eos> C"))
    assert not gr.well_formed(ids(gr, "C <sep> <eos>")) and not gr.well_formed([])


def test_mask_reference_known_rows():
    gr = grammar()
    x = torch.randn(4, 31, generator=torch.Generator().manual_seed(0))
    ys = torch.full((4, 8), PAD)
    ys[0, :4] = torch.tensor([SOS] + ids(gr, "C 1 C"))
    ys[1, :3] = torch.tensor([SOS, 7, SEP])                                          # prefix <sos> N <sep>, nothing generated
    ys[2, :3] = torch.tensor([SOS] + ids(gr, "C <eos>"))
    ys[3, :3] = torch.tensor([SOS, 7, SEP])                                          # still inside its prefix
    out = gr.mask_reference(x, ys, [1, 3, 1, 3], [4, 3, 3, 2], [5, 6, 6, 6])
    keep = torch.isfinite(out)
    assert torch.equal(out[keep], x[keep]) and bool((out[~keep] == -float("inf")).all())
    assert names(gr, keep[0].nonzero().view(-1).tolist()) == ["1"]                   # 2 slots left
    assert names(gr, keep[1].nonzero().view(-1).tolist()) == names(gr, gr.allowed([], 6))
    assert names(gr, keep[2].nonzero().view(-1).tolist()) == ["<pad>"]
    assert torch.equal(out[3], x[3])


# ------------------------------------------------------------------------------------------- the length budget
RINGS = 3
ALPHABET = ([(ops.GRAMMAR_ATOM, 0), (ops.GRAMMAR_BOND, 0), (ops.GRAMMAR_OPEN, 0), (ops.GRAMMAR_CLOSE, 0),
             (ops.GRAMMAR_DOT, 0), (ops.GRAMMAR_EOS, 0)] + [(ops.GRAMMAR_RING, r) for r in range(RINGS)])


def successors(state):
    return {s for s in (grammar_step(state, c, r) for c, r in ALPHABET) if s is not None}


def shortest_finish(state, limit=24):
    """Breadth-first search: tokens on the shortest allowed path from `state` to END."""
    seen, frontier = {state}, {state}
    for dist in range(limit + 1):
        if any(s[0] == G_END for s in frontier):
            return dist
        frontier = {n for s in frontier for n in successors(s)} - seen
        seen |= frontier
    raise AssertionError(f"no finish within {limit} tokens of {state}")


def test_min_finish_is_the_breadth_first_distance():
    reach, frontier = {GRAMMAR_START}, {GRAMMAR_START}
    for _ in range(7):
        frontier = {n for s in frontier for n in successors(s)} - reach
        reach |= frontier
    live = sorted(s for s in reach if s[0] != G_END)
    print(f"{len(live)} states within 7 tokens and {RINGS} ring numbers, and END")
    assert len(live) + 1 == 340                                                      # (the count the closed form was derived on)
    wrong = [(s, grammar_min_finish(s), shortest_finish(s)) for s in live if grammar_min_finish(s) != shortest_finish(s)]
    assert not wrong, wrong[:5]
    assert grammar_min_finish((G_END, 0, 0, 0)) == 0 and grammar_min_finish(GRAMMAR_START) == 2


# ------------------------------------------------------------------------------------------------ random walks
def test_random_walks_end_well_formed():
    """20 000 walks drawing uniformly from `allowed`, budgets 2 .. 14: the allowed set is never empty, the walk ends with
    <eos> inside its budget, and the independent parser accepts it."""
    rng = random.Random(5)
    seen_classes, longest = set(), 0
    for vocab in (VOCAB31, VOCAB70):
        gr = grammar(vocab)
        for _ in range(10000):
            G = rng.randint(2, 14)
            toks = []
            while not toks or toks[-1] != EOS:
                assert len(toks) < G, (G, [gr.itos[t] for t in toks])
                ok = gr.allowed(toks, G - len(toks))
                assert ok, (G, [gr.itos[t] for t in toks])
                toks.append(rng.choice(ok))
            strings = [gr.itos[t] for t in toks]
            assert parses(strings), strings
            assert gr.well_formed(toks)
            assert gr.allowed(toks, G - len(toks)) == [PAD]
            seen_classes |= {gr.classes[t] for t in toks}
            longest = max(longest, len(toks))
    assert longest == 14 and seen_classes == set(range(ops.GRAMMAR_EOS + 1))       # every class was walked through


def test_well_formed_agrees_with_the_checker_on_corrupted_walks():
    """Walks with one token replaced at random: SmilesGrammar.well_formed and the parser give the same verdict, and both
    verdicts occur."""
    rng = random.Random(9)
    gr = grammar()
    verdicts = {True: 0, False: 0}
    for _ in range(3000):
        G = rng.randint(2, 12)
        toks = []
        while not toks or toks[-1] != EOS:
            toks.append(rng.choice(gr.allowed(toks, G - len(toks))))
        toks[rng.randrange(len(toks))] = rng.randrange(len(gr))
        verdict = parses([gr.itos[t] for t in toks])
        assert gr.well_formed(toks) == verdict, [gr.itos[t] for t in toks]
        verdicts[verdict] += 1
    assert min(verdicts.values()) > 100, verdicts


# ------------------------------------------------------------------------------------------------ validation
def tiny_model(vocab):
    from gct_plus_amd.Model import model_dict
    torch.manual_seed(0)
    return model_dict["vaetf"](len(vocab) - 2, len(vocab), dropout=0.0, nconds=0, use_cond2lat=True, N=1, d_model=32,
                               dff=64, h=4, latent_dim=8).eval()


def test_bad_arguments_raise():
    with pytest.raises(ValueError, match="atom"):
        SmilesGrammar(["<unk>", "<pad>", "<sos>", "<eos>", "=", "(", ")", "1"], 1, 3)
    with pytest.raises(ValueError, match="<eos>"):
        SmilesGrammar(["<unk>", "<pad>", "C"], 1, 3)
    gr = grammar()
    for budget in (1, 0, torch.tensor([5, 1, 7])):
        with pytest.raises(ValueError, match="at least 2"):
            check_grammar(gr, 31, budget)
    check_grammar(gr, 31, 2), check_grammar(None, 31, 0), check_grammar(gr, 31, torch.tensor([2, 9]))
    with pytest.raises(ValueError, match="vocabulary"):
        check_grammar(gr, 30, 5)
    with pytest.raises(ValueError):
        check_grammar("C", 31, 5)
    kd = KVDecoder(tiny_model(VOCAB31), PAD, SOS, EOS)                               # no start(): no device state
    ys0 = torch.full((3, 1), SOS)
    with pytest.raises(ValueError, match="at least 2"):
        kd.generate(ys0, 2, grammar=gr)                                              # G = max_strlen - 1 = 1
    with pytest.raises(ValueError, match="vocabulary"):
        kd.generate(ys0, 12, grammar=grammar(VOCAB70))


def test_sampler_refuses_beam_search_with_well_formed():
    from gct_plus_amd.Inference.sampling_tool import get_sampler
    model = tiny_model(VOCAB31)
    SRC, TRG = data.Vocab(["<unk>", "<pad>"] + VOCAB31[4:]), data.Vocab(VOCAB31)
    kw = dict(latent_dim=8, max_strlen=12, device="cpu")
    with pytest.raises(ValueError, match="well_formed"):
        get_sampler("vaetf", model, SRC, TRG, decode_algo="beam", beam_size=2, well_formed=True, **kw)
    sp = get_sampler("vaetf", model, SRC, TRG, decode_algo="multinomial", well_formed=True, **kw)
    assert isinstance(sp.grammar, SmilesGrammar) and len(sp.grammar) == 31
    assert get_sampler("vaetf", model, SRC, TRG, **kw).grammar is None
    with pytest.raises(ValueError, match="grammar"):                                 # beam search takes no grammar
        sp.decode_beams(torch.zeros(2, 5, 8), torch.full((2, 1), SOS), torch.ones(2, 1, 5, dtype=torch.bool))


# ------------------------------------------------------------------------- the sampling filter on masked logits
def test_a_forbidden_token_weighs_exactly_zero_through_the_filter():
    """A -inf logit (what the grammar mask writes) has weight exactly 0 at every stage of sample_filter_reference: in
    particular top-k's 1e-6 floor goes to the finite tokens outside the top k only."""
    inf = float("inf")
    x = torch.tensor([[2.0, -inf, 1.0, 0.0, -inf, -1.0]])
    p = torch.softmax(x, -1)[0].double()
    w = sample_filter_reference(x, top_k=2)[0].double()
    want = torch.tensor([float(p[0]), 0.0, float(p[2]), TOP_K_FLOOR, 0.0, TOP_K_FLOOR], dtype=torch.float64)
    assert w[1] == 0 and w[4] == 0
    assert torch.allclose(w, want / want.sum(), atol=1e-7, rtol=0)
    gr = grammar()
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(40, 31, generator=g) * 2
    ys = torch.full((40, 6), PAD)
    ys[:, 0] = SOS
    hist = ids(gr, "C ( =")
    ys[:20, 1:4] = torch.tensor(hist)
    masked = gr.mask_reference(logits, ys, 1, [4] * 20 + [1] * 20, 9)
    off = torch.isneginf(masked)
    assert bool(off.any(1).all()) and bool((~off).any(1).all())
    for kw in (dict(top_k=3), dict(top_k=30), dict(top_p=0.8), dict(temperature=1.7),
               dict(top_k=3, top_p=0.9, temperature=1.5)):
        w = sample_filter_reference(masked, **kw)
        assert bool((w[off] == 0).all()), kw
        assert bool(torch.isfinite(w).all()) and torch.allclose(w.sum(1), torch.ones(40), atol=1e-5), kw
        assert bool((w[~off].view(40, -1).max(1).values > 0).all()), kw
