"""The chemistry check on the device: gct_smiles_check (ops.smiles_check, SmilesChemistry.check_rows) against
SmilesChemistry.check_reference, all four int32 columns exactly, with the output pre-filled with a sentinel that must not
survive -- the mixed set of tests/test_chem_host.py at n = 37, spans longer than a wave, degenerate rows -- and the front
ends on the tiny model: Sampling.check_rows on constrained and free decodes, validity_reward into reinforce_step."""
import random

import pytest
import torch

from gct_plus_amd import data, synthetic
from gct_plus_amd.smiles import SmilesChemistry, SmilesGrammar
from tests.test_chem_host import (AROMATIC, CHEMV, EOS, INVALID, OK, PAD, RING_BOND, SYNTAX, VALENCE, VALID, VOCAB31,
                                  VOCAB70, ids_of, mixed_set, walk)
from tests.test_mixed_scaffold_decode_gpu import TINY, mixed_prefixes

pytestmark = pytest.mark.gpu

SENT = -77
CHEMS = {len(v): SmilesChemistry(v, PAD, EOS) for v in (VOCAB31, VOCAB70, CHEMV)}
_MIXED = {}


@pytest.fixture(scope="module")
def ops():
    from gct_plus_amd import ops as _ops
    _ops._L()
    return _ops


def mixed_rows(V):
    """The generated ids of the host test's mixed set over the vocabulary of V tokens (built once)."""
    if not _MIXED:
        for vocab, ids in mixed_set():
            _MIXED.setdefault(len(vocab), []).append(ids)
    return _MIXED[V]


def launch(ops, ch, ys, starts):
    """ops.smiles_check into a sentinel-filled output -> int32 [n, 4] on the CPU, no sentinel left."""
    table, chem = ch.device_tables("cuda")
    out = torch.full((ys.shape[0], 4), SENT, dtype=torch.int32, device="cuda")
    got = ops.smiles_check(ys.cuda(), torch.as_tensor(starts, dtype=torch.int32).cuda(), table, chem, out=out)
    assert got is out
    out = out.cpu()
    assert not bool((out == SENT).any())
    return out


def same(out, ref):
    want = torch.stack(list(ref), 1)
    bad = (out != want).any(1).nonzero().view(-1).tolist()
    assert not bad, [(r, out[r].tolist(), want[r].tolist()) for r in bad[:5]]


# --------------------------------------------------------------------------------------- 1. the mixed set at n = 37
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("V", [31, 70, len(CHEMV)], ids=["V31", "V70", "chem"])
def test_mixed_set_equals_the_reference(ops, V, layout):
    """n = 37 rows a launch (not a multiple of the 4 rows of a workgroup), W = 40, until the vocabulary's rows of the
    mixed set are used up.  Every row has random ids in front of its start; a quarter of the rows, chosen at random so
    that every wave of a workgroup gets both kinds, also have random ids behind a pad region of 0 .. 3 tokens (the
    reference calls the first of them a SYNTAX offence: on every row they would leave no graph verdict to compare), the
    others pad to the end of the row."""
    ch, rows = CHEMS[V], mixed_rows(V)
    n, W = 37, 40
    rng = random.Random(V + len(layout))
    g = torch.Generator().manual_seed(V)
    seen = set()
    for lo in range(0, len(rows), n):
        part = [rows[(lo + r) % len(rows)] for r in range(n)]
        starts = [rng.randint(1, 7) for _ in range(n)] if layout == "mixed" else [3] * n
        ys = torch.randint(0, V, (n, W), generator=g)
        for r, ids in enumerate(part):
            t0, k = starts[r], len(ids)
            junk = t0 + k + rng.randint(0, 3) if rng.random() < 0.25 else W
            ys[r, t0:junk] = PAD
            ys[r, t0:t0 + k] = torch.tensor(ids)
        ref = ch.check_reference(ys, starts)
        same(launch(ops, ch, ys, starts), ref)
        same(torch.stack(list(ch.check_rows(ys.cuda(), starts)), 1).cpu(), ref)
        seen |= set(ref.status.tolist())
    assert seen == {OK, SYNTAX, VALENCE, RING_BOND, AROMATIC} or V == 31           # (V31 has no ring-bond case for sure)
    assert {OK, SYNTAX, VALENCE, AROMATIC} <= seen


def test_known_answers_on_the_device(ops):
    """The host test's hand-written molecules as device rows, each with its exact four numbers: the closures that double
    a chain bond or an earlier closure and those whose ends disagree are reached for sure, not by a walk's luck.  Pad
    to the end of the row, mixed starts, and the same rows once more with junk behind one pad."""
    ch = CHEMS[len(CHEMV)]
    cases = VALID + INVALID
    n, W = len(cases), 40
    rng = random.Random(5)
    starts = [rng.randint(0, 7) for _ in range(n)]
    ys = torch.randint(0, len(CHEMV), (n, W), generator=torch.Generator().manual_seed(5))
    dirty = ys.clone()
    ends = []
    for r, (s, _) in enumerate(cases):
        ids = ids_of(s) + [EOS]
        ys[r, starts[r]:] = PAD
        ys[r, starts[r]:starts[r] + len(ids)] = torch.tensor(ids)
        ends.append(len(ids) + 1)                                                    # the first column behind one pad
        dirty[r, starts[r]:starts[r] + ends[r]] = ys[r, starts[r]:starts[r] + ends[r]]
        dirty[r, starts[r] + ends[r]] = CHEMV.index("C")
    out = launch(ops, ch, ys, starts)
    assert [tuple(row) for row in out.tolist()] == [want for _, want in cases]
    same(out, ch.check_reference(ys, starts))
    out = launch(ops, ch, dirty, starts)
    assert [tuple(row) for row in out.tolist()] == [                                # (an earlier offence stays first)
        (SYNTAX, w[1] if w[0] == SYNTAX else e, 0, 0) for (_, w), e in zip(cases, ends)]
    same(out, ch.check_reference(dirty, starts))


# ------------------------------------------------------------------------------------- 2. spans longer than a wave
def long_rows():
    """Rows of 150 and 250 generated tokens over the chemistry vocabulary: [(name, token strings without the <eos>)].
    A branch level costs three tokens, `(C` and `)`, so the deepest chain that 250 tokens hold has 83 levels: deeper
    than a wave is wide.  The last row leaves 100 levels open, which the walk pushes before the <eos> finds them."""
    ring = [str(k) if k < 10 else f"%{k}" for k in range(40)]
    rows = [
        ("branch depth 83", ["C"] + ["(", "C"] * 83 + [")"] * 83),
        ("branch depth 49, 150 tokens", ["C"] + ["(", "C"] * 49 + [")"] * 49 + ["C"]),
        ("40 rings open at once", [t for k in range(40) for t in ("C", ring[k])] * 2),
        ("40 rings, ring 35 closes with another order",
         [t for k in range(40) for t in (("C", "=", ring[k]) if k == 35 else ("C", ring[k]))] +
         [t for k in range(40) for t in (("C", "#", ring[k]) if k == 35 else ("C", ring[k]))]),
        ("the offending atom is the last token", ["C"] * 147 + ["=", "F"]),
        ("the first atom is over its valence by the last closure",
         ["C", "1", "(", "C", ")", "(", "C", ")", "(", "C", ")"] + ["C"] * 237 + ["1"]),
        ("an aromatic chain of 249", ["c"] * 249),
        ("100 branches open at the <eos>: the stack at depth 100", ["C"] + ["(", "C"] * 100),
    ]
    return rows


def test_spans_longer_than_a_wave(ops):
    """W = 256, start 4.  The hand-made rows with their known verdicts, and random walks of 150 and 250 tokens through
    the grammar (branches and rings open along the way), all against the reference."""
    ch = CHEMS[len(CHEMV)]
    W, t0 = 256, 4
    made = long_rows()
    assert {len(t) + 1 for _, t in made} == {150, 161, 163, 202, 250, 251}               # (with the <eos>)
    gr, rng = SmilesGrammar(VOCAB70, PAD, EOS), random.Random(9)
    walked = [walk(gr, G, rng, G + 1, 0.01) for G in (149, 249, 149, 249, 249)]      # V70 ids are CHEMV ids
    n = len(made) + len(walked)
    ys = torch.randint(0, len(CHEMV), (n, W), generator=torch.Generator().manual_seed(2))
    ys[:, t0:] = PAD
    for r, (_, toks) in enumerate(made):
        ys[r, t0:t0 + len(toks) + 1] = torch.tensor([CHEMV.index(t) for t in toks] + [EOS])
    for r, ids in enumerate(walked, len(made)):
        ys[r, t0:t0 + len(ids)] = torch.tensor(ids)
    ref = ch.check_reference(ys, [t0] * n)
    want = [(OK, -1, 84, 0), (OK, -1, 51, 0), (OK, -1, 80, 40), (RING_BOND, 153, 80, 40), (VALENCE, 148, 148, 0),
            (VALENCE, 0, 241, 1), (AROMATIC, 0, 249, 0), (SYNTAX, 201, 0, 0)]
    for r, w in enumerate(want):
        assert tuple(int(t[r]) for t in ref) == w, made[r][0]
    assert all(int(s) != SYNTAX for s in ref.status[len(made):])                    # the walks end inside their budgets
    assert max(ch.grammar.state(w[:100])[1] for w in walked) >= 2                   # branches open along the way
    same(launch(ops, ch, ys, [t0] * n), ref)
    same(torch.stack(list(ch.check_rows(ys.cuda(), torch.full((n,), t0))), 1).cpu(), ref)


# ------------------------------------------------------------------------------------------- 3. degenerate rows
def test_degenerate_rows(ops):
    ch = CHEMS[len(CHEMV)]
    V, W = len(CHEMV), 12
    C = CHEMV.index("C")
    ys = torch.full((6, W), PAD)
    starts = [W, 11, 3, 3, 0, 2]
    ys[1, 11] = EOS                                                                 # <eos> alone
    ys[2, 3:6] = torch.tensor([C, -1, EOS])
    ys[3, 3:6] = torch.tensor([C, V, EOS])
    ys[4, 0:3] = torch.tensor([C, C, EOS])                                          # no prefix at all
    ys[5, 2:] = C                                                                   # never ends
    ref = ch.check_reference(ys, starts)
    assert [tuple(int(t[r]) for t in ref) for r in range(6)] == [
        (SYNTAX, 0, 0, 0), (SYNTAX, 0, 0, 0), (SYNTAX, 1, 0, 0), (SYNTAX, 1, 0, 0), (OK, -1, 2, 0), (SYNTAX, 10, 0, 0)]
    same(launch(ops, ch, ys, starts), ref)
    for r in range(6):                                                              # a single row
        same(launch(ops, ch, ys[r:r + 1], starts[r:r + 1]), ChemReportRow(ref, r))
    table, chem = ch.device_tables("cuda")
    out = torch.full((0, 4), SENT, dtype=torch.int32, device="cuda")                # n = 0: a no-op
    ops.smiles_check(torch.zeros(0, W, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                     table, chem, out=out)
    assert ops.smiles_check(torch.zeros(0, W, dtype=torch.int64, device="cuda"),
                            torch.zeros(0, dtype=torch.int32, device="cuda"), table, chem).shape == (0, 4)
    rep = ch.check_rows(ys.cuda()[:, 2:], [W - 2, 9, 1, 1, 0, 0])                   # a view: rows wider than the span
    assert rep.status.dtype == torch.int32 and rep.status.is_cuda
    same(torch.stack(list(rep), 1).cpu(), ch.check_reference(ys[:, 2:], [W - 2, 9, 1, 1, 0, 0]))
    same(torch.stack(list(ch.check_rows(ys.int().cuda(), starts)), 1).cpu(), ref)   # any integer dtype
    with pytest.raises(ValueError):
        ops.smiles_check(ys.cuda(), torch.zeros(5, dtype=torch.int32, device="cuda"), table, chem)


def ChemReportRow(ref, r):
    return type(ref)(*(t[r:r + 1] for t in ref))


# ------------------------------------------------------------------------------------------- 4. the front ends
def tiny_sampler(seed=21, **kw):
    """A PscavaetfSampling over the tiny config (N 2, d_model 64) with the 31-token target vocabulary, dropout 0."""
    from gct_plus_amd.Inference.sampling_tool import PscavaetfSampling
    from gct_plus_amd.Model import model_dict
    nc = synthetic.n_conds("pscavaetf")
    TRG = data.Vocab(VOCAB31)
    SRC = data.Vocab([t for t in VOCAB31 if t not in ("<sos>", "<eos>")])
    torch.manual_seed(seed)
    model = model_dict["pscavaetf"](len(SRC), len(TRG), dropout=0.0, nconds=nc, use_cond2lat=True, **TINY).cuda().eval()
    return PscavaetfSampling(model, SRC, TRG, latent_dim=TINY["latent_dim"], max_strlen=12, cond_dim=nc,
                             decode_algo="multinomial", seed=5, **kw)


def tiny_inputs(seed=31):
    """12 rows with mixed scaffold prefixes of 3 / 6 / 2 / 5 tokens."""
    g = torch.Generator().manual_seed(seed)
    nc = synthetic.n_conds("pscavaetf")
    ys0, lens = mixed_prefixes([3, 6, 2, 5], 3, g)
    n, Le = ys0.shape[0], 20 + nc
    z = torch.randn(n, Le, TINY["latent_dim"], generator=g)
    klen = torch.randint(8, Le + 1, (n,), generator=g)
    src_mask = (torch.arange(Le)[None, :] < klen[:, None]).unsqueeze(1)
    return z, ys0, src_mask, torch.randn(n, nc, generator=g), lens


def test_sampler_check_rows_constrained_and_free():
    z, ys0, src_mask, dconds, lens = tiny_inputs()
    reports = {}
    for well_formed in (True, False):
        sp = tiny_sampler(well_formed=well_formed)
        _, rows = sp.decode(z, ys0, src_mask, dconds, prefix_lens=lens, return_rows=True)
        rep = sp.check_rows(rows)
        assert all(t.is_cuda and t.dtype == torch.int32 and t.shape == (12,) for t in rep)
        ref = sp.chemistry.check_reference(rows.ys.cpu(), rows.prefix_lens)
        same(torch.stack(list(rep), 1).cpu(), ref)
        same(torch.stack(list(sp.check_rows(rows.ys, rows.prefix_lens)), 1).cpu(), ref)
        same(torch.stack(list(sp.check_rows((rows.ys, rows.prefix_lens))), 1).cpu(), ref)
        reports[well_formed] = ref
        for r in range(12):                                                         # is_valid: the same verdict per string
            smi = sp.id_to_smi(rows.ys[r, int(lens[r]):].tolist())
            if int(ref.status[r]) != SYNTAX:
                assert sp.is_valid(smi) == (int(ref.status[r]) == OK), smi
        assert sp.chemistry is sp.chemistry
    print("constrained:", reports[True].status.tolist(), " free:", reports[False].status.tolist())
    assert SYNTAX not in reports[True].status.tolist()
    assert SYNTAX in reports[False].status.tolist()
    sp = tiny_sampler()
    assert sp.is_valid("CC(=O)O") and sp.is_valid("c1ccccc1", scaffold="CC") and not sp.is_valid("C1C1")
    assert not sp.is_valid("C(C)(C)(C)(C)C") and not sp.is_valid("CC(") and not sp.is_valid("")


@pytest.mark.parametrize("shaped", [False, True])
def test_validity_reward_on_the_device_is_the_host_reward(shaped):
    """reinforce_step with validity_reward of the device report against the same step on an equal model with the reward
    worked out from the host `check` and copied over: the same loss and the same parameter bits.  Five of the twelve
    decoded rows are overwritten with valid molecules, so that the rewards differ and the step moves the weights."""
    from gct_plus_amd.optim import FusedAdam
    from gct_plus_amd.Train.finetune import reinforce_step, validity_reward
    z, ys0, src_mask, dconds, lens = tiny_inputs()
    final, losses = [], []
    for host in (False, True):
        sp = tiny_sampler(well_formed=True)
        start = {k: p.detach().clone() for k, p in sp.model.named_parameters()}
        _, rows = sp.decode(z, ys0, src_mask, dconds, prefix_lens=lens, return_rows=True)
        ys = rows.ys.clone()
        for r, s in enumerate(("CCO", "C1CC1", "CC(=O)O", "c1ccccc1", "N#N")):
            ids, t0 = ids_of(s, VOCAB31) + [EOS], int(rows.prefix_lens[r])
            assert t0 + len(ids) <= ys.shape[1]
            ys[r, t0:] = PAD
            ys[r, t0:t0 + len(ids)] = torch.tensor(ids, device=ys.device)
        rows = rows._replace(ys=ys)
        span = rows.ys.shape[1] - rows.prefix_lens
        if host:
            got = [sp.chemistry.check(r[t0:]) for r, t0 in zip(rows.ys.cpu().tolist(), rows.prefix_lens.tolist())]
            reward = torch.tensor([1.0 if s == OK else (p / float(w) if shaped else 0.0)
                                   for (s, p, _, _), w in zip(got, span.tolist())], dtype=torch.float64).float()
        else:
            reward = validity_reward(sp.check_rows(rows), shaped=shaped, lengths=span if shaped else None)
            assert reward.is_cuda and reward.dtype == torch.float32 and reward.shape == (12,)
        opt = FusedAdam(sp.model.parameters(), lr=1e-3, betas=(0.9, 0.98), eps=1e-9, model=sp.model)
        losses.append(reinforce_step(sp, opt, rows, reward)["loss"])
        final.append({k: p.detach().clone() for k, p in sp.model.named_parameters()})
        assert 5 <= int((reward == 1).sum()) < 12
        assert any(not torch.equal(final[-1][k], start[k]) for k in start)          # the step did move the weights
    assert losses[0] == losses[1]
    for k in final[0]:
        assert torch.equal(final[0][k], final[1][k]), k
