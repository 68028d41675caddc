"""decode.StepPlan on the host: the graph-key table for every valid step unit, what construction refuses, and the row
view KVDecoder._rows hands the step's kernels for each layout.  No GPU, no library."""
import itertools

import pytest
import torch

from gct_plus_amd.decode import BEAM, FILTERED, GRAMMAR, LOGP, MIXED, STREAM, UNIFORM, KVDecoder, StepPlan

SELECTS, LAYOUTS = (0, 1, FILTERED), (UNIFORM, MIXED, STREAM)


def test_names_are_the_ones_the_keys_are_read_by():
    assert (BEAM, FILTERED, UNIFORM, MIXED, STREAM, GRAMMAR, LOGP) == (
        "beam", "filtered", "uniform", "mixed", "stream", "grammar", "logp")


@pytest.mark.parametrize("m", SELECTS)
def test_key_table(m):
    """The table of the graph keys, row by row, for every layout L."""
    assert StepPlan(m).key == StepPlan(m, UNIFORM, False, False).key == m
    assert StepPlan(m, MIXED).key == (m, "mixed")
    assert StepPlan(m, STREAM).key == (m, "stream")
    assert StepPlan(m, UNIFORM, grammar=True).key == (m, "uniform", "grammar")
    for L in LAYOUTS:
        assert StepPlan(m, L, grammar=True).key == (m, L, "grammar")
        assert StepPlan(m, L, logp=True).key == (m, L, "logp")
        assert StepPlan(m, L, grammar=True, logp=True).key == (m, L, "grammar", "logp")


def test_keys_are_distinct_and_readable():
    plans = [StepPlan(m, L, g, lp) for m, L, g, lp in itertools.product(SELECTS, LAYOUTS, (False, True), (False, True))]
    plans.append(StepPlan(BEAM))
    assert StepPlan(BEAM).key == "beam"
    keys = [p.key for p in plans]
    assert len(set(keys)) == len(plans) == 37                        # 3 selects x 3 layouts x grammar x logp, and beam
    for p, k in zip(plans, keys):
        assert (isinstance(k, tuple) and k[-1] == LOGP) == p.logp     # what test_score_gpu reads
        assert (isinstance(k, tuple) and k[1] == STREAM) == (p.layout == STREAM)      # what _drop_stream_graphs reads
        assert (isinstance(k, tuple) and GRAMMAR in k) == p.grammar
        assert p.key is p.key and hash(p) == hash(StepPlan(p.select, p.layout, p.grammar, p.logp))


def test_a_plan_is_a_value():
    assert StepPlan() == StepPlan(0, UNIFORM, False, False)          # step() without an argument: uniform greedy
    with pytest.raises(AttributeError):
        StepPlan().layout = MIXED


@pytest.mark.parametrize("kw", [dict(layout=MIXED), dict(layout=STREAM), dict(grammar=True), dict(logp=True)])
def test_beam_takes_none_of_the_others(kw):
    with pytest.raises(ValueError, match="beam"):
        StepPlan(BEAM, **kw)


def test_unknown_select_and_layout():
    for bad in (dict(select=2), dict(select="greedy"), dict(layout="ragged")):
        with pytest.raises(ValueError):
            StepPlan(**bad)


def test_row_view():
    """CPU stand-ins for the decoder's buffers: uniform rows get no row_off / item / prefix_len, mixed rows row_off only,
    streamed rows all three; the grammar mask's view adds gram and, streamed, the items' limit."""
    from tests.test_grammar_host import EOS, PAD, SOS, VOCAB31, tiny_model
    kd = KVDecoder(tiny_model(VOCAB31), PAD, SOS, EOS)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)                # noqa: E731
    kd.row_off, kd.gram = i32(4), i32(2)
    kd.stream = dict(item=i32(4), prefix_len=i32(6), limit=i32(6), item_base=0)
    assert kd._rows(StepPlan()) == dict(row_off=None, item=None, prefix_len=None)
    for m in SELECTS:
        v = kd._rows(StepPlan(m, MIXED))
        assert v["row_off"] is kd.row_off and v["item"] is None and v["prefix_len"] is None and len(v) == 3
        v = kd._rows(StepPlan(m, STREAM, logp=True))
        assert v["row_off"] is kd.row_off and v["item"] is kd.stream["item"]
        assert v["prefix_len"] is kd.stream["prefix_len"] and len(v) == 3
    assert kd._rows(StepPlan(BEAM)) == dict(row_off=None, item=None, prefix_len=None)
    v = kd._rows(StepPlan(0, UNIFORM, grammar=True), mask=True)
    assert v["gram"] is kd.gram and v["limit"] is None and v["row_off"] is None and len(v) == 5
    v = kd._rows(StepPlan(1, MIXED, grammar=True), mask=True)
    assert v["gram"] is kd.gram and v["limit"] is None and v["row_off"] is kd.row_off and v["item"] is None
    v = kd._rows(StepPlan(1, STREAM, grammar=True), mask=True)
    assert v["limit"] is kd.stream["limit"] and v["item"] is kd.stream["item"] and v["gram"] is kd.gram
    # a pool left over from an earlier call is not seen by a plan that does not stream
    assert kd._rows(StepPlan(0, MIXED, grammar=True), mask=True)["limit"] is None
