"""The host reference of the row maps (tests/rowmap_ref.py) against the contract the kernels are held to, and the
conditions on the random plans the device tests use.  No GPU."""
import itertools

import torch

from tests.rowmap_ref import compact_rows, gap_rows, prefix_live, random_plans, row_plan_reference


def _every_prefix_plan():
    for T in range(5, 10):
        for B in range(2, 5):
            for n in itertools.product(range(T + 1), repeat=B):
                yield B, T, n


def test_reference_meets_the_contract_on_every_small_prefix_plan():
    """T = 5..9, B = 2..4, every tuple of prefix lengths (27 469 plans, empty samples included): compact row
    cstart[b]+t is original row b*T+t for t < n_b; cstart never decreases; gap rows and live-prefix rows are disjoint
    and together cover [0, Mc).  With the offset of row 0 inside its quad also applied to samples whose first quad is
    dead (cstart as it was first defined) 891 of these plans put a live row into another sample's gap."""
    plans = old_overlaps = 0
    for B, T, n in _every_prefix_plan():
        plans += 1
        p = row_plan_reference(prefix_live(B, T, n))
        orig, prefix = (x.tolist() for x in compact_rows(p))
        cs, nb, Mc = p["cstart"].tolist(), p["n_b"].tolist(), p["Mc"]
        assert nb == list(n)
        for b in range(B):
            assert 0 <= cs[b] and cs[b] + nb[b] <= Mc, (B, T, n)
            assert orig[cs[b]:cs[b] + nb[b]] == list(range(b * T, b * T + nb[b])), (B, T, n)
        assert all(cs[b] <= cs[b + 1] for b in range(B - 1)), (B, T, n, cs)

        def walk(start):       # the rows gct_zero_gap_rows visits: [start[b] + n_b, start[b+1]) and the tail up to Mc
            w = set()
            for b in range(B):
                w.update(range(start[b] + nb[b], start[b + 1] if b + 1 < B else Mc))
            return w

        live_rows = {r for r in range(Mc) if prefix[r]}
        walked = walk(cs)
        assert not (walked & live_rows), (B, T, n, cs)                          # disjoint
        assert walked | live_rows == set(range(Mc)), (B, T, n, cs)              # together they cover [0, Mc)
        assert len(live_rows) == sum(nb) == p["info"][0]
        # the earlier definition, for the record: the offset of row 0 inside its quad for every sample
        flat = [x for r in p["live"].tolist() for x in r]
        rank, seen = [], 0
        for q in range((B * T + 3) // 4):
            rank.append(seen)
            seen += int(any(flat[4 * q:4 * q + 4]))
        old = [4 * rank[(b * T) >> 2] + ((b * T) & 3) for b in range(B)]
        old_live = {old[b] + t for b in range(B) for t in range(nb[b])}
        old_overlaps += int(bool(walk(old) & old_live))
    assert plans == 27469 + 15          # the 15 (B, T) pairs' all-dead plan included
    assert old_overlaps == 891
    p = row_plan_reference(prefix_live(2, 7, (3, 7)))
    assert torch.equal(gap_rows(p, p["Mc"] + 5)[:p["Mc"]], ~compact_rows(p)[1]) and gap_rows(p, p["Mc"] + 5)[p["Mc"]:].all()


def test_the_issue_example():
    p = row_plan_reference(prefix_live(3, 6, (0, 0, 2)))
    assert p["cstart"].tolist() == [0, 0, 0] and p["Mc"] == 128 and p["info"][5] == 1
    orig, prefix = compact_rows(p)
    assert orig[:4].tolist() == [12, 13, 14, 15] and prefix[:4].tolist() == [True, True, False, False]


def test_reference_counters_on_known_plans():
    T = 6
    live = torch.tensor([[1, 1, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=torch.bool)
    p = row_plan_reference(live, None)
    assert p["info"][:3] == [4, 2, 1] and p["tile_list"].tolist() == [0]
    seen = torch.zeros(3, T, T, dtype=torch.uint8)
    seen[:, :, 0] = 1                                # every query sees key 0 only
    p = row_plan_reference(live, seen)
    assert p["info"][1] == 1                         # sample 1: key 0 is dead and visible to its live rows
    seen[0, 1, :] = 0                                # sample 0: live row 1 sees no key, dead rows exist
    assert row_plan_reference(live, seen)["info"][1] == 2
    k = row_plan_reference(torch.tensor([[1, 1, 0], [0, 0, 0], [1, 0, 1]]), key_side=True)
    assert k["info"] == [4, 0, 1, 0, 128, 3, 1, 0] and k["tile_list"] is None
    # flat rows 0, 1, 6, 8 are live: all three quads of the 9 rows, and every sample starts inside a live quad
    assert k["quad_list"][:4].tolist() == [0, 1, 2, -1] and k["cstart"].tolist() == [0, 3, 6]


def test_random_plans_cover_what_the_device_tests_need():
    """Conditions on the generator (fixed seed, 60 plans), not measurements."""
    plans = random_plans()
    assert len(plans) == 60
    assert [n for n, *_ in plans] == [n for n, *_ in random_plans()]          # deterministic
    usable = empty = full = viol = nonpre = 0
    for _, live, mask in plans:
        p = row_plan_reference(live, mask)
        usable += int(p["info"][1] == 0 and p["info"][2] == 0)
        empty += int(bool((p["n_b"] == 0).any()))
        full += int(bool((p["n_b"] == p["T"]).any()))
        viol += int(p["info"][1] != 0)
        nonpre += int(p["info"][2] != 0)
    assert usable >= 30 and empty >= 10 and full >= 10 and viol >= 5 and nonpre >= 5, (usable, empty, full, viol, nonpre)
