"""CPU-only: the oracle search of test_tail_block_lane.py (tests/_tail_block.py).  Every event the GPU test names must be
found in the family it is named for within the seeds the GPU test uses, so that a change to a generator cannot silently
empty the GPU test; and the located rounds must be block rounds of the kind they are named for."""
import pytest

import _tail_block as tb


@pytest.mark.parametrize("family", list(tb.REQUIRED), ids=lambda f: "%d-%s-%s" % f[:3])
def test_every_event_is_found(family):
    found, missing = tb.locate(family, tb.REQUIRED[family])
    assert not missing, missing
    assert all(1 <= sd <= 8 and rr for sd, rr in found.values())


def test_shapes_are_what_they_say():
    n, kind, prob, opts = tb.TIE200
    found, missing = tb.locate(tb.TIE200, tb.SHAPES)
    assert not missing
    for name, (seed, rounds) in found.items():
        loc, val, ev, total = tb.trace((n, seed, kind, prob, opts))
        assert set(rounds) <= set(ev["block"]) and rounds[0] <= total
    _, _, ev, _ = tb.trace((400, 1, "tie", "max", tb.TIE400[3]))
    assert set(ev["K>160"]) <= set(ev["block"]) and not set(ev["K>160"]) & set(ev.get("K=17", []))


def test_clean_rounds_in_the_named_seeds():
    n, kind, prob, opts = tb.INTS200
    for seed in tb.CLEAN_SEEDS:
        ev = tb.trace((n, seed, kind, prob, opts))[2]
        assert ev.get("clean"), seed
        assert not set(ev["clean"]) & (set(ev.get("chain end", [])) | set(ev.get("contested, equal bids", [])))


def test_single_edge_family_starts_in_a_block_round():
    found, missing = tb.locate(tb.SINGLE40, tb.REQUIRED[tb.SINGLE40])
    assert not missing and found["single edge"][1][0] == 1
    n, kind, prob, opts = tb.SINGLE40
    loc = tb.trace((n, found["single edge"][0], kind, prob, opts))[0]
    assert sum((loc[:, 0] == i).sum() == 1 for i in range(n)) == 2


def test_long_rows_family_has_block_rounds():
    loc, val, ev, total = tb.trace(tb.LONG)
    assert int(loc[:, 0].max()) >= 96 and len(ev["block"]) >= 8
    assert sum((loc[:, 0] == i).sum() == 40 for i in range(96)) == 36


def test_without_lines_and_batch_events():
    found, missing = tb.locate(tb.INTS200, tb.NO_LINES)
    assert not missing, missing
    for key, cap in zip(tb.BATCH_KEYS, tb.BATCH_CAPS):
        assert cap is None or tb.trace(key)[2].get(cap), (key, cap)
    assert len(set(k[0] for k in tb.BATCH_KEYS)) == 1
