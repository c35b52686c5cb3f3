"""Host: arena.SlotArenas, the grow-only per-slot buffer protocol of every encoder and head, on plain Python objects (no device, no library)."""
import pytest

from interspeech_ser_amd.arena import SlotArenas


def _arenas():
    built = []

    def build(cap):
        built.append(dict(cap))
        return dict(rows=[0] * cap["M"], offs=[0] * (cap["B"] + 1))
    return SlotArenas(build), built


def test_a_fitting_request_returns_the_identical_dict_without_building():
    ar, built = _arenas()
    first = ar.fit(0, M=10, B=3)
    assert built == [dict(M=10, B=3)] and first["cap"] == dict(M=10, B=3) and first["plan"] is None and len(first["rows"]) == 10
    first["plan"], first["tape"] = "laid out", "recorded"
    for need in (dict(M=10, B=3), dict(M=1, B=1), dict(M=10, B=1)):
        assert ar.fit(0, **need) is first
    assert len(built) == 1 and first["plan"] == "laid out" and first["tape"] == "recorded"
    assert ar[0] is first and ar.get(0) is first


def test_growth_takes_the_per_key_maximum_and_drops_tape_plan_and_memos():
    ar, built = _arenas()
    old = ar.fit(0, M=10, B=3)
    old["plan"], old["tape"], old["table_T"] = "laid out", "recorded", 7
    new = ar.fit(0, M=4, B=5)                                 # only B exceeds: M keeps its capacity
    assert new is not old and built[-1] == dict(M=10, B=5) and new["cap"] == dict(M=10, B=5)
    assert new["plan"] is None and "tape" not in new and "table_T" not in new
    assert len(new["rows"]) == 10 and len(new["offs"]) == 6
    assert ar[0] is new and ar.fit(0, M=10, B=5) is new and ar.fit(0, M=10, B=3) is new      # no capacity ever shrinks
    assert old["tape"] == "recorded"                          # the old dict is left alone, only forgotten
    assert ar.fit(0, M=11, B=1)["cap"] == dict(M=11, B=5) and len(built) == 3


def test_slots_are_independent():
    ar, built = _arenas()
    a, b = ar.fit(0, M=10, B=3), ar.fit(1, M=2, B=1)
    assert a is not b and b["cap"] == dict(M=2, B=1)
    a["tape"] = "recorded"
    assert ar.fit(1, M=20, B=1)["cap"] == dict(M=20, B=1) and ar[0] is a and a["tape"] == "recorded" and a["cap"] == dict(M=10, B=3)
    assert ar.get(2) is None and ar.get(2, "none") == "none"
    with pytest.raises(KeyError):
        ar[2]


def test_a_key_met_for_the_first_time_counts_as_capacity_zero():
    made = []
    ar = SlotArenas(lambda cap: made.append(dict(cap)) or {})
    first = ar.fit(0, B=2)
    grown = ar.fit(0, B=1, work=0)                            # a need of nothing fits a capacity of nothing
    assert grown is first and len(made) == 1
    grown = ar.fit(0, B=1, work=6)
    assert grown is not first and grown["cap"] == dict(B=2, work=6) and made[-1] == dict(B=2, work=6)


# ---------------------------------------------------------------------------------------------------------- the table blob's layout
@pytest.mark.parametrize("cap_b", [1, 2, 17])
def test_table_layout_regions_are_disjoint_aligned_and_independent_of_the_batch(cap_b):
    from interspeech_ser_amd.arena import TableLayout
    lay = TableLayout(cap_b, 5)
    assert lay.region == cap_b + 2 and lay.words == 5 * (cap_b + 2)
    spans = []
    for r in range(5):
        w = lay.offset(r, cap_b + 1)                          # a 64-bit table of B + 1 entries fits ...
        e = lay.offset(r, 2 * cap_b + 2, 2)                   # ... and so does a 32-bit table of 2 B + 2 entries
        assert e == 2 * w                                     # an int32 table starts on its region's first word: 8-byte aligned
        spans.append((w, w + max(cap_b + 1, (2 * cap_b + 2 + 1) // 2)))
        for b in range(1, cap_b + 1):                         # the batch's own B moves nothing
            assert lay.offset(r, b + 1) == w and lay.offset(r, b, 2) == e and lay.offset(r, 0) == w
    assert spans[0][0] == 0 and spans[-1][1] <= lay.words
    assert all(a[1] <= b[0] for a, b in zip(spans[:-1], spans[1:]))          # no region reaches into the next
    assert lay.offset(0, cap_b + 2) == 0 and lay.offset(0, 2 * cap_b + 4, 2) == 0
    for bad in ((0, cap_b + 3, 1), (0, 2 * cap_b + 5, 2), (5, 1, 1), (-1, 1, 1)):
        with pytest.raises(ValueError):
            lay.offset(*bad)
