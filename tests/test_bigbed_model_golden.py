"""CPU-only: tests/summary_model.py over a bigBed file's records as items of value 1 equals every array the reference's
``BigBedFile.summarize_from_full`` gave for the cases of tests/golden/bigbed (recorded by tools/record_bigbed_golden.py), bit for
bit; the regions the reference took from a zoom level equal tests/zoom_model.py over that level; ``query`` is the model's
derivation of either; the None answers and the choice of the level are the recorded ones; the straddle case sees a wrong order."""
import numpy as np
import pytest

import summary_model as S
import zoom_model as Z
from bed_cases import FILES, MANIFEST, SIZES, items, path_of, recorded, with_ones


@pytest.mark.parametrize("name", sorted(FILES))
def test_model_gives_the_recorded_arrays_and_queries(name):
    from bxmi import bigbed

    entry = FILES[name]
    levels = bigbed.read_zoom_file(path_of(name))
    assert [r for r, _ in levels] == entry["reductions"]
    for k, case in enumerate(entry["cases"]):
        _, full, picked, query = recorded(name, k)
        args = (case["start"], case["end"], case["size"])
        track = items(name).get(case["chrom"])
        if case["none"]:
            assert track is None or S.summarize_region(with_ones(track), *args) is None, case
            continue
        assert Z.pick_level(entry["reductions"], *args) == case["level"], case
        got = S.summarize_region(with_ones(track), *args)
        for p, g, w in zip(S.PLANES, got, full):
            assert S.same_bits(g, w), (name, case, p)
        if case["level"] is not None:
            got = Z.summarize_region(levels[case["level"]][1][case["chrom"]], *args)
        for p, g, w in zip(S.PLANES, got, picked):
            assert S.same_bits(g, w), (name, case, p, "summarize")
        for key, g, w in zip(S.QUERY_KEYS, S.query_region(got, *args), query):
            assert S.same_bits(g, w), (name, case, key)
        assert case["query_types"] == ["coverage:float64", "max:float64", "mean:float64", "min:float64", "std_dev:float"]


def test_every_plane_is_the_chain_of_weights():
    """with a value of 1 the five chains are one: sum = sumsq, valid = its rounding, min = max = 1 exactly where it is positive"""
    for name in FILES:
        for k, case in enumerate(FILES[name]["cases"]):
            if case["none"]:
                continue
            valid, mn, mx, sm, sq = recorded(name, k)[1]
            assert S.same_bits(sm, sq) and S.same_bits(valid, np.rint(sm)), (name, case)
            assert np.array_equal(mn == 1.0, sm > 0) and np.array_equal(mx == 1.0, sm > 0), (name, case)
            assert np.all(np.isposinf(mn[sm == 0])) and np.all(np.isneginf(mx[sm == 0]))


def test_the_recorded_cases_see_a_wrong_order():
    """what the recorder asserted, and that it does fail here: the reversed chain misses the recorded straddle region"""
    seen = MANIFEST["straddle"]
    assert seen["bins_changed_when_reversed"] >= 32
    name, (chrom, start, end, size) = seen["file"], seen["region"]
    k = next(k for k, c in enumerate(FILES[name]["cases"]) if (c["start"], c["end"], c["size"]) == (start, end, size))
    want = recorded(name, k)[1]
    track = with_ones(items(name)[chrom])
    assert np.count_nonzero(np.diff(track[1].astype(np.int64)) < 0) > 100  # the ends do descend
    other = S.summarize_region(track, start, end, size, reverse=True)
    assert sum(1 for j in range(size) if other[3][j] != want[3][j]) == seen["bins_changed_when_reversed"]
    depth = [int(((track[0] < start + 40 * (j + 1)) & (track[1] > start + 40 * j)).sum()) for j in range(size)]
    assert size >= 1000 and max(depth) <= 8 and sum(d >= 4 for d in depth) >= size - 4


def test_sizes_and_edges_are_among_the_recorded_cases():
    cases = [c for n in FILES for c in FILES[n]["cases"]]
    assert set(SIZES) <= {c["size"] for c in cases}
    assert sum(c["none"] for c in cases) >= 4 and {c["level"] for c in FILES["zoom.bb"]["cases"]} == {None, 0, 1}
    assert all(e["str_chrom"] == {"summarize_from_full": "TypeError", "get": "TypeError"} for e in FILES.values())
    # the hand-written case: five records and one of another chromosome in the same block, which is not counted
    valid = recorded("hand.bb", 0)[1][0]
    assert FILES["hand.bb"]["cases"][0]["start"] == 3 and valid.tolist() == [37.0, 35.0, 24.0, 15.0]
    # the first record of long.bb spans its chromosome; zero-length records exist
    s, e, _ = items("long.bb")["chrL"]
    assert (s[0], e[0]) == (0, FILES["long.bb"]["chroms"]["chrL"]) and len(s) > 1000
    assert any(np.any(t[0] == t[1]) for t in items("genes.bb").values())
