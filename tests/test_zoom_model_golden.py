"""CPU-only: tests/zoom_model.py -- the reference's walk over a zoom level, deque included -- equals every array the reference's
``summarize`` and every value its ``query`` gave for the cases of tests/golden/zoom (recorded by tools/record_zoom_golden.py), bit
for bit, NaN equal to NaN; the rule that picks the level gives the recorded choices; the reader returns what the walk needs."""
import os
import struct

import numpy as np
import pytest

import summary_model as S
import zoom_model as M
from zoom_cases import FILES, GOLDEN, INT32_MAX, MANIFEST, levels, path_of, recorded, spans, zoom_cases


@pytest.mark.parametrize("name", sorted(FILES))
def test_model_gives_the_recorded_arrays_and_queries(name):
    entry = FILES[name]
    assert zoom_cases(name), name
    for k, case in enumerate(entry["cases"]):
        _, planes, query = recorded(name, k)
        args = (case["start"], case["end"], case["size"])
        if case["none"]:
            assert case["level"] is None
            continue
        assert M.pick_level(entry["reductions"], *args) == case["level"], case
        if case["level"] is None:
            got = S.summarize_region(spans(name)[case["chrom"]], *args)
        else:
            got = M.summarize_region(levels(name)[case["level"]][1][case["chrom"]], *args)
        for p, g, w in zip(M.PLANES, got, planes):
            assert M.same_bits(g, w), (name, case, p)
        for key, g, w in zip(M.QUERY_KEYS, M.query_region(got, *args), query):
            assert M.same_bits(g, w), (name, case, key)


def test_the_recorded_cases_see_the_mistakes_that_matter():
    """what the recorder asserted about its own cases; the reading of the accumulating lines is the one the built reference showed"""
    seen = MANIFEST["seen"]
    assert MANIFEST["reading"] == M.READING == "b"
    assert seen["other_reading"] >= 64 and seen["reversed"] >= 64 and seen["front_only"] >= 16 and seen["all_nan"] >= 16
    # and the other reading does fail here: one recorded region that it misses
    name = "leaves.bw"
    k = next(k for k in zoom_cases(name) if FILES[name]["cases"][k]["size"] == 200)
    case, planes, _ = recorded(name, k)
    other = M.summarize_region(levels(name)[case["level"]][1][case["chrom"]], case["start"], case["end"], case["size"], reading="a")
    assert not all(M.same_bits(g, w) for g, w in zip(other, planes))


def test_sizes_and_edges_are_among_the_recorded_cases():
    sizes = {FILES[n]["cases"][k]["size"] for n in FILES for k in zoom_cases(n)}
    assert {1, 2, 64, 65, 200} <= sizes
    for name, reductions in (("test.bw", [20, 80, 320, 1280, 5120, 20480]), ("odd.bw", [40, 10, 10])):
        assert FILES[name]["reductions"] == reductions
    # the duplicated reduction: the first in file order is the one chosen, never the second
    picked = {FILES["odd.bw"]["cases"][k]["level"] for k in zoom_cases("odd.bw")}
    assert picked == {0, 1}
    assert {FILES["test.bw"]["cases"][k]["level"] for k in zoom_cases("test.bw")} >= {0, 1, 2, 5}


def test_pick_level():
    from bxmi import summary

    for pick in (M.pick_level, summary.pick_level):
        assert pick([20, 80], 0, 100, 10) is None and pick([20, 80], 0, 30, 10) is None  # desired 5; desired 1
        assert pick([20, 80], 0, 400, 10) == 0 and pick([20, 80], 0, 1600, 10) == 1 and pick([20, 80], 0, 1599, 10) == 0
        assert pick([80, 20], 0, 1600, 10) == 0 and pick([80, 20], 0, 400, 10) == 1  # an unsorted list
        assert pick([10, 10, 40], 0, 300, 10) == 0  # equal reductions: the first in file order
        assert pick([], 0, 10 ** 6, 1) is None and pick([2], 0, 4, 1) == 0
    for name, entry in FILES.items():
        for case in entry["cases"]:
            if not case["none"]:
                assert summary.pick_level(entry["reductions"], case["start"], case["end"], case["size"]) == case["level"], (name, case)


def test_reader_on_the_references_file():
    got = levels("test.bw")
    assert [r for r, _ in got] == [20, 80, 320, 1280, 5120, 20480]
    assert [len(m["chr1"].start) for _, m in got] == [500, 125, 32, 8, 2, 1]
    for _, m in got:
        z = m["chr1"]
        assert list(m) == ["chr1"] and len(z.leaf_lo) == len(z.leaf_hi) == 1 and list(z.leaf_first) == [0, len(z.start)]
        assert [a.dtype for a in z] == [np.int32, np.int32, np.uint32] + [np.float32] * 4 + [np.int32, np.int32, np.int64]
        assert z.leaf_lo[0] == z.start[0] == 10917 and z.leaf_hi[0] == z.end[-1]


def test_reader_on_the_written_files():
    from bxmi import bigwig

    for name in ("leaves.bw", "chroms.bw", "odd.bw"):
        with open(path_of(name), "rb") as f:
            data = f.read()
        for (_, a), (_, b) in zip(levels(name), bigwig.read_zoom_file(data=data)):
            assert all(np.array_equal(x, y, equal_nan=True) for c in a for x, y in zip(a[c], b[c]))
        for _, per in levels(name):
            for z in per.values():
                assert bigwig.ordered_level(z) is None
                assert z.leaf_first[0] == 0 and z.leaf_first[-1] == len(z.start) and np.all(np.diff(z.leaf_first) > 0)
    fine = levels("leaves.bw")[0][1]["chrL"]
    assert len(fine.start) == 301 and len(fine.leaf_lo) == 43 and np.all(np.diff(fine.leaf_first) <= 7)
    assert np.max(fine.start[1:] - fine.end[:-1]) > 7 * 16  # a gap wider than a leaf
    # blocks and leaf entries that cross chromosomes: the entry is clamped to the chromosome it is read for
    per = levels("chroms.bw")[0][1]
    assert list(per) == ["chrA", "chrB", "chrC"] and [len(z.start) for z in per.values()] == [23, 17, 26]
    assert per["chrA"].leaf_hi[-1] == INT32_MAX and per["chrB"].leaf_lo[0] == -1 and per["chrB"].leaf_hi[-1] == INT32_MAX and per["chrC"].leaf_lo[0] == -1
    assert per["chrA"].leaf_lo[0] == 0 and per["chrC"].leaf_hi[-1] == per["chrC"].end[-1]
    odd = levels("odd.bw")[1][1]["chrO"]
    assert odd.valid.max() > 2 ** 24 and np.isnan(odd.min).any() and np.isnan(odd.max).any()
    (_, per), = bigwig.read_zoom_file(os.path.join(GOLDEN, "unordered.z.bw"))
    assert "record starts" in bigwig.ordered_level(per["chrU"])


def test_reader_refuses_what_the_leaf_test_cannot_answer():
    from bxmi import bigwig

    with open(path_of("leaves.bw"), "rb") as f:
        data = bytearray(f.read())
    index = struct.unpack_from("<Q", data, 64 + 16)[0]
    is_leaf, _, count = struct.unpack_from("<BBH", data, index + 48)
    assert not is_leaf and count > 1  # the root of a tree of several levels
    struct.pack_into("<I", data, index + 48 + 4 + 12, 0)  # its first entry now ends at base 0: the children reach beyond it
    with pytest.raises(ValueError, match="not contained in its parent"):
        bigwig.read_zoom_file(data=bytes(data))
    with open(path_of("chroms.bw"), "rb") as f:
        data = bytearray(f.read())
    index = struct.unpack_from(">Q", data, 64 + 16)[0]
    node = struct.unpack_from(">Q", data, index + 48 + 4 + 16)[0]
    while not struct.unpack_from(">B", data, node)[0]:
        node = struct.unpack_from(">Q", data, node + 4 + 16)[0]
    block = struct.unpack_from(">Q", data, node + 4 + 16)[0]  # the first leaf entry's block, not compressed: records of 32 bytes
    struct.pack_into(">I", data, block + 8, 2 ** 31)  # the first record's end
    with pytest.raises(ValueError, match="beyond 2\\^31 - 1"):
        bigwig.read_zoom_file(data=bytes(data))
    with pytest.raises(ValueError):
        bigwig.read_zoom_file(data=b"not a bigWig file at all" * 4)
