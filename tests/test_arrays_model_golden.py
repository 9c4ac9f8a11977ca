"""CPU-only: tests/arrays_model.py reproduces every ``get_as_array`` result recorded from the reference, byte for byte (a NaN with
its bits): the regions of tests/golden/arrays (written by tools/record_arrays_golden.py: tracks that are not ordered, items whose
value is NaN, regions past the data and past the chromosome's end, ``None`` where the reference answers ``None``) and the regions
of the seven bigWig files of tests/golden/profile (tools/record_profile_golden.py).  The tracks come from the project's bigWig
reader, which tests/test_bigwig_reader.py pins separately."""
import json
import os
import sys

import numpy as np
import pytest

import arrays_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "arrays")
PROFILE = os.path.join(HERE, "golden", "profile")
BX = os.path.join(os.path.dirname(HERE), "bx-python_amd")
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    FILES = {os.path.basename(f["file"]): f for f in json.load(_f)["files"]}
with open(os.path.join(PROFILE, "manifest.json")) as _f:
    PROFILE_MANIFEST = json.load(_f)
PROFILE_FILES = {f["file"]: f for f in PROFILE_MANIFEST["files"]}
_loaded = {}


def path_of(name):
    """a file of either set by its name"""
    return os.path.normpath(os.path.join(GOLDEN, FILES[name]["file"])) if name in FILES else os.path.join(PROFILE, name)


def spans(name):
    """{chrom: (starts, ends, values)} of a golden bigWig file, read once"""
    if name not in _loaded:
        if BX not in sys.path:
            sys.path.insert(0, BX)
        from bxmi import bigwig

        _loaded[name] = bigwig.read_spans_file(path_of(name))
    return _loaded[name]


def recorded(name):
    """[((chrom, start, end), float32 array or None)] of a file of tests/golden/arrays"""
    entry = FILES[name]
    flat = np.load(os.path.join(GOLDEN, entry["arrays"]))
    assert flat.dtype == np.float32
    return [((c["chrom"], c["start"], c["end"]), None if c["none"] else flat[c["at"]:c["at"] + c["end"] - c["start"]]) for c in entry["cases"]]


def recorded_profile_regions(name):
    """[((chrom, start, end), float32 array)] of a file of tests/golden/profile"""
    entry = PROFILE_FILES[name]
    flat = np.load(os.path.join(PROFILE, entry["arrays"]))
    out, at = [], 0
    for chrom, s, e in entry["regions"]:
        out.append(((chrom, s, e), flat[at:at + e - s]))
        at += e - s
    assert at == len(flat) and flat.dtype == np.float32
    return out


def all_recorded(name):
    return recorded(name) if name in FILES else recorded_profile_regions(name)


ALL_FILES = sorted(FILES) + sorted(PROFILE_FILES)


def model_region(name, chrom, start, end):
    track = spans(name).get(chrom)
    return None if track is None or start >= end else M.region(track, start, end)


@pytest.mark.parametrize("name", sorted(FILES))
def test_model_reproduces_the_new_recordings(name):
    for (chrom, s, e), want in recorded(name):
        got = model_region(name, chrom, s, e)
        if want is None:
            assert got is None, (name, chrom, s, e)
        else:
            M.assert_same(got, want, (name, chrom, s, e))


@pytest.mark.parametrize("name", sorted(PROFILE_FILES))
def test_model_reproduces_the_profile_regions(name):
    for (chrom, s, e), want in recorded_profile_regions(name):
        M.assert_same(model_region(name, chrom, s, e), want, (name, chrom, s, e))


def test_recorded_cases_cover_what_they_should():
    assert set(FILES) == {"unordered.bw", "nan.bw", "straddle.bw", "test.bw"} and len(PROFILE_FILES) == 7
    regions = {name: [r for r, _ in recorded(name)] for name in FILES}
    assert {("chrU", 0, 300), ("chrU", 25, 215), ("chrU", 44, 45)} <= set(regions["unordered.bw"])
    for name in FILES:
        assert sum(a is None for _, a in recorded(name)) >= 1, name
    nones = [r for name in FILES for r, a in recorded(name) if a is None]
    assert any(s >= e for _, s, e in nones) and any(s < e for _, s, e in nones)  # start >= end, and an unknown chromosome
    # where overlapping items disagree the order of the items shows: the same items in reverse order give other arrays
    track = spans("unordered.bw")["chrU"]
    assert not M.is_ordered(track)
    back = tuple(a[::-1] for a in track)
    for (chrom, s, e), want in recorded("unordered.bw")[:3]:
        assert not M.same_bytes(M.region(back, s, e), want), (s, e)
    # NaNs that are items' own values, between bases that have data
    (_, want) = recorded("nan.bw")[0]
    assert np.isnan(want[5:9]).all() and want[4] == 1.0 and want[9] == 2.5 and np.isnan(want[20:30]).all()
    # regions that run past the data and past the chromosome's end
    sizes = {name: {c: int(e.max()) if len(e) else 0 for c, (_, e, _) in spans(name).items()} for name in FILES}
    assert any(a is not None and e > sizes[name][c] and np.isnan(a[-1]) for name in FILES for (c, s, e), a in recorded(name))
    assert ("chr1", 247249700, 247249800) in regions["test.bw"]
    # the fill is numpy's NaN
    assert int(recorded("test.bw")[3][1].view(np.uint32)[0]) == M.NAN_BITS


def test_model_edges():
    t = M.overlap_track()
    assert M.is_ordered(t)
    got = M.region(t, 0, 95).view(np.uint32)
    assert got[0] == M.NAN_BITS and got[11] == 0x7FC00001 and got[45] == 0xFFA00000  # an item's own NaN keeps its bits
    assert M.region(t, 3, 12).tolist()[:2] == [1.5, 1.5]  # equal starts: the last item wins
    assert len(M.region(t, 9, 5)) == 0 and np.isnan(M.region(None, -3, 2)).all()
    values, offsets = M.arrays([t], [0, -1, 0], [-5, 0, 7], [4, 3, 7])
    assert offsets.tolist() == [0, 9, 12, 12] and np.isnan(values[:8]).all() and values[8] == 1.5
