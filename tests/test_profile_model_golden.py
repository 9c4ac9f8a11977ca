"""CPU-only: tests/profile_model.py reproduces every result recorded from the reference (tests/golden/profile, written by
tools/record_profile_golden.py): `totals` byte for byte (NaN compared as NaN), `valid`, and the savetxt text.  The model reads the
tracks out of the recorded ``get_as_array`` arrays where a case's windows lie inside a recorded region, so it does not depend
on the project's bigWig reader (tests/test_bigwig_reader.py pins that one separately).

Also here: the synthetic wide-range case that the GPU tests use for the ordered chain is order-sensitive enough to tell a chain
from anything else -- at least half of its columns differ from the same chain split in two halves (measured when the goldens
were recorded: 78 % differ from the split, 88 % from math.fsum)."""
import json
import math
import os

import numpy as np
import pytest

import profile_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile")
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
FILES = {f["file"]: f for f in MANIFEST["files"]}
PROFILES = {p["name"]: p for p in MANIFEST["profiles"]}


def recorded_regions(name):
    """[((chrom, start, end), float32 array)] of one bigWig file"""
    entry = FILES[name]
    flat = np.load(os.path.join(GOLDEN, entry["arrays"]))
    out, at = [], 0
    for chrom, s, e in entry["regions"]:
        out.append(((chrom, s, e), flat[at:at + e - s]))
        at += e - s
    assert at == len(flat)
    return out


def recorded_tracks(name):
    """{chrom: (offset, float32 array)}: per chromosome the LONGEST recorded region, standing for the track over [offset, offset + len)"""
    best = {}
    for (chrom, s, e), a in recorded_regions(name):
        if chrom not in best or len(a) > len(best[chrom][1]):
            best[chrom] = (s, a)
    return best


def model_case(case):
    """(totals, valid) of the model over a recorded case, windows cut from the recorded regions"""
    tracks = recorded_tracks(case["scores"])
    names = list(tracks)
    rows = M.bed_rows(os.path.join(GOLDEN, case["bed"]))
    chroms, starts, width = M.centred_windows(rows, case["padding"])
    dense, shifted = [], []
    for c, s in zip(chroms, starts):
        off, a = tracks[c]
        size = FILES[case["scores"]]["chroms"][c]
        # the recorded region is the whole chromosome, or holds the whole window: otherwise the model would invent NaNs
        assert (off == 0 and len(a) >= size) or (s >= off and s + width <= off + len(a)), (case["name"], c, s)
        shifted.append(s - off)
        dense.append(names.index(c))
    return M.profile([tracks[c][1] for c in names], dense, shifted, width)


@pytest.mark.parametrize("name", sorted(PROFILES))
def test_model_reproduces_the_recorded_profile(name):
    case = PROFILES[name]
    totals, valid = model_case(case)
    want_totals = np.load(os.path.join(GOLDEN, case["totals"]))
    want_valid = np.load(os.path.join(GOLDEN, case["valid"]))
    assert want_totals.dtype == np.float64 and want_valid.dtype == np.int32 and len(want_totals) == 2 * case["padding"]
    assert np.array_equal(valid, want_valid)
    nan = np.isnan(want_totals)
    assert np.array_equal(np.isnan(totals), nan)
    assert totals[~nan].tobytes() == want_totals[~nan].tobytes()
    with open(os.path.join(GOLDEN, case["text"])) as f:
        assert M.text(totals, valid) == f.read()


def test_recorded_cases_cover_what_they_should():
    assert len(PROFILES) >= 8 and all(p["rows"] > 0 for p in PROFILES.values())
    # a case with an inf - inf or 0 / 0 column, one with two chromosomes interleaved, the reference's own file
    assert any("nan" in open(os.path.join(GOLDEN, p["text"])).read() for p in PROFILES.values())
    assert len(FILES["two.z.bw"]["chroms"]) == 2 and "test.bw" in FILES


def test_window_is_nan_outside_the_track():
    t = np.arange(5, dtype=np.float32)
    assert np.array_equal(M.window(t, -2, 4), np.array([np.nan, np.nan, 0, 1], dtype=np.float32), equal_nan=True)
    assert np.array_equal(M.window(t, 3, 4), np.array([3, 4, np.nan, np.nan], dtype=np.float32), equal_nan=True)
    assert np.isnan(M.window(t, 9, 3)).all() and np.isnan(M.window(t, -9, 3)).all() and np.isnan(M.window(t[:0], 0, 2)).all()


def test_wide_range_case_tells_a_chain_from_anything_else():
    tracks, track_of, starts, width = M.wide_range_case()
    assert len(tracks[0]) == 20000 and len(starts) == 600 and width == 130
    assert starts.min() < 0 and abs(np.isnan(tracks[0]).mean() - 0.10) < 0.01
    assert M.fraction_split_sensitive(tracks, track_of, starts, width) >= 0.5
    # and from the correctly rounded sum
    totals, _ = M.profile(tracks, track_of, starts, width)
    exact = np.empty(width)
    for j in range(width):
        col = [float(v) for s in starts for v in [M.window(tracks[0], s + j, 1)[0]] if not math.isnan(v)]
        exact[j] = math.fsum(col)
    assert np.mean(totals != exact) >= 0.5
