"""
A NumPy restatement of what the reference's scripts/bed_bigwig_profile.py computes (:29-41) over dense float32 tracks -- the
model the device path is compared with, itself pinned to the reference's recorded results by tests/test_profile_model_golden.py.

  * a track is float32, NaN where the file has nothing (what BigWigFile.get_as_array fills, lib/bx/bbi/bigwig_file.pyx:122-137);
    `window` cuts [start, start + width) out of it, NaN outside the track, whoever filled the track;
  * per window, in input order: the NaNs become +0.0, the float32 row is added into a float64 accumulator (numpy converts each
    value to double, then one rounded add per element), and every position that was not NaN counts;
  * the text is savetxt of totals / valid: one %.18e per line, nan where nothing counted.
"""
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scores_model  # noqa: E402


def window(track, start, width):
    """float32[width]: track[start : start + width], NaN where that leaves [0, len(track))"""
    out = np.full(int(width), np.nan, dtype=np.float32)
    start = int(start)
    lo, hi = max(start, 0), min(start + int(width), len(track))
    if lo < hi:
        out[lo - start:hi - start] = track[lo:hi]
    return out


def profile(tracks, track_of, win_starts, width):
    """(totals float64[width], valid int32[width]) of windows win_starts[i] on tracks[track_of[i]] (-1: no track), one chain per
    column over the windows in the order given"""
    totals = np.zeros(int(width), dtype=np.float64)
    valid = np.zeros(int(width), dtype=np.int32)
    nothing = np.zeros(0, dtype=np.float32)
    for t, s in zip(track_of, win_starts):
        row = window(tracks[t] if t >= 0 else nothing, s, width)
        has = ~np.isnan(row)
        totals += np.where(has, row, np.float32(0.0))
        valid += has
    return totals, valid


def text(totals, valid):
    out = io.StringIO()
    with np.errstate(all="ignore"):
        np.savetxt(out, totals / valid)
    return out.getvalue()


def centred_windows(rows, padding):
    """(chromosome names, window starts, width) of BED rows [(chrom, start, end)]: the window of 2 * padding bases around
    floor((start + end) / 2)"""
    return [r[0] for r in rows], [(int(r[1]) + int(r[2])) // 2 - int(padding) for r in rows], 2 * int(padding)


def bed_rows(path):
    with open(path) as f:
        return [(x[0], int(x[1]), int(x[2])) for x in (line.split("\t") for line in f if line.strip() and not line.startswith("#"))]


def fill_spans(size, spans):
    """dense track of (starts, ends, values) span arrays, applied in order"""
    return scores_model.fill(size, *spans)


def load_wiggle(path):
    """{chrom: dense float32 track} of a wiggle file (.gz too), sized to its largest span end"""
    with scores_model.open_text(path) as f:
        return scores_model.load_wiggle(f)


def wide_range_case():
    """(tracks, track_of, win_starts, width): scores over 80 binary orders of magnitude, so that almost every column's float64
    chain rounds and its result depends on the order of the adds"""
    rng = np.random.default_rng(7)
    size, n, width = 20000, 600, 130
    track = (rng.standard_normal(size) * np.exp2(rng.integers(-40, 41, size=size))).astype(np.float32)
    track[rng.random(size) < 0.10] = np.nan
    starts = rng.integers(-50, size - 80, size=n).astype(np.int32)
    return [track], np.zeros(n, dtype=np.int32), starts, width


def fraction_split_sensitive(tracks, track_of, win_starts, width):
    """the fraction of columns whose ordered sum differs from the same chain cut into two halves that are summed separately"""
    whole, _ = profile(tracks, track_of, win_starts, width)
    half = len(track_of) // 2
    a, _ = profile(tracks, track_of[:half], win_starts[:half], width)
    b, _ = profile(tracks, track_of[half:], win_starts[half:], width)
    return float(np.mean(whole.view(np.uint64) != (a + b).view(np.uint64)))
