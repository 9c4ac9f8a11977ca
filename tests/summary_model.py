"""
A plain Python / numpy restatement of the reference's from-full bigWig summaries (lib/bx/bbi/bbi_file.pyx:80-111, 231-260 under
bigwig_file.pyx:46-108, 176-185), which tests/test_summary_model_golden.py pins to the recorded results and the GPU tests compare
the device against.  Python floats are IEEE doubles and Python never fuses a multiply into an add, so the chains below round
exactly as the reference's x86-64 build does.

A track is (starts, ends, values): int arrays and float32 values IN FILE ORDER.  `fused=True` evaluates every  acc += a * b  with
ONE rounding (exact rational arithmetic, then a correctly rounded conversion) and `reverse=True` walks the items backwards: the
two mistakes the recorded cases must be able to see (tools/record_summary_golden.py asserts that they can).
"""
import math
from fractions import Fraction

import numpy as np

INF = float("inf")
PLANES = ("valid_count", "min_val", "max_val", "sum_data", "sum_squares")
QUERY_KEYS = ("mean", "max", "min", "coverage", "std_dev")


def _madd(acc, a, b, fused):
    if not fused or not (math.isfinite(acc) and math.isfinite(a) and math.isfinite(b)):
        return acc + a * b
    return float(Fraction(acc) + Fraction(a) * Fraction(b))


def overlapping(track, start, end):
    """indices, in file order, of the items that can meet [start, end)"""
    s, e, _ = track
    return np.nonzero((np.asarray(e) > start) & (np.asarray(s) < end))[0]


def summarize_region(track, start, end, size, fused=False, reverse=False):
    """five lists of `size` floats (valid_count, min_val, max_val, sum_data, sum_squares), or None where the reference answers None"""
    if start >= end:
        return None
    valid, mn, mx, sm, sq = [0.0] * size, [INF] * size, [-INF] * size, [0.0] * size, [0.0] * size
    step = (end - start) // size
    starts, ends, values = track
    idx = overlapping(track, start, end) if step > 0 else np.zeros(0, dtype=np.intp)
    if reverse:
        idx = idx[::-1]
    # the items' fields as Python numbers, converted once for the whole region (a long region walks tens of thousands of items)
    val32 = np.asarray(values, dtype=np.float32)[idx]
    with np.errstate(all="ignore"):
        squares = (val32 * val32).astype(np.float64).tolist()  # the square is a float32 product
    fields = zip(np.asarray(starts)[idx].tolist(), np.asarray(ends)[idx].tolist(), val32.astype(np.float64).tolist(), squares)
    for item_start, item_end, v, v2 in fields:
        s, e = max(item_start, start), min(item_end, end)
        if s >= e:
            continue
        n = e - s
        for j in range((s - start) // step, min((e - 1 - start) // step, size - 1) + 1):
            b0 = start + step * j
            overlap = min(b0 + step, e) - max(b0, s)
            if overlap > 0:
                w = n * (overlap / n)
                valid[j] += w
                sm[j] = _madd(sm[j], v, w, fused)
                sq[j] = _madd(sq[j], v2, w, fused)
                if mx[j] < v:
                    mx[j] = v
                if mn[j] > v:
                    mn[j] = v
    return [float(round(x)) for x in valid], mn, mx, sm, sq


def empty_row(size):
    return [0.0] * size, [INF] * size, [-INF] * size, [0.0] * size, [0.0] * size


def summarize(tracks, track_of, starts, ends, size, **how):
    """the batch: five float64 arrays [n, size]; a row without a track (track_of < 0) or with start >= end is an empty row"""
    n = len(starts)
    out = np.empty((5, n, size), dtype=np.float64)
    for i in range(n):
        t, s, e = int(track_of[i]), int(starts[i]), int(ends[i])
        row = summarize_region(tracks[t], s, e, size, **how) if t >= 0 else None
        out[:, i, :] = row if row is not None else empty_row(size)
    return tuple(out)


def _div(a, b):
    """float64 division as numpy scalars do it: x / 0 is +-inf or NaN, not an exception"""
    if b != 0:
        return a / b
    return float("nan") if a == 0 or math.isnan(a) else math.copysign(INF, a) * math.copysign(1.0, b)


def query_region(planes, start, end, size):
    """bbi_file.pyx:245-258 over the five lists of one region -> five lists (mean, max, min, coverage, std_dev)"""
    valid, mn, mx, sm, sq = planes
    mean, cov, std = [], [], []
    for i in range(size):
        s, v = float(sm[i]), float(valid[i])
        mean.append(_div(s, v))
        cov.append(size / (end - start) * v)
        variance = float(sq[i]) - _div(s * s, v)
        if v > 1:
            variance = _div(variance, v - 1)
        m = 0 if 0 > variance else variance  # Python's max(variance, 0): a NaN stays
        std.append(math.sqrt(m))
    return mean, list(mx), list(mn), cov, std


def stats(planes, starts, ends, size):
    """mean, coverage, std_dev of a batch as [n, size] arrays (rows with start >= end: whatever the empty row gives)"""
    n = len(starts)
    out = np.empty((3, n, size), dtype=np.float64)
    for i in range(n):
        row = [p[i] for p in planes]
        span = int(ends[i]) - int(starts[i])
        if span <= 0:
            out[:, i, :] = np.nan
            continue
        mean, _, _, cov, std = query_region(row, int(starts[i]), int(ends[i]), size)
        out[0, i], out[1, i], out[2, i] = mean, cov, std
    return tuple(out)


def picks_zoom(reductions, start, end, size):
    """whether BBIFile.summarize (bbi_file.pyx:205-215, 281-294) answers from a zoom level: reductions = the file's reduction levels"""
    desired = ((end - start) // size) // 2
    return desired > 1 and any(r <= desired for r in reductions)


def same_bits(a, b):
    """float64 arrays equal byte for byte, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))
