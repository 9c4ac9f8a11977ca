"""
A plain Python restatement of the reference's bigWig summaries FROM A ZOOM LEVEL (lib/bx/bbi/bbi_file.pyx:187-215, 281-294,
296-432 over cirtree_file.pyx:5-20, 49-105), which tests/test_zoom_model_golden.py pins to the recorded results and the kernel
tests compare the device against.

A level part is what bxmi.bigwig.read_zoom_file returns per chromosome (any object with its fields): the summary records in load
order and the leaf entries that decide which of them a region loads.  The walk is the reference's own, deque included: the list
of loaded records is shared by the bins of a region and loses records at its front only, so it is right for levels that are not
ordered as well.

`reading` names the roundings of  acc += record field * overlap_factor  (the accumulators are C floats):
    "a"  the product and the sum are each rounded to float32;
    "b"  the product and the sum are each rounded to float64, the sum then to float32 -- what the reference's build performs,
         because its loop variable is an untyped object: the fields arrive as Python numbers (tools/record_zoom_golden.py).
`reverse=True` accumulates each bin's records backwards.  The recorder asserts that its cases can see both differences.
"""
import collections

import numpy as np

import summary_model as S

NAN = float("nan")
PLANES, QUERY_KEYS, same_bits, query_region = S.PLANES, S.QUERY_KEYS, S.same_bits, S.query_region
READING = "b"


def f32(x):
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def pick_level(reductions, start, end, size):
    """index into `reductions` (file order) of the level BBIFile.summarize takes, or None for full data"""
    desired = ((end - start) // size) // 2
    if desired <= 1:
        return None
    best, best_diff = None, 2 ** 31 - 1
    for k, r in enumerate(reductions):
        diff = desired - r
        if 0 <= diff < best_diff:
            best, best_diff = k, diff
    return best


def loaded(z, start, end):
    """indices of the records a region loads: those of every leaf entry that overlaps it, in leaf order"""
    out = []
    for k in range(len(z.leaf_lo)):
        if start < int(z.leaf_hi[k]) and end > int(z.leaf_lo[k]):
            out.extend(range(int(z.leaf_first[k]), int(z.leaf_first[k + 1])))
    return out


def _add(acc, field, factor, reading):
    with np.errstate(all="ignore"):
        if reading == "a":
            return float(np.float32(acc) + np.float32(np.float32(field) * np.float32(factor)))
        return float(np.float32(acc + float(field) * factor))


def summary_slice(z, records, b0, b1, reading=READING, reverse=False):
    """_get_summary_slice: (valid, min, max, sum, sumsq) of the bin [b0, b1) over `records` (indices, the deque as it stands)"""
    if not records:
        return 0.0, NAN, NAN, 0.0, 0.0
    mn, mx = float(z.min[records[0]]), float(z.max[records[0]])
    walked = []
    for i in records:
        if int(z.start[i]) >= b1:
            break
        walked.append(i)
    valid = sm = sq = 0.0
    for i in (walked[::-1] if reverse else walked):
        s, e = int(z.start[i]), int(z.end[i])
        overlap = min(b1, e) - max(b0, s)
        if overlap > 0:
            factor = f32(overlap / (e - s))
            valid = _add(valid, int(z.valid[i]), factor, reading)
            sm = _add(sm, z.sum[i], factor, reading)
            sq = _add(sq, z.sumsq[i], factor, reading)
            if mx < float(z.max[i]):
                mx = float(z.max[i])
            if mn > float(z.min[i]):
                mn = float(z.min[i])
    return valid, mn, mx, sm, sq


def summarize_region(z, start, end, size, reading=READING, reverse=False):
    """ZoomLevel._summarize: five lists of `size` floats (valid_count, min_val, max_val, sum_data, sum_squares)"""
    records = collections.deque(loaded(z, start, end))
    step = (end - start) // size
    out = [[], [], [], [], []]
    b0 = b1 = start
    for _ in range(size):
        b1 += step
        while records and int(z.end[records[0]]) <= b0:
            records.popleft()
        for plane, x in zip(out, summary_slice(z, records, b0, b1, reading, reverse)):
            plane.append(x)
        b0 = b1
    return out


def summarize(tracks, track_of, starts, ends, size, **how):
    """the batch: five float64 arrays [n, size]; a row without a track, with start >= end or with a negative coordinate is the
    empty row of the full-data path"""
    n = len(starts)
    out = np.empty((5, n, size), dtype=np.float64)
    for i in range(n):
        t, s, e = int(track_of[i]), int(starts[i]), int(ends[i])
        out[:, i, :] = summarize_region(tracks[t], s, e, size, **how) if 0 <= t < len(tracks) and 0 <= s < e else S.empty_row(size)
    return tuple(out)
