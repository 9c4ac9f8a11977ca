"""
Inputs and comparisons shared by the tests of the zoom-level summaries (tests/test_zoom_model_golden.py and
tests/test_zoom_kernel_host.py on the host, tests/test_gpu_zoom.py on the device): the recorded results of tests/golden/zoom, the
chunk size read out of zoom_summary.hpp, seeded ordered levels and batches with the model's answer (tests/zoom_model.py).
"""
import json
import os
import re

import numpy as np

import zoom_model as M
from summary_cases import TOP_SIZES, assert_planes, empty_planes, shifted_to_the_top, top_regions  # noqa: F401  (the byte-for-byte comparison of the five planes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "zoom")
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "zoom_summary.hpp")) as _f:
    CHUNK = int(re.search(r"constexpr int ZM_CHUNK = (\d+);", _f.read()).group(1))
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
FILES = {os.path.basename(e["file"]): e for e in MANIFEST["files"]}
SIZES = (1, 2, 64, 65, 200)
INT32_MAX = 2 ** 31 - 1

_cache = {}


def path_of(name):
    return os.path.normpath(os.path.join(GOLDEN, FILES[name]["file"])) if name in FILES else os.path.join(GOLDEN, name)


def levels(name):
    """bxmi.bigwig.read_zoom_file of a fixture file, read once"""
    from bxmi import bigwig

    if ("levels", name) not in _cache:
        _cache["levels", name] = bigwig.read_zoom_file(path_of(name))
    return _cache["levels", name]


def spans(name):
    from bxmi import bigwig

    if ("spans", name) not in _cache:
        _cache["spans", name] = bigwig.read_spans_file(path_of(name))
    return _cache["spans", name]


def recorded(name, k):
    """(case, planes [5, size], query [5, size]) of case k of a file; None arrays where the reference answered None"""
    entry = FILES[name]
    for kind in ("planes", "query"):
        if (kind, name) not in _cache:
            _cache[kind, name] = np.load(os.path.join(GOLDEN, entry[kind]))
    case = entry["cases"][k]
    if case["none"]:
        return case, None, None
    cut = slice(case["at"], case["at"] + case["size"])
    return case, _cache["planes", name][:, cut], _cache["query", name][:, cut]


def zoom_cases(name):
    """indices of the cases of a file that the reference answers from a zoom level"""
    return [k for k, c in enumerate(FILES[name]["cases"]) if c["level"] is not None]


def random_level(rng, n_records, reduction, first=0, gap_rate=0.05, edge_leaves=False):
    """an ORDERED level part: records of 1 .. reduction bases, touching or (rarely) a gap of up to 40 reductions apart, in leaves of
    1 .. 9 records whose range is their records'; with `edge_leaves` the first leaf starts on an earlier chromosome and the last
    one ends on a later one"""
    from bxmi.bigwig import ZoomArrays

    lengths = rng.integers(1, reduction + 1, size=n_records)
    gaps = np.where(rng.random(n_records) < gap_rate, rng.integers(1, 40 * reduction, size=n_records), 0)
    starts = first + np.cumsum(lengths + gaps) - lengths
    ends = starts + lengths
    valid = rng.integers(0, lengths + 1).astype(np.uint32)
    valid[rng.random(n_records) < 0.02] = 2 ** 24 + 1 + 2 * rng.integers(0, 2 ** 20)
    lo = (rng.standard_normal(n_records) * 2).astype(np.float32)
    hi = lo + np.abs(rng.standard_normal(n_records)).astype(np.float32)
    lo[rng.random(n_records) < 0.02] = np.nan
    hi[rng.random(n_records) < 0.02] = np.nan
    sums = (rng.standard_normal(n_records) * np.exp2(rng.integers(-8, 9, size=n_records))).astype(np.float32)
    sumsq = np.abs(sums * rng.uniform(0.5, 3.0, size=n_records)).astype(np.float32)
    first_of, at = [0], 0
    while at < n_records:
        at = min(at + int(rng.integers(1, 10)), n_records)
        first_of.append(at)
    first_of = np.array(first_of, dtype=np.int64)
    leaf_lo, leaf_hi = starts[first_of[:-1]].astype(np.int32), ends[first_of[1:] - 1].astype(np.int32)
    if edge_leaves and len(leaf_lo):
        leaf_lo[0], leaf_hi[-1] = -1, INT32_MAX
    return ZoomArrays(starts.astype(np.int32), ends.astype(np.int32), valid, lo, hi, sums, sumsq, leaf_lo, leaf_hi, first_of)


def chunk_level():
    """records [3 k, 3 k + 3) in leaves of 5: the region [3 a, 3 (a + r)) in one bin walks exactly r of them"""
    from bxmi.bigwig import ZoomArrays

    n = 4 * CHUNK + 130
    k = np.arange(n, dtype=np.int32)
    sums = (np.sin(k.astype(np.float64)) * 3.0).astype(np.float32)
    first_of = np.append(np.arange(0, n, 5, dtype=np.int64), n)
    return ZoomArrays(3 * k, 3 * k + 3, (1 + k % 3).astype(np.uint32), sums - 1, sums + 1, sums, sums * sums, (3 * first_of[:-1]).astype(np.int32),
                      (3 * first_of[1:]).astype(np.int32), first_of)


def empty_level():
    from bxmi.bigwig import ZoomArrays

    z32, zf = np.zeros(0, np.int32), np.zeros(0, np.float32)
    return ZoomArrays(z32, z32, np.zeros(0, np.uint32), zf, zf, zf, zf, z32, z32, np.zeros(1, np.int64))


CHUNK_RUNS = (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 2 * CHUNK)


def differential_case(size):
    """(level parts, track_of, starts, ends, the model's answer), once per size: several tracks and levels in one batch -- a fine
    and a coarse level, one whose outer leaves reach other chromosomes, the chunk level, an empty one -- rows without a track and
    with start >= end, regions narrower than their bins are many (step 0), regions that walk runs around the chunk size in one
    bin, a fine level under a wide region (a long run), a region that ends at 2^31 - 1"""
    if size not in _cache:
        rng = np.random.default_rng(300 + size)
        tracks = [random_level(rng, 3000, 16, first=500), random_level(rng, 700, 64, first=100, gap_rate=0.2),
                  random_level(rng, 400, 8, first=2000, edge_leaves=True), chunk_level(), empty_level()]
        n = 360
        track_of = rng.integers(-1, 5, size=n)
        reach = np.array([int(t.end.max()) if len(t.end) else 100 for t in tracks] + [100])[track_of]
        starts = (rng.random(n) * (reach + 400)).astype(np.int64)
        widths = np.where(rng.random(n) < 0.5, rng.integers(1, 4 * size + 2, size=n), rng.integers(1, 9000, size=n))
        widths[:8] = (size, size - 1 if size > 1 else 1, size + 1, 2 * size + 1, 1, 64 * size, 65 * size + 3, 63 * size)
        ends = starts + widths
        ends[8:12] = starts[8:12] - np.array([0, 1, 5, 0])  # start >= end: empty rows
        extra_start = np.array([3 * 5 + 1] * len(CHUNK_RUNS))
        extra_end = 3 * 5 + 3 * np.array(CHUNK_RUNS)
        track_of = np.concatenate([track_of, [3] * len(CHUNK_RUNS), [0, 2, 2]]).astype(np.int32)
        starts = np.concatenate([starts, extra_start, [0, 2 ** 31 - 2 - 4 * size, 0]]).astype(np.int32)
        ends = np.concatenate([ends, extra_end, [int(tracks[0].end.max()) + 77, INT32_MAX, 1500]]).astype(np.int32)
        _cache[size] = (tracks, track_of, starts, ends, M.summarize(tracks, track_of, starts, ends, size))
    return _cache[size]


def top_case(size):
    """(level parts, track_of, starts, ends, the model's answer), once per size: two levels of 2000 records (one with many gaps),
    records and leaf ranges shifted by one amount so that the last record and the last leaf end at exactly 2^31 - 1, under
    summary_cases.top_regions()"""
    if ("top", size) not in _cache:
        rng = np.random.default_rng(700 + size)
        tracks = []
        for gap_rate in (0.05, 0.2):
            z = random_level(rng, 2000, 16, first=40, gap_rate=gap_rate)
            end, start, leaf_lo, leaf_hi = shifted_to_the_top(z.end, z.start, z.leaf_lo, z.leaf_hi)
            tracks.append(z._replace(start=start, end=end, leaf_lo=leaf_lo, leaf_hi=leaf_hi))
        assert all(int(z.end[-1]) == INT32_MAX and int(z.leaf_hi[-1]) == INT32_MAX for z in tracks)
        track_of, starts, ends = top_regions(rng, [z.start[0] for z in tracks], size)
        _cache["top", size] = (tracks, track_of, starts, ends, M.summarize(tracks, track_of, starts, ends, size))
    return _cache["top", size]
