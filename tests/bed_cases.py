"""
Inputs and comparisons shared by the tests of the bigBed coverage summaries (tests/test_gpu_bed_summary.py on the device,
tests/test_bed_summary_kernel_host.py on the host, tests/test_bigbed_model_golden.py on the model): the chunk size read out of
bed_summary.hpp, what tools/record_bigbed_golden.py recorded under tests/golden/bigbed, seeded tracks and batches, the chunk
cases, the cases of more than 64 chunks (window_cases) and the tracks that end at 2^31 - 1 (top_case) with the model's answer --
tests/summary_model.py over the same records as items of value 1, which is what the reference computes
(tests/test_bigbed_model_golden.py pins it to the recorded arrays).
"""
import json
import os
import re

import numpy as np

import summary_model as M
from summary_cases import TOP_SIZES, shifted_to_the_top, top_regions  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bigbed")
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "bed_summary.hpp")) as _f:
    CHUNK = int(re.search(r"constexpr int BD_CHUNK = (\d+);", _f.read()).group(1))
with open(os.path.join(GOLDEN, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
FILES = {entry["file"]: entry for entry in MANIFEST["files"]}
SIZES = (1, 2, 3, 63, 64, 65, 200)
INT32_MAX = 2 ** 31 - 1

_items, _arrays = {}, {}


def path_of(name):
    return os.path.join(GOLDEN, name)


def items(name):
    """{chrom: (starts, ends, rest)} of a fixture, read once"""
    from bxmi import bigbed

    if name not in _items:
        _items[name] = bigbed.read_items_file(path_of(name))
    return _items[name]


def with_ones(track):
    """(starts, ends) -> the span track of tests/summary_model.py with every value 1"""
    return track[0], track[1], np.ones(len(track[0]), dtype=np.float32)


def recorded(name, k):
    """(case, from-full planes [5, size], summarize planes [5, size], query [5, size]) of case k of a file; None arrays where the
    reference answers None"""
    entry = FILES[name]
    if name not in _arrays:
        _arrays[name] = [np.load(os.path.join(GOLDEN, entry[key])) for key in ("planes", "summarize", "query")]
    case = entry["cases"][k]
    if case["none"]:
        return case, None, None, None
    cut = slice(case["at"], case["at"] + case["size"])
    return (case,) + tuple(a[:, cut] for a in _arrays[name])


def assert_planes(got, want, what):
    for name, g, w in zip(M.PLANES, got, want):
        g = np.asarray(g)
        assert g.dtype == np.float64 and g.shape == np.asarray(w).shape, (what, name, g.shape)
        if not M.same_bits(g, w):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [float(g[tuple(b)]) for b in bad[:4]], [float(w[tuple(b)]) for b in bad[:4]]))


def empty_planes(size):
    return np.array(M.empty_row(size))


def model(tracks, track_of, starts, ends, size):
    """the model's five planes [n, size] for bed tracks (starts, ends); a track_of outside the list is no track"""
    ones = [with_ones(t) for t in tracks]
    track_of = [int(t) if 0 <= int(t) < len(tracks) else -1 for t in track_of]
    return M.summarize(ones, track_of, starts, ends, size)


def by_size(name):
    """[(size, case indices, track_of, starts, ends)] of a file's recorded cases: all regions that share a size form one batch,
    rows the reference answers with None included; track_of counts the file's chromosomes in order"""
    order, cases, out = list(FILES[name]["chroms"]), FILES[name]["cases"], []
    for size in sorted({c["size"] for c in cases}):
        ks = [k for k, c in enumerate(cases) if c["size"] == size]
        rows = [cases[k] for k in ks]
        out.append((size, ks, [order.index(c["chrom"]) if c["chrom"] in order else -1 for c in rows], [c["start"] for c in rows], [c["end"] for c in rows]))
    return out


def recorded_batch(name, ks, size, which=1):
    """the recorded planes [5, rows, size] of cases `ks` (which: 1 from full data, 2 what summarize answered)"""
    return np.stack([recorded(name, k)[which] if not FILES[name]["cases"][k]["none"] else empty_planes(size) for k in ks], axis=1)


# ------------------------------------------------------------ seeded tracks --
def nested_track(rng, n):
    """sorted starts; most records short, one in ten long enough to hold many others: the ends descend all the time"""
    starts = np.sort(rng.integers(0, 20 * n, size=n))
    lengths = np.where(rng.random(n) < 0.1, rng.integers(200, 5000, size=n), rng.integers(1, 61, size=n))
    return starts.astype(np.int32), (starts + lengths).astype(np.int32)


def spanning_track(rng, n):
    """the first record spans the chromosome; short records with gaps follow"""
    lengths = rng.integers(1, 50, size=n)
    starts = np.cumsum(lengths + rng.integers(0, 40, size=n)) - lengths
    starts, ends = np.concatenate([[0], starts]), np.concatenate([[int(starts[-1]) + 5000], starts + lengths])
    return starts.astype(np.int32), ends.astype(np.int32)


def equal_starts_track(rng, n):
    """many records per start, their ends in any order"""
    starts = np.sort(rng.choice(np.arange(0, 40 * n, 37), size=n // 12)[rng.integers(0, n // 12, size=n)])
    return starts.astype(np.int32), (starts + rng.integers(1, 120, size=n)).astype(np.int32)


def zero_length_track(rng, n):
    starts = np.sort(rng.integers(0, 12 * n, size=n))
    lengths = np.where(rng.random(n) < 0.3, 0, rng.integers(1, 70, size=n))
    return starts.astype(np.int32), (starts + lengths).astype(np.int32)


def shuffled(rng, track):
    perm = rng.permutation(len(track[0]))
    return track[0][perm].copy(), track[1][perm].copy()


EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))
_diff = {}


def differential_case(size):
    """(host tracks, track_of, starts, ends, the model's answer), once per size: 150 regions over six tracks -- sorted with
    nesting, first record spanning the chromosome, many equal starts, zero-length records, not sorted, empty -- with rows without
    a track, rows with start >= end and regions that end at 2^31 - 1"""
    if size not in _diff:
        rng = np.random.default_rng(300 + size)
        tracks = [nested_track(rng, 3000), spanning_track(rng, 2500), equal_starts_track(rng, 1500), zero_length_track(rng, 800),
                  shuffled(rng, nested_track(rng, 300)), EMPTY]
        n = 150
        track_of = rng.integers(-1, 7, size=n)  # (-1 and 6: no track)
        reach = np.array([int(t[1].max()) if len(t[1]) else 100 for t in tracks] + [100, 100])[track_of]
        starts = (rng.random(n) * (reach + 50)).astype(np.int64)
        widths = np.where(rng.random(n) < 0.5, rng.integers(1, 4 * size + 2, size=n), rng.integers(1, 6000, size=n))
        widths[:8] = (size, size - 1 if size > 1 else 1, size + 1, 2 * size + 1, 1, 64 * size, 65 * size + 3, 63 * size)
        ends = starts + widths
        ends[8:12] = starts[8:12] - np.array([0, 1, 5, 0])  # start >= end: empty rows
        # whole tracks, and regions at the end of int32 (the spanning track's first record is all that could reach them)
        whole = [(t, 0, int(tracks[t][1].max())) for t in range(5)]
        far = [(0, INT32_MAX - 1 - 4 * size, INT32_MAX), (1, INT32_MAX - 200 * size, INT32_MAX), (5, 0, INT32_MAX)]
        track_of = np.concatenate([track_of, [r[0] for r in whole + far]]).astype(np.int32)
        starts = np.concatenate([starts, [r[1] for r in whole + far]]).astype(np.int32)
        ends = np.concatenate([ends, [r[2] for r in whole + far]]).astype(np.int32)
        _diff[size] = (tracks, track_of, starts, ends, model(tracks, track_of, starts, ends, size))
    return _diff[size]


# ------------------------------------------------------------ chunk cases --
def run_track():
    """records [3 k, 3 k + 3): the region [3 a, 3 (a + r)) meets exactly r of them"""
    k = np.arange(4 * CHUNK + 128, dtype=np.int32)
    return 3 * k, 3 * k + 3


def skip_track():
    """record 0 reaches to the end (so every region's first record is record 0, in chunk 0); the rest of chunk 0 and all of chunk 1
    are short records that end before base 100000; chunk 2 and a part of chunk 3 lie from base 100000 on.  A region there has its
    `lo` at 0, stages chunk 0, SKIPS chunk 1 and counts in chunks 2 and 3."""
    k = np.arange(2 * CHUNK - 1, dtype=np.int64)
    near_s, near_e = 10 + 5 * k, 10 + 5 * k + 1 + k % 9
    j = np.arange(CHUNK + 40, dtype=np.int64)
    far_s = 100000 + 4 * j
    far_e = far_s + 1 + (j * 7) % 23
    starts, ends = np.concatenate([[0], near_s, far_s]), np.concatenate([[200000], near_e, far_e])
    assert near_e.max() < 100000 and len(starts) == 3 * CHUNK + 40
    return starts.astype(np.int32), ends.astype(np.int32)


_chunk = []


def chunk_cases():
    """[(label, tracks, track_of, starts, ends, size, the model's answer)]"""
    if _chunk:
        return _chunk
    rng = np.random.default_rng(77)
    runs, skip = run_track(), skip_track()
    lengths = [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 2 * CHUNK]
    # from record 5 (lo mid-chunk); from record CHUNK - 3 (the run crosses an aligned boundary at once); from record CHUNK (aligned)
    regions = [(3 * first + 1, 3 * (first + r)) for first in (5, CHUNK - 3, CHUNK) for r in lengths if first + r <= len(runs[0])]
    starts, ends = (np.array(x, dtype=np.int32) for x in zip(*regions))
    zeros = np.zeros(len(regions), dtype=np.int32)
    cases = []
    for size in (1, 2, 3):  # (size 2 over 2 CHUNK records from an aligned start: every record of bin 1 lies in the second chunk)
        cases.append(("runs, %d bins" % size, [runs], zeros, starts, ends, size))
    back = shuffled(rng, runs)
    cases.append(("runs shuffled: the general walk", [back], zeros, starts, ends, 3))
    s2 = np.array([100000, 100003, 100000, 99990, 0, 100500], dtype=np.int32)
    e2 = np.array([100000 + 4 * CHUNK, 100900, 100064, 100010, 200000, 100700], dtype=np.int32)
    z2 = np.zeros(len(s2), dtype=np.int32)
    for size in (1, 3, 64, 65):
        cases.append(("a skipped chunk, %d bins" % size, [skip], z2, s2, e2, size))
    cases.append(("the same records shuffled", [shuffled(rng, skip)], z2, s2, e2, 3))
    _chunk.extend(c + (model(c[1], c[2], c[3], c[4], c[5]),) for c in cases)
    return _chunk


# ------------------------------------------------------------ chunk windows --
# bd_summary_kernel tests a run's chunks 64 at a time (lane = chunk): a run of more than 64 chunks takes a second window
WINDOW = 64


def at(c):
    """the start of record c of paced_records()"""
    return 10 + 5 * c


def paced_records(n):
    """record k = [10 + 5 k, 10 + 5 k + 1 + (7 k mod 9)): sorted, 1 to 9 bases long, a start every 5 bases"""
    k = np.arange(n, dtype=np.int64)
    return at(k), at(k) + 1 + (7 * k) % 9


def long_track():
    """150 CHUNK + 77 paced records -- three windows of chunks, the last one partly filled, its last chunk partly filled -- with
    three ends raised: record 0 ends 500 bases behind the last start (every region's first record is record 0), record
    70 CHUNK + 13 ends 100 bases behind it (a far-reaching record inside the second window), record 100 CHUNK + 200 ends where record
    140 CHUNK starts.  A region near the end stages chunk 0, chunk 70, perhaps chunk 100 and its own, and skips all between."""
    starts, ends = paced_records(150 * CHUNK + 77)
    ends[0], ends[70 * CHUNK + 13], ends[100 * CHUNK + 200] = starts[-1] + 500, starts[-1] + 100, at(140 * CHUNK)
    return starts.astype(np.int32), ends.astype(np.int32)


def plain_track():
    """the records of long_track() without the raised ends: a region's first record is its own, so its first chunk is any chunk"""
    starts, ends = paced_records(150 * CHUNK + 77)
    return starts.astype(np.int32), ends.astype(np.int32)


def big_track():
    """2^20 + 77 paced records, 4097 chunks: record 0 spans everything, and every 100000th record reaches 40 chunks ahead"""
    n = 2 ** 20 + 77
    starts, ends = paced_records(n)
    ends[0] = starts[-1] + 500
    for k in range(100000, n - 40 * CHUNK, 100000):
        ends[k] = at(k + 40 * CHUNK)
    return starts.astype(np.int32), ends.astype(np.int32)


def staged_chunks(track, s, e):
    """(c_first, c_end, the chunks of [c_first, c_end) that the kernel stages) for the region [s, e) of a sorted track in ONE bin,
    worked out from the definitions: the run [glo, ghi) is from the first record at or behind which something ends after s to the
    first that starts at or after e; a chunk is staged when one of its records inside the run ends after s"""
    starts, ends = (np.asarray(a, dtype=np.int64) for a in track)
    glo = int(np.searchsorted(np.maximum.accumulate(ends), s, side="right"))
    ghi = max(int(np.searchsorted(starts, e - 1, side="right")), glo)
    c_first, c_end = glo // CHUNK, (ghi + CHUNK - 1) // CHUNK
    return c_first, c_end, [c for c in range(c_first, c_end) if ends[c * CHUNK:min((c + 1) * CHUNK, ghi)].max() > s]


_window = []


def window_cases():
    """[(label, tracks, track_of, starts, ends, size, the model's answer)]: runs of more than WINDOW chunks"""
    if _window:
        return _window
    rng = np.random.default_rng(78)
    long, plain, big = long_track(), plain_track(), big_track()
    last = int(long[0][-1])
    # on `long`: near the end; where record 100 CHUNK + 200 still reaches; two wide ones; everything; a narrow one; beyond the last
    # short record, where only records 0 and 70 CHUNK + 13 reach
    regions = [(at(149 * CHUNK + 5), 400), (at(140 * CHUNK - 3), 3000), (at(66 * CHUNK), 90 * CHUNK * 5), (at(5 * CHUNK + 9), 70 * CHUNK * 5),
               (0, int(long[1][0])), (at(130 * CHUNK), 64), (last + 20, 70)]
    wide = [2, 4]
    starts = np.array([r[0] for r in regions], dtype=np.int32)
    ends = np.array([r[0] + r[1] for r in regions], dtype=np.int32)
    assert sorted(range(len(regions)), key=lambda k: regions[k][1])[-2:] == wide
    c_first, c_end, staged = staged_chunks(long, starts[1], ends[1])
    assert (c_first, c_end) == (0, 143) and staged[:3] == [0, 70, 100] and staged[3:] == list(range(139, 143)), (c_first, c_end, staged)
    assert staged_chunks(long, starts[0], ends[0])[2] == [0, 70, 149] and staged_chunks(long, starts[6], ends[6]) == (0, 151, [0, 70])
    assert staged_chunks(long, starts[4], ends[4])[2] == list(range(151))
    zeros = np.zeros(len(regions), dtype=np.int32)
    back = shuffled(rng, long)
    # on `plain`: runs of exactly 63, 64, 65 and 128 chunks from an aligned first record and from one in the middle of chunk 5
    runs = [(64 * CHUNK, 63), (64 * CHUNK, 64), (64 * CHUNK, 65), (16 * CHUNK, 128), (5 * CHUNK + 9, 63), (5 * CHUNK + 9, 64), (5 * CHUNK + 9, 65),
            (5 * CHUNK + 9, 128)]
    run_starts = np.array([at(first) for first, _ in runs], dtype=np.int32)
    run_ends = np.array([at(first + r * CHUNK) for first, r in runs], dtype=np.int32)
    spans = [staged_chunks(plain, s, e) for s, e in zip(run_starts, run_ends)]
    assert [(c0, c1 - c0) for c0, c1, _ in spans] == [(64, 63), (64, 64), (64, 65), (16, 128), (5, 64), (5, 65), (5, 66), (5, 129)], spans
    assert all(chunks == list(range(c0, c1)) for c0, c1, chunks in spans)
    run_zeros = np.zeros(len(runs), dtype=np.int32)
    cases = []
    for size in (1, 3, 64, 65):
        cases.append(("long, %d bins" % size, [long], zeros, starts, ends, size))
        cases.append(("plain: runs of 63 to 129 chunks, %d bins" % size, [plain], run_zeros, run_starts, run_ends, size))
        cases.append(("long shuffled: the general walk, %d bins" % size, [back], zeros, starts, ends, size))
    cases.append(("long, the two widest regions, 200 bins", [long], zeros[wide], starts[wide], ends[wide], 200))
    # the scenario of a whole chromosome: 200 regions of 50 to 50000 bases all over `big`, each with 64 windows or so to test
    n = 200
    big_starts = rng.integers(0, int(big[0][-1]), size=n)
    big_ends = big_starts + (50 * 1000 ** rng.random(n)).astype(np.int64)
    big_starts[:2], big_ends[:2] = (at(2 ** 20) - 30, at(400000 + 40 * CHUNK) - 40), (at(2 ** 20) + 49970, at(400000 + 40 * CHUNK) + 10)
    assert (big_ends - big_starts).min() >= 50 and (big_ends - big_starts).max() <= 50000
    c_first, c_end, staged = staged_chunks(big, big_starts[1], big_ends[1])
    assert c_first == 0 and c_end > 8 * WINDOW and len(staged) <= 4 and 400000 // CHUNK in staged, (c_first, c_end, staged)
    for size in (1, 65):
        cases.append(("big, %d bins" % size, [big], np.zeros(n, dtype=np.int32), big_starts.astype(np.int32), big_ends.astype(np.int32), size))
    _window.extend(c + (model(c[1], c[2], c[3], c[4], c[5]),) for c in cases)
    return _window


# ------------------------------------------------------------ records that end at 2^31 - 1 --
_top = {}


def top_case(size):
    """(host tracks, track_of, starts, ends, the model's answer), once per size: a nested and a spanning track of 2000 records,
    each shifted so that its furthest end is exactly 2^31 - 1, under summary_cases.top_regions()"""
    if size not in _top:
        rng = np.random.default_rng(600 + size)
        tracks = []
        for s, e in (nested_track(rng, 2000), spanning_track(rng, 1999)):
            e, s = shifted_to_the_top(e, s)
            tracks.append((s, e))
        assert all(len(t[0]) == 2000 and int(t[1].max()) == INT32_MAX for t in tracks)
        track_of, starts, ends = top_regions(rng, [t[0].min() for t in tracks], size)
        _top[size] = (tracks, track_of, starts, ends, model(tracks, track_of, starts, ends, size))
    return _top[size]
