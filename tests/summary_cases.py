"""
Inputs and comparisons shared by the tests of the binned summaries (tests/test_gpu_summary.py on the device,
tests/test_summary_kernel_host.py on the host): the chunk size read out of summary.hpp, seeded tracks and batches with the model's
answer (tests/summary_model.py), and the byte-for-byte comparison of the five planes.  The tests of the zoom and bed summaries
share two things with them: the regions under tracks that end at 2^31 - 1 (top_regions) and the batch of more than one slab of the
host form with its checks (slab_batch, assert_slabs; the slab size is read out of summary.hip).
"""
import os
import re

import numpy as np

import summary_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "summary.hpp")) as _f:
    CHUNK = int(re.search(r"constexpr int SM_CHUNK = (\d+);", _f.read()).group(1))
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "summary.hip")) as _f:
    _m = re.search(r"constexpr int64_t SM_SLAB_CELLS = (\d+) << (\d+);", _f.read())
    SLAB_CELLS = int(_m.group(1)) << int(_m.group(2))  # (row, bin) cells per slab of the host forms of the span, zoom and bed summaries
INT32_MAX = 2 ** 31 - 1


def assert_planes(got, want, what):
    for name, g, w in zip(M.PLANES, got, want):
        g = np.asarray(g)
        assert g.dtype == np.float64 and g.shape == np.asarray(w).shape, (what, name, g.shape)
        if not M.same_bits(g, w):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), [float(g[tuple(b)]) for b in bad[:4]], [float(w[tuple(b)]) for b in bad[:4]]))


def empty_planes(size):
    return np.array(M.empty_row(size))


def random_track(rng, n_items, ordered=True):
    """items of 1-40 bases, touching or a little apart (ordered) or overlapping and shuffled (not); values over a wide range"""
    lengths = rng.integers(1, 41, size=n_items)
    gaps = np.where(rng.random(n_items) < 0.3, rng.integers(0, 30, size=n_items), 0)
    starts = np.cumsum(lengths + gaps) - lengths
    values = (rng.standard_normal(n_items) * np.exp2(rng.integers(-12, 13, size=n_items))).astype(np.float32)
    values[rng.random(n_items) < 0.01] = np.nan
    if not ordered:
        starts = starts - rng.integers(0, 25, size=n_items)
        starts[starts < 0] = 0
        lengths = lengths + rng.integers(0, 60, size=n_items)
        perm = rng.permutation(n_items)
        starts, lengths, values = starts[perm], lengths[perm], values[perm]
    return starts.astype(np.int32), (starts + lengths).astype(np.int32), values


def chunk_track():
    """items [3 k, 3 k + 3): the region [3 a, 3 (a + r)) meets exactly r of them"""
    k = np.arange(4 * CHUNK + 128, dtype=np.int32)
    values = (np.sin(k.astype(np.float64)) * 3.0).astype(np.float32)
    return 3 * k, 3 * k + 3, values


_diff = {}


def differential_case(size):
    """(host tracks, track_of, starts, ends, the model's answer), once per size"""
    if size not in _diff:
        rng = np.random.default_rng(100 + size)
        tracks = [random_track(rng, 5000), random_track(rng, 1200), random_track(rng, 300, ordered=False), chunk_track(),
                  (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))]
        n = 1200
        track_of = rng.integers(-1, 5, size=n)
        reach = np.array([int(t[1].max()) if len(t[1]) else 100 for t in tracks] + [100])[track_of]
        starts = (rng.random(n) * (reach + 50)).astype(np.int64)
        widths = np.where(rng.random(n) < 0.5, rng.integers(1, 4 * size + 2, size=n), rng.integers(1, 6000, size=n))
        widths[:8] = (size, size - 1 if size > 1 else 1, size + 1, 2 * size + 1, 1, 64 * size, 65 * size + 3, 63 * size)
        ends = starts + widths
        ends[8:12] = starts[8:12] - np.array([0, 1, 5, 0])  # start >= end: empty rows
        # the chunk track (index 3): runs of CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 7 items from an odd offset, and 2 CHUNK items,
        # which with size == 2 puts all the items of bin 1 into the second chunk
        runs = [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 2 * CHUNK]
        extra_start = np.array([3 * 5] * len(runs))
        extra_end = extra_start + 3 * np.array(runs)
        track_of = np.concatenate([track_of, [3] * len(runs), [0, 0]]).astype(np.int32)
        starts = np.concatenate([starts, extra_start, [0, 2 ** 31 - 2 - 4 * size]]).astype(np.int32)
        ends = np.concatenate([ends, extra_end, [int(tracks[0][1].max()), 2 ** 31 - 1]]).astype(np.int32)
        _diff[size] = (tracks, track_of, starts, ends, M.summarize(tracks, track_of, starts, ends, size))
    return _diff[size]


# ------------------------------------------------------------ records that end at 2^31 - 1 --
def shifted_to_the_top(ends, *others):
    """int32 copies of the coordinate arrays, all shifted (in int64) by one amount, so that the largest of `ends` is 2^31 - 1"""
    shift = INT32_MAX - int(np.max(ends))
    out = [(np.asarray(a, dtype=np.int64) + shift) for a in (ends,) + others]
    assert all(a.min() >= 0 and a.max() <= INT32_MAX for a in out if len(a))
    return [a.astype(np.int32) for a in out]


def top_regions(rng, first_starts, size):
    """(track_of, starts, ends) over tracks whose last record ends at 2^31 - 1 and whose first starts at first_starts[t]: 60 seeded
    regions inside the last 100000 bases -- one in three ends at 2^31 - 1, one in three starts in the last 2000 bases -- and on every
    track [first start, 2^31 - 1), [2^31 - 2, 2^31 - 1) and [2^31 - 1 - 700, 2^31 - 1)"""
    n = 60
    track_of = rng.integers(0, len(first_starts), size=n)
    starts = INT32_MAX - np.where(np.arange(n) % 3 == 1, rng.integers(1, 2000, size=n), rng.integers(1, 100000, size=n))
    widths = np.where(rng.random(n) < 0.5, rng.integers(1, 4 * size + 2, size=n), rng.integers(1, 9000, size=n))
    ends = np.minimum(starts + widths, INT32_MAX)
    ends[np.arange(n) % 3 == 0] = INT32_MAX
    fixed = [(t, a, INT32_MAX) for t, first in enumerate(first_starts) for a in (int(first), INT32_MAX - 1, INT32_MAX - 700)]
    track_of = np.concatenate([track_of, [r[0] for r in fixed]]).astype(np.int32)
    starts = np.concatenate([starts, [r[1] for r in fixed]]).astype(np.int32)
    ends = np.concatenate([ends, [r[2] for r in fixed]]).astype(np.int32)
    assert (starts < ends).all() and (ends == INT32_MAX).sum() >= 20 + len(fixed)
    return track_of, starts, ends


_top = {}
TOP_SIZES = (1, 3, 65)


def top_case(size):
    """(host tracks, track_of, starts, ends, the model's answer), once per size: an ordered and an unordered track of 3000 items,
    each shifted so that its last end is exactly 2^31 - 1, under top_regions()"""
    if size not in _top:
        rng = np.random.default_rng(500 + size)
        tracks = []
        for ordered in (True, False):
            s, e, v = random_track(rng, 3000, ordered=ordered)
            e, s = shifted_to_the_top(e, s)
            tracks.append((s, e, v))
        assert all(int(t[1].max()) == INT32_MAX for t in tracks)
        track_of, starts, ends = top_regions(rng, [t[0].min() for t in tracks], size)
        _top[size] = (tracks, track_of, starts, ends, M.summarize(tracks, track_of, starts, ends, size))
    return _top[size]


# ------------------------------------------------------------ more than one slab of the host form --
SLAB_SIZE = 3000  # bins per row: does not divide SLAB_CELLS, so a slab's last row ends short of it


def slab_batch(seed, n_full, reaches):
    """(slab, track_of, starts, ends): n_full * slab + 5 rows of SLAB_SIZE bins, slab = SLAB_CELLS // SLAB_SIZE rows -- n_full full
    slabs of the host form and a short one.  Regions of 3000 to 12000 bases over two tracks that end at reaches[0], reaches[1]; one
    row in ten has no track (-1), but none of the six rows around a slab edge, which lie on one track at starts 37 bases apart"""
    assert SLAB_CELLS % SLAB_SIZE != 0
    slab = SLAB_CELLS // SLAB_SIZE
    n = n_full * slab + 5
    rng = np.random.default_rng(seed)
    track_of = rng.integers(0, 2, size=n)
    widths = rng.integers(3000, 12001, size=n)
    starts = (rng.random(n) * np.maximum(np.asarray(reaches)[track_of] - widths, 1)).astype(np.int64)
    track_of[rng.random(n) < 0.1] = -1
    for first in range(slab, n, slab):
        around = np.arange(first - 3, first + 3)
        track_of[around] = (first // slab) % 2
        starts[around] = 1000 + 37 * np.arange(6) + 500 * (first // slab)
    return slab, track_of.astype(np.int32), starts.astype(np.int32), (starts + widths).astype(np.int32)


def assert_slabs(host, device, model, slab, n):
    """host, device: the five [n, SLAB_SIZE] planes of the host form and of the device form; model(rows): the model's planes of
    those rows.  The six rows around every slab edge differ pairwise in the model's sum_data, so a slab copied back one row off
    shows; the host form equals the device form in every cell; rows 0, n - 1, those six and every 97th are the model's"""
    edges = list(range(slab, n, slab))
    assert len(edges) >= 1 and n % slab == 5 and all(p.shape == (n, SLAB_SIZE) for p in host)
    rows = sorted(set([0, n - 1] + [r for first in edges for r in range(first - 3, first + 3)] + list(range(0, n, 97))))
    want = model(np.array(rows))
    for first in edges:
        around = [want[3][rows.index(r)].tobytes() for r in range(first - 3, first + 3)]
        assert len(set(around)) == 6, ("the rows around the slab edge are not all different", first)
    assert_planes(host, device, "the host form against the device form")
    assert_planes([p[rows] for p in host], want, "the host form against the model")
