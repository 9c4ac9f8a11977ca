"""
Seeded inputs for the score tracks at batch scale and at their structural edges: what tests/test_gpu_scores_scale.py sends to
the device and tests/test_scores_cases.py checks for the conditions that keep those tests from passing vacuously (a helper: no
tests here, no GPU).

A large batch is `pool[idx]`: at most MAX_UNIQUE different intervals, so that tests/scores_model.py answers the pool once and
the expectation of a batch of millions is `answer[idx]`.  `tiled` makes every pool interval appear at least once.

Thresholds that depend on the device are written in terms of `cap` = compute units x 8, the bound of the library's grid-stride
grids (csrc/common.hpp: stream_grid); the GPU tests pass the device's, the CPU tests CAP_MI355X.
"""
import numpy as np

from test_gpu_scores import random_intervals, random_track

MAX_UNIQUE = 4096
CAP_MI355X = 256 * 8
SIZE = 70_003                                                   # the shared track: more than 65 000 + 64 bases, odd
INF_BAND = (30_000, 33_000)
SCATTER_NS = (1023, 1024, 1025, 2047, 2048, 2049, 4097, 70_001)  # around the count's 1024 and the scatter's 2048 per workgroup
KNOB_EDGES = (64, 128, 8192)                                    # scores.wave_min_len values whose L-1, L, L+1 the edge case holds
HANDLE_NS = (5000, 3, 70_001, 1, 2049, 0, 64)                   # one handle answers these in this order
MASK_SIZES = (1, 63, 64, 65, 127, 128, 129, 199, 200, 4097)
GEOMETRY_SIZE = 200


def tiled(rng, n_pool, n):
    """idx of a batch of n rows over the first min(n, n_pool) pool intervals: each of them once, in random order, then draws"""
    u = min(n, n_pool)
    return np.concatenate([rng.permutation(u), rng.integers(0, max(u, 1), n - u)]).astype(np.int64)


def runs_mask(rng, size, n_runs, max_run=300):
    m = np.zeros(size, dtype=bool)
    for a in rng.integers(0, max(size - max_run, 1), n_runs):
        m[a:a + int(rng.integers(1, max_run))] = True
    return m


_world = {}


def world():
    """the shared track (random_track plus +-inf), a mask shorter than it, one longer than it with other runs, a pool of
    intervals of up to 600 bases and one of up to 130 -- both with the empty, inverted, far-left and far-right ones of
    random_intervals -- made once and never changed.  The twelve +inf and twelve -inf lie in INF_BAND: an interval that reaches
    from a far end over the whole band sums to NaN whatever the order, and all over the track that would be most long ones.
    `dense` is the track of the 130-base pool: one magnitude and few gaps, so that sums of a few dozen scores depend on their
    order (among the three magnitudes of random_track the largest one alone decides most short sums)."""
    if not _world:
        rng = np.random.default_rng(101)
        track = random_track(rng, SIZE)
        at = INF_BAND[0] + rng.permutation(INF_BAND[1] - INF_BAND[0])[:24]
        track[at[:12]], track[at[12:]] = np.inf, -np.inf
        dense = (rng.standard_normal(SIZE) * 100).astype(np.float32)
        kind = rng.random(SIZE)
        dense[kind < 0.05] = np.nan
        dense[(kind >= 0.05) & (kind < 0.07)] = 0.0
        mask = runs_mask(rng, SIZE - 4321, 200)
        mask[64:128] = True
        mask[191:257] = True
        mask_b = runs_mask(rng, SIZE + 501, 150, max_run=90)
        s, e = random_intervals(rng, SIZE, MAX_UNIQUE)
        ss, se = random_intervals(rng, SIZE, MAX_UNIQUE, max_len=130)
        for a in (track, dense, mask, mask_b, s, e, ss, se):
            a.setflags(write=False)
        _world.update(size=SIZE, track=track, dense=dense, mask=mask, mask_b=mask_b, s=s, e=e, short_s=ss, short_e=se)
    return _world


def scatter_batches():
    """{n: idx into the 600-base pool} for n in SCATTER_NS"""
    rng = np.random.default_rng(102)
    return {n: tiled(rng, MAX_UNIQUE, n) for n in SCATTER_NS}


def count_stride_n(cap=CAP_MI355X):
    return cap * 1024 + 3       # the count kernel's grid is capped at `cap` workgroups of 1024 intervals: beyond, it strides


def count_stride_batch(cap=CAP_MI355X):
    """idx into the 130-base pool"""
    return tiled(np.random.default_rng(103), MAX_UNIQUE, count_stride_n(cap))


def wave_stride_ns(cap=CAP_MI355X):
    """with the knob at 0 every interval takes a wave: the first n gives each of the cap * 4 waves two trips and five of them a
    third, the others leave the last workgroup of four waves with one, two or three of them busy (and the one before full)"""
    return (cap * 4 * 2 + 5, 5, 6, 7, 9, 10, 11)


def wave_stride_batches(cap=CAP_MI355X):
    """{n: idx into the 130-base pool}"""
    rng = np.random.default_rng(104)
    return {n: tiled(rng, MAX_UNIQUE, n) for n in wave_stride_ns(cap)}


def edge_lengths():
    """clipped lengths around the steps of sc_bucket (64 bases each, the 511th and beyond in one bucket) and around the knobs"""
    lens = {0, 1, 63, 64, 65, 127, 128, 129, 65_000, 65_001, SIZE}
    lens |= {k * 64 + d for k in (509, 510, 511, 512) for d in (-1, 0, 1)}
    lens |= {L + d for L in KNOB_EDGES for d in (-1, 0, 1)}
    return sorted(lens)


def bucket_edge_case():
    """(starts, ends) for a track of SIZE bases (the tests use `dense`: nearly every long interval of the shared track crosses
    INF_BAND): every length of edge_lengths at the track's start, at its end, twice inside it, and
    hanging over either end so that the raw length is larger than the clipped one (for a clipped length of L - 1 the raw one is
    at least L); shuffled among 300 rows of under 100 bases so long and short rows share waves"""
    rng = np.random.default_rng(105)
    s, e = [], []
    for ln in edge_lengths():
        for a in (0, SIZE - ln, int(rng.integers(0, SIZE - ln + 1)), int(rng.integers(0, SIZE - ln + 1))):
            s.append(a)
            e.append(a + ln)
        s += [-7, SIZE - ln]
        e += [ln, SIZE + 9]
    ps = rng.integers(-50, SIZE, 300)
    s, e = np.concatenate([s, ps]), np.concatenate([e, ps + rng.integers(0, 100, 300)])
    p = rng.permutation(len(s))
    return s[p].astype(np.int64), e[p].astype(np.int64)


def clipped_lengths(s, e, size=SIZE):
    return np.maximum(np.minimum(e, size) - np.maximum(s, 0), 0)


ONE_BUCKET_N, ONE_BUCKET_LEN = 70_001, 200


def one_bucket_case():
    """(pool starts, pool ends, idx): ONE_BUCKET_N intervals of ONE_BUCKET_LEN bases inside the track, so one bucket holds all"""
    rng = np.random.default_rng(106)
    s = rng.integers(0, SIZE - ONE_BUCKET_LEN + 1, MAX_UNIQUE).astype(np.int64)
    return s, s + ONE_BUCKET_LEN, tiled(rng, MAX_UNIQUE, ONE_BUCKET_N)


def handle_sequence():
    """[(n, idx into the 600-base pool, knob, mask name or None)] for the batches one handle answers one after the other: the
    knob changes before each, the mask alternates between present and absent and between two masks"""
    from test_gpu_scores import HUGE

    rng = np.random.default_rng(107)
    knobs = (HUGE, 0, 128, None, HUGE, 0, 128)
    masks = ("mask", None, "mask_b", None, "mask", None, "mask_b")
    return [(n, tiled(rng, MAX_UNIQUE, n), k, m) for n, k, m in zip(HANDLE_NS, knobs, masks)]


def geometry_track():
    """GEOMETRY_SIZE bases, a score on every one of them: the mask alone decides what counts"""
    rng = np.random.default_rng(108)
    v = (rng.standard_normal(GEOMETRY_SIZE) * rng.choice(np.array([1e-3, 1.0, 1e4]), size=GEOMETRY_SIZE)).astype(np.float32)
    v[v == 0] = np.float32(1.5)
    return v


def geometry_mask(size):
    """a mask of `size` bits with its first, its last and a middle run set"""
    m = np.zeros(size, dtype=bool)
    m[:min(3, size)] = True
    m[size - min(2, size):] = True
    m[size // 2:size // 2 + max(1, size // 7)] = True
    return m


def all_intervals(size=GEOMETRY_SIZE):
    """every 0 <= s <= e <= size"""
    s, e = np.triu_indices(size + 1)
    return s.astype(np.int64), e.astype(np.int64)


SUBNORMAL_SEGMENTS = {"A": dict(seed=109, exp=(-145, -123), max_len=399), "B": dict(seed=110, exp=(-149, -132), max_len=39)}


def subnormal_segment(which):
    """(track, starts, ends): scores ldexp(N(0, 1), U{exp}), a tenth of them NaN; 2000 intervals of 1 .. max_len bases"""
    spec = SUBNORMAL_SEGMENTS[which]
    rng = np.random.default_rng(spec["seed"])
    size = 20_011
    track = np.ldexp(rng.standard_normal(size), rng.integers(spec["exp"][0], spec["exp"][1] + 1, size)).astype(np.float32)
    track[rng.random(size) < 0.1] = np.nan
    s = rng.integers(0, size - 1, 2000)
    e = s + rng.integers(1, spec["max_len"] + 1, 2000)
    return track, s.astype(np.int64), e.astype(np.int64)


def is_subnormal(a):
    a = np.asarray(a, dtype=np.float32)
    return (a != 0) & (np.abs(a) < np.finfo(np.float32).tiny)


def fill_run_n(cap=CAP_MI355X):
    return cap * 256 + 7        # sc_fill_kernel's grid is capped at `cap` workgroups of 256 spans: beyond, it strides


def fill_case(cap=CAP_MI355X):
    """(size, starts, ends, values): one ascending, disjoint run of fill_run_n(cap) spans of 0 .. 3 bases, every 1000th one
    64 .. 900 wide (the whole wave stores those), the first one hanging over the track's start and the last ones over its end;
    then 50 descending spans and 50 that each overlap the one before"""
    rng = np.random.default_rng(111)
    m = fill_run_n(cap)
    ln = rng.integers(0, 4, m)
    ln[::1000] = rng.integers(64, 901, len(ln[::1000]))
    gap = rng.integers(0, 3, m)
    s = np.cumsum(gap + np.concatenate([[0], ln[:-1]])) - 5
    e = s + ln
    size = int(e[-1]) - 11
    ds = size // 2 - 40 * np.arange(50)
    os_ = size // 3 + 5 * np.arange(50)
    s = np.concatenate([s, ds, os_])
    e = np.concatenate([e, ds + 30, os_ + 70])
    v = rng.standard_normal(len(s)).astype(np.float32)
    v[::7] = np.nan
    v[3::50] = 0.0
    return size, s.astype(np.int64), e.astype(np.int64), v


def fill_intervals(size, n=2049):
    """random_intervals; beyond the first 300 rows an interval ends at most 600 bases into the track from its start (the model
    walks every base, and an interval to a far end of this track is 780 k bases long on average)"""
    s, e = random_intervals(np.random.default_rng(112), size, n)
    k = np.arange(n) >= 300
    e[k] = np.minimum(e[k], np.maximum(s[k], 0) + 600)
    return s, e
