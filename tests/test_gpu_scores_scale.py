"""
Score aggregation (bxmi_scores_*, csrc/scores.hpp) at batch scale and at its structural edges, against tests/scores_model.py
bit for bit as tests/test_gpu_scores.py compares: counts as int32, sums / minima / maxima as uint32 views.  The inputs come from
tests/scores_cases.py; tests/test_scores_cases.py pins, on the model alone, what keeps these tests from passing vacuously.

A batch of millions is `pool[idx]` over at most 4096 different intervals: the model answers the pool once and the expectation
is `answer[idx]`.  No expected value comes from the device.  Where a threshold depends on the device it is computed from the
compute units bxmi_device_info reports: cap = CUs x 8 bounds every grid-stride grid of the library (csrc/common.hpp).

  piece of scores.hpp / scores.hip                     crossed by
  sc_bucket_scatter_kernel, 2048 intervals a workgroup  n = 2047 .. 2049, 4097, 70 001                       (edges, one bucket, dev)
  sc_bucket_count_kernel, 1024 a workgroup, cap of them n = 1023 .. 1025; n = cap * 1024 + 3                 (edges, count stride)
  sc_wave_kernel, 4 waves a workgroup, cap of them      knob 0 and n = cap * 8 + 5, n = 4k + 1 .. 3; 20 301  (wave stride, geometry)
  sc_fill_kernel, 256 spans a workgroup, cap of them    one run of cap * 256 + 7 spans                       (fill)
  sc_bucket, 512 buckets of 64-base steps               clipped lengths around k * 64 and 509 .. 512 steps   (bucket edges)
  len >= wave_min_len on the clipped length             knobs 64, 128, 8192 with L - 1, L, L + 1             (bucket edges)
  the handle's scratch                                  seven batches and two masks through one handle       (one handle)
  sc_mask_bits                                          ten mask sizes, inverted too, every start and end    (geometry)
  subnormals kept                                       two tracks of subnormal scores and sums              (subnormals)
"""
import ctypes as C

import numpy as np
import pytest

import scores_cases as SC
import scores_model as M
from test_gpu_scores import HUGE, KNOBS, assert_same, bits, device_mask, device_track, set_knob

pytestmark = pytest.mark.gpu

# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_scores_aggregate_dev",)


@pytest.fixture(autouse=True)
def _knob_back():
    yield
    set_knob(None)


@pytest.fixture(scope="module")
def cap():
    """compute units x 8 of the device the library runs on"""
    from bxmi import _ffi

    dev, cus = C.c_int(0), C.c_int(0)
    _ffi.call("bxmi_get_device", C.byref(dev))
    _ffi.call("bxmi_device_info", dev.value, None, 0, C.byref(cus), None)
    assert cus.value > 0
    return cus.value * 8


@pytest.fixture(scope="module")
def W():
    return SC.world()


_answers = {}


def answer(W, track, pool, mask=None):
    """the model's answer for a whole pool of the shared world, computed once and left unchanged"""
    key = (track, pool, mask)
    if key not in _answers:
        s, e = (W["s"], W["e"]) if pool == "long" else (W["short_s"], W["short_e"])
        _answers[key] = M.aggregate(W[track], s, e, W[mask] if mask else None)
        for a in _answers[key]:
            a.setflags(write=False)
    return _answers[key]


def take(ans, idx):
    return [a[idx] for a in ans]


# ---------------------------------------------------- a. workgroup edges --
_scatter = {}


def scatter_idx(n):
    if not _scatter:
        _scatter.update(SC.scatter_batches())
    return _scatter[n]


@pytest.mark.parametrize("n", SC.SCATTER_NS)
def test_scatter_and_count_workgroup_edges(W, n):
    """one, two, three and 35 workgroups of the scatter (2048 intervals each), the last one full, one short of full and holding a
    single interval; one and two of the count (1024): all rows, a mix of both paths, the default; with and without the mask"""
    idx = scatter_idx(n)
    s, e = W["s"][idx], W["e"][idx]
    t, dm = device_track(W["track"]), device_mask(W["mask"])
    for knob in (HUGE, 128, None):
        set_knob(knob)
        assert_same(t.aggregate(s, e), take(answer(W, "track", "long"), idx), (n, knob, "plain"))
        assert_same(t.aggregate(s, e, mask=dm), take(answer(W, "track", "long", "mask"), idx), (n, knob, "masked"))
    t.close()


# ------------------------------------------------------- b. count stride --
def test_count_kernel_strides_over_a_batch_of_millions(W, cap):
    """more intervals than the count kernel's capped grid takes in one trip (cap workgroups x 1024): every workgroup comes back for
    more, the last trip is three intervals long.  2.1 M rows on an MI355X, 1025 workgroups of the scatter.  The intervals are drawn
    under 130 bases; the seventh of them that random_intervals stretches to a far end is as long as the track allows, so every
    bucket is in use (both passes and their comparison take 0.2 s on an MI355X all the same)"""
    n = SC.count_stride_n(cap)
    assert n > cap * 1024
    idx = SC.count_stride_batch(cap)
    s, e = W["short_s"][idx], W["short_e"][idx]
    want = take(answer(W, "dense", "short"), idx)
    t = device_track(W["dense"])
    for knob in (HUGE, 128):
        set_knob(knob)
        assert_same(t.aggregate(s, e), want, (n, knob))
    t.close()


# -------------------------------------------------------- c. wave stride --
def test_wave_kernel_strides_and_partial_last_block(W, cap):
    """knob 0: long_list holds every interval, empty and inverted ones too.  cap * 4 waves share cap * 8 + 5 intervals (two trips
    each, a third for five of them); then batches that leave the last workgroup's four waves partly idle"""
    ns = SC.wave_stride_ns(cap)
    assert ns[0] > cap * 4 * 2 and {n % 4 for n in ns[1:]} == {1, 2, 3}
    batches = SC.wave_stride_batches(cap)
    t = device_track(W["dense"])
    set_knob(0)
    for n in ns:
        idx = batches[n]
        assert len(idx) == n
        assert_same(t.aggregate(W["short_s"][idx], W["short_e"][idx]), take(answer(W, "dense", "short"), idx), n)
    t.close()


# ----------------------------------------------- d. bucket and knob edges --
@pytest.fixture(scope="module")
def edge_case(W):
    s, e = SC.bucket_edge_case()
    return s, e, M.aggregate(W["dense"], s, e), M.aggregate(W["dense"], s, e, W["mask"])


@pytest.mark.parametrize("knob", [HUGE, 0] + list(SC.KNOB_EDGES))
def test_bucket_and_knob_edges(W, edge_case, knob):
    """clipped lengths on either side of every 64-base step sc_bucket tells apart, of the step from which all share a bucket, and
    of the knob; raw lengths that reach the knob where the clipped ones do not, at both ends of the track"""
    s, e, plain, masked = edge_case
    t, dm = device_track(W["dense"]), device_mask(W["mask"])
    set_knob(knob)
    assert_same(t.aggregate(s, e), plain, (knob, "plain"))
    assert_same(t.aggregate(s, e, mask=dm), masked, (knob, "masked"))
    t.close()


# ------------------------------------------------------ e. one hot bucket --
def test_all_intervals_in_one_bucket(W):
    """70 001 intervals of one length: every LDS histogram has one hot bin, all 35 workgroups of the scatter queue at one cursor;
    then as many empty ones (the last bucket)"""
    ps, pe, idx = SC.one_bucket_case()
    want = take(M.aggregate(W["track"], ps, pe), idx)
    t = device_track(W["track"])
    for knob in (HUGE, None):
        set_knob(knob)
        assert_same(t.aggregate(ps[idx], pe[idx]), want, ("one length", knob))
    n = SC.ONE_BUCKET_N
    got = t.aggregate(ps[idx], ps[idx] - (idx % 3))
    assert_same(got, (np.zeros(n, np.int32), np.zeros(n, np.float32), np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)), "empty")
    t.close()


# ------------------------------------------- f. one handle, many batches --
def test_one_handle_answers_many_batches(W):
    """the handle's long_list, order, counters and staging serve a large batch, then a small one, then a larger one ...; the knob
    moves between them and two masks come and go.  A track made afterwards answers the first batch again"""
    t = device_track(W["track"])
    masks = {"mask": device_mask(W["mask"]), "mask_b": device_mask(W["mask_b"], granularity=64)}
    seq = SC.handle_sequence()
    assert [n for n, _, _, _ in seq] == list(SC.HANDLE_NS)
    for n, idx, knob, mask in seq:
        set_knob(knob)
        got = t.aggregate(W["s"][idx], W["e"][idx], mask=masks.get(mask))
        assert all(len(a) == n for a in got)
        assert_same(got, take(answer(W, "track", "long", mask), idx), (n, knob, mask))
    n, idx, knob, mask = seq[0]
    t2 = device_track(W["track"])
    set_knob(knob)
    for track in (t2, t):
        assert_same(track.aggregate(W["s"][idx], W["e"][idx], mask=masks[mask]), take(answer(W, "track", "long", mask), idx), ("again", track is t))
    t.close()
    t2.close()


# ------------------------------------------------------ g. mask geometry --
FLAT_MASK_SIZE = 129


@pytest.mark.parametrize("size", SC.MASK_SIZES)
def test_mask_geometry_exhaustive(size):
    """every interval of a 200-base track against masks that end inside their first word, at a word's end and one bit into the
    next, shorter and longer than the track: a mask with its first, last and a middle run set, and its inversion on the device
    (which sets the bits beyond the size in the last word)"""
    from bxmi.bitset import DeviceBitSet

    track = SC.geometry_track()
    s, e = SC.all_intervals()
    m = SC.geometry_mask(size)
    if size == FLAT_MASK_SIZE:
        dm = DeviceBitSet(size, flat=True)
        edges = np.flatnonzero(np.diff(np.concatenate(([0], m.astype(np.int8), [0]))))
        dm.set_ranges(edges[0::2].astype(np.int32), (edges[1::2] - edges[0::2]).astype(np.int32))
    else:
        dm = device_mask(m, granularity=16)
    t = device_track(track)
    for model_mask, what in ((m, "mask"), (~m, "inverted")):
        if what == "inverted":
            dm.invert()
        want = M.aggregate(track, s, e, model_mask)
        for knob in (HUGE, 0):
            set_knob(knob)
            assert_same(t.aggregate(s, e, mask=dm), want, (size, what, knob))
    t.close()


# --------------------------------------------------------- h. subnormals --
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("segment", sorted(SC.SUBNORMAL_SEGMENTS))
def test_subnormal_scores_and_sums(segment, knob):
    """scores below 2^-126 count and add up (A: flushed to zero they would change nearly every count and sum); sums that stay
    subnormal (B).  The chain's "+0.0f is an identity" needs both"""
    track, s, e = SC.subnormal_segment(segment)
    t = device_track(track)
    set_knob(knob)
    assert_same(t.aggregate(s, e), M.aggregate(track, s, e), (segment, knob))
    t.close()


# ------------------------------------------------------ i. fill at scale --
def test_fill_strides_over_a_long_run(cap):
    """one ascending run of more spans than the fill kernel's capped grid takes in one trip (cap workgroups x 256), wide spans
    among the short ones, then a launch per span for descending and overlapping ones, all in one call; the track then serves"""
    from bxmi.scores import ScoreTrack

    size, s, e, v = SC.fill_case(cap)
    assert SC.fill_run_n(cap) > cap * 256 and len(s) == SC.fill_run_n(cap) + 100
    t = ScoreTrack(size)
    t.set_spans(s, e, v)
    want = M.fill(size, s, e, v)
    got = t.read()
    bad = np.flatnonzero(bits(got) != bits(want))
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:4]], want[bad[:4]])
    qs, qe = SC.fill_intervals(size)
    assert len(qs) == 2049
    assert_same(t.aggregate(qs, qe), M.aggregate(want, qs, qe), "after the fill")
    t.close()


# ------------------------------------------------ j. the device entry point --
@pytest.mark.parametrize("n", [2049, 70_001])
def test_aggregate_dev_at_scale_with_guarded_buffers(W, n):
    """bxmi_scores_aggregate_dev as tests/test_gpu_scores.py drives it at n = 1000, past one and past many workgroups of the
    ordering: caller-owned buffers of 4-byte alignment between guard bytes, a caller's non-blocking stream"""
    from bxmi import _ffi
    from test_gpu_device_entry_points import Guarded, Stream

    idx = scatter_idx(n)
    s32, e32 = _ffi.as_i32(np.clip(W["s"][idx], -(2**31), 2**31 - 1)), _ffi.as_i32(np.clip(W["e"][idx], -(2**31), 2**31 - 1))
    t, dm = device_track(W["track"]), device_mask(W["mask"])
    st = Stream()
    try:
        for knob, mask, pool_mask in ((128, None, None), (None, dm, "mask"), (HUGE, dm, "mask")):
            set_knob(knob)
            src_s, src_e = Guarded.holding(s32), Guarded.holding(e32)
            ds, de = Guarded(n * 4, mis=4), Guarded(n * 4, mis=12)
            outs = [Guarded(n * 4, mis=m) for m in (4, 8, 12, 0)]
            st.copy_d2d(ds.ptr, src_s.ptr, n * 4)
            st.copy_d2d(de.ptr, src_e.ptr, n * 4)
            t.aggregate_ptrs(mask, ds.ptr, de.ptr, n, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, stream=st.s)
            st.sync()
            got = []
            for g, dt, name in zip(outs, (np.int32, np.float32, np.float32, np.float32), ("count", "sum", "min", "max")):
                got.append(g.payload(g.check(n * 4, name), dt, n))
            assert_same(got, take(answer(W, "track", "long", pool_mask), idx), ("dev", n, knob, pool_mask))
            for g, a in ((ds, s32), (de, e32)):
                assert np.array_equal(g.payload(g.check(n * 4, "input"), np.int32, n), a)
    finally:
        st.close()
        t.close()
