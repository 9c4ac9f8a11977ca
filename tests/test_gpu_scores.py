"""
Score tracks on the device (bxmi_scores_*, bxmi.scores.ScoreTrack, bxmi.cli.aggregate_scores_in_intervals) against the
reference's recorded answers (tests/golden/scores; tests/test_scores_model_golden.py pins the same files to the model) and, on
fresh inputs and on the edges the recorded cases lack, against tests/scores_model.py.  Every comparison is bit-exact: counts as
integers, sums / minima / maxima as uint32 views of the float32 results.

Both kernels are forced onto every case through `scores.wave_min_len`: 0 (a wave per interval), a huge value (64 intervals per
wave), 128 (both inside one batch) and the default.  "bxmi_scores_aggregate_dev" is driven as a caller outside the suite would:
guarded caller-owned buffers, a non-blocking stream of the caller's (the helpers of tests/test_gpu_device_entry_points.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scores_model as M
from test_scores_model_golden import GOLDEN, MANIFEST, golden_lines, model_tracks, recorded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points of the score tracks this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_scores_values_dev", "bxmi_scores_aggregate_dev")
HUGE = 1 << 40
KNOBS = [None, 0, HUGE, 128]  # None = the library's default


def _ffi():
    from bxmi import _ffi

    return _ffi


def _default_knob():
    return _ffi().options()["scores.wave_min_len"]


DEFAULT_KNOB = _default_knob()


def set_knob(v):
    _ffi().call("bxmi_set_option", b"scores.wave_min_len", DEFAULT_KNOB if v is None else int(v))


@pytest.fixture(autouse=True)
def _knob_back():
    yield
    set_knob(None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    """got: Aggregate (or a 4-tuple of arrays); want: the model's 4-tuple"""
    for name, g, w in zip(("count", "total", "minimum", "maximum"), got, want):
        if name == "count":
            assert np.asarray(g).dtype == np.int32 and np.array_equal(g, w), (what, name, np.nonzero(np.asarray(g) != w)[0][:8])
        else:
            bad = np.nonzero(bits(g) != bits(w))[0]
            assert len(bad) == 0, (what, name, bad[:8], np.asarray(g)[bad[:4]], np.asarray(w)[bad[:4]])


def device_track(values):
    from bxmi.scores import ScoreTrack

    t = ScoreTrack(len(values))
    t.write(0, values)
    return t


def device_mask(model_mask, size=None, granularity=1024):
    """a DeviceBitSet holding a model mask (bool array)"""
    from bxmi.bitset import DeviceBitSet

    size = len(model_mask) if size is None else size
    d = DeviceBitSet(size, granularity)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], model_mask.astype(np.int8), [0]))))
    if len(edges):
        d.set_ranges(edges[0::2].astype(np.int32), (edges[1::2] - edges[0::2]).astype(np.int32))
    return d


# ------------------------------------------------------------ recorded cases --
_expect = {}


def case_batches(k):
    """per chromosome with scores of recorded case k: (model track, model mask or None, starts, ends, the model's answer), once"""
    if k not in _expect:
        case = MANIFEST[k]
        tracks = model_tracks(case["scores"])
        masks = M.load_mask(golden_lines(case["mask"])) if case["mask"] else {}
        rows = [line.split() for line in golden_lines(case["intervals"])]
        out = {}
        for chrom, track in tracks.items():
            s = np.array([int(r[1]) for r in rows if r[0] == chrom], dtype=np.int64)
            e = np.array([int(r[2]) for r in rows if r[0] == chrom], dtype=np.int64)
            out[chrom] = (track, masks.get(chrom), s, e, M.aggregate(track, s, e, masks.get(chrom)))
        _expect[k] = out
    return _expect[k]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("k", range(4))
def test_recorded_cases(k, knob):
    """the wiggle fixture through bxmi.wiggle + set_spans, every interval of the case in one aggregate call per chromosome"""
    from bxmi import wiggle
    from bxmi.scores import ScoreTrack, format_row

    case = MANIFEST[k]
    spans = wiggle.read_spans_file(os.path.join(GOLDEN, case["scores"]))
    set_knob(knob)
    lines = {}
    rows = [line.split() for line in golden_lines(case["intervals"])]
    for chrom, (track, mask, s, e, want) in case_batches(k).items():
        ss, se, sv = spans[chrom]
        t = ScoreTrack(int(se.max()))
        t.set_spans(ss, se, sv)
        assert np.array_equal(bits(t.read()), bits(track)), chrom
        dm = device_mask(mask, len(mask) + 77) if mask is not None else None
        got = t.aggregate(s, e, mask=dm)
        assert_same(got, want, (case["expected"], chrom, knob))
        mine = [i for i, r in enumerate(rows) if r[0] == chrom]
        for j, i in enumerate(mine):
            lines[i] = format_row(chrom, int(s[j]), int(e[j]), int(got.count[j]), got.total[j], got.minimum[j], got.maximum[j])
        t.close()
    for i, r in enumerate(rows):
        lines.setdefault(i, format_row(r[0], int(r[1]), int(r[2]), 0, 0.0, 0.0, 0.0))
    assert [lines[i] for i in range(len(rows))] == recorded(case).split("\n")[:-1]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("k", range(4))
def test_command_line_prints_the_recorded_text(k, knob, tmp_path):
    """python -m bxmi.cli.aggregate_scores_in_intervals in a fresh process; the knob through BXMI_OPTS; the out_file argument"""
    case = MANIFEST[k]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    if knob is not None:
        env["BXMI_OPTS"] = "scores.wave_min_len=%d" % knob
    cmd = [sys.executable, "-m", "bxmi.cli.aggregate_scores_in_intervals", os.path.join(GOLDEN, case["scores"]), os.path.join(GOLDEN, case["intervals"])]
    to_file = knob == 128
    if to_file:
        cmd.append(str(tmp_path / "out.txt"))
    if case["mask"]:
        cmd += ["-m", os.path.join(GOLDEN, case["mask"])]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    text = (tmp_path / "out.txt").read_text() if to_file else p.stdout
    assert text == recorded(case)


# --------------------------------------------------------------- fresh inputs --
def random_track(rng, size):
    scale = rng.choice(np.array([1e-3, 1.0, 1e4]), size=size)
    v = (rng.standard_normal(size) * scale).astype(np.float32)
    kind = rng.random(size)
    v[kind < 0.2] = np.nan
    v[(kind >= 0.2) & (kind < 0.25)] = 0.0
    v[(kind >= 0.25) & (kind < 0.26)] = -0.0
    v[(kind >= 0.26) & (kind < 0.27)] = np.float32(1e-41)
    v[(kind >= 0.27) & (kind < 0.28)] = np.float32(3e8)
    return v


def random_intervals(rng, size, n, max_len=600):
    s = rng.integers(-200, size + 100, n)
    e = s + rng.integers(0, max_len, n)
    e[::11] = s[::11] - rng.integers(0, 50, len(s[::11]))        # empty and inverted
    s[::13] = rng.integers(-(2**31), 0, len(s[::13]))            # far left of the track
    e[::17] = rng.integers(size, 2**31, len(e[::17]))            # far right of it
    s[:3], e[:3] = [-(2**31), 0, size - 1], [2**31 - 1, size, size]
    return s[:n].astype(np.int64), e[:n].astype(np.int64)


@pytest.fixture(scope="module")
def world():
    """one track, one mask shorter than it, and the model's answers for the batches the tests below share"""
    rng = np.random.default_rng(7)
    size = 20000 + 37
    track = random_track(rng, size)
    mask = np.zeros(size - 4321, dtype=bool)
    for a in rng.integers(0, len(mask) - 300, 60):
        mask[a:a + int(rng.integers(1, 300))] = True
    mask[64:128] = True
    mask[191:257] = True
    s, e = random_intervals(rng, size, 1000)
    return dict(track=track, mask=mask, s=s, e=e, plain=M.aggregate(track, s, e), masked=M.aggregate(track, s, e, mask))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes(world, n):
    """partial waves: the first n intervals of the shared batch, on each path"""
    t, dm = device_track(world["track"]), device_mask(world["mask"])
    for knob in (HUGE, 0, 128):
        set_knob(knob)
        assert_same(t.aggregate(world["s"][:n], world["e"][:n]), [a[:n] for a in world["plain"]], (n, knob, "plain"))
        assert_same(t.aggregate(world["s"][:n], world["e"][:n], mask=dm), [a[:n] for a in world["masked"]], (n, knob, "masked"))
    t.close()


@pytest.mark.parametrize("knob", KNOBS)
def test_infinities_long_intervals_and_an_inverted_mask(knob):
    """+-inf scores (a sum that turns NaN on the way), intervals longer than the default threshold, a mask whose inversion leaves
    ALL_ONE bins and set bits beyond its size in the last word, and a flat mask"""
    rng = np.random.default_rng(11)
    size = 40000 + 5
    track = random_track(rng, size)
    track[rng.integers(0, size, 12)] = np.inf
    track[rng.integers(0, size, 12)] = -np.inf
    s, e = random_intervals(rng, size, 200, max_len=3000)
    s[5:9], e[5:9] = [0, 1, 63, 100], [size, size - 1, 20000, 9000 + 100]
    small = np.zeros(30000 - 11, dtype=bool)
    small[1000:3000] = True
    small[8191:8193] = True
    inverted = ~small
    t = device_track(track)
    dm = device_mask(small, granularity=16)
    dm.invert()
    from bxmi.bitset import DeviceBitSet

    flat = DeviceBitSet(len(small), flat=True)
    flat.set_ranges(np.array([1000, 8191], dtype=np.int32), np.array([2000, 2], dtype=np.int32))
    set_knob(knob)
    assert_same(t.aggregate(s, e), M.aggregate(track, s, e), (knob, "plain"))
    assert_same(t.aggregate(s, e, mask=dm), M.aggregate(track, s, e, inverted), (knob, "inverted"))
    assert_same(t.aggregate(s, e, mask=flat), M.aggregate(track, s, e, small), (knob, "flat"))
    t.close()


def test_drop_in_bitsets_serve_as_masks(world):
    """a bx.bitset.BinnedBitSet with queued set_range calls (what bxmi.builders hands the command line)"""
    from bx.bitset import BinnedBitSet

    b = BinnedBitSet(len(world["mask"]))
    edges = np.flatnonzero(np.diff(np.concatenate(([0], world["mask"].astype(np.int8), [0]))))
    for a, z in zip(edges[0::2].tolist(), edges[1::2].tolist()):
        b.set_range(a, z - a)
    t = device_track(world["track"])
    assert_same(t.aggregate(world["s"], world["e"], mask=b), world["masked"], "drop-in mask")
    t.close()


def test_set_spans_applies_in_order():
    """overlapping, descending, nested, clipped and empty spans, short ones and ones a wave stores: the later span wins"""
    from bxmi.scores import ScoreTrack

    rng = np.random.default_rng(3)
    size = 5000 + 3
    s = rng.integers(-100, size + 50, 400)
    e = s + rng.integers(0, 90, 400)
    e[::9] = s[::9] + rng.integers(64, 900, len(s[::9]))     # wide
    e[::10] = s[::10] - 1                                     # inverted
    s[100:140] = np.arange(4000, 3600, -10)                   # descending and disjoint
    e[100:140] = s[100:140] + 10
    s[140:160] = np.arange(2000, 2100, 5)                     # ascending, each overlapping the one before
    e[140:160] = s[140:160] + 70
    s[-3:], e[-3:] = [-(2**31), size, 10], [5, 2**31 - 1, 10]
    v = rng.standard_normal(400).astype(np.float32)
    v[::7] = np.nan
    t = ScoreTrack(size)
    assert np.isnan(t.read()).all()
    t.set_spans(s, e, v)
    want = M.fill(size, s, e, v)
    assert np.array_equal(bits(t.read()), bits(want))
    t.set_spans(np.sort(s), np.sort(s) + 3, v)                # a second list on top of the first
    want2 = want.copy()
    for a, x in zip(np.sort(s), v):
        a, z = max(int(a), 0), min(int(a) + 3, size)
        if a < z:
            want2[a:z] = x
    assert np.array_equal(bits(t.read()), bits(want2))
    assert np.array_equal(bits(t.read(1234, 100)), bits(want2[1234:1334]))
    t.set_spans(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    t.close()


def test_windows_and_arguments():
    from bxmi.scores import ScoreTrack

    ffi = _ffi()
    t = ScoreTrack(100)
    t.write(90, np.arange(10, dtype=np.float32))
    assert t.read(88, 12).tolist()[2:] == list(range(10)) and np.isnan(t.read(88, 2)).all()
    import ctypes as C

    p, n = C.c_void_p(), C.c_int64(0)
    ffi.call("bxmi_scores_values_dev", t._h, C.byref(p), C.byref(n))
    assert (p.value, n.value) == t.values_dev() and n.value == 100 and p.value
    through_view = np.empty(100, dtype=np.float32)
    ffi.call("bxmi_memcpy_d2h", ffi.ptr(through_view), p.value, through_view.nbytes)
    assert np.array_equal(bits(through_view), bits(t.read()))
    for bad in (lambda: t.write(95, np.zeros(6, np.float32)), lambda: t.read(-1, 2), lambda: t.read(101, 0), lambda: ScoreTrack(2**31)):
        with pytest.raises(ffi.BxmiError) as err:
            bad()
        assert err.value.code == ffi.EINVAL
    got = t.aggregate(np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert all(len(a) == 0 for a in got)
    got = t.aggregate([95, 0, 50], [200, 90, 50])
    assert got.count.tolist() == [5, 0, 0] and got.total.tolist() == [5 + 6 + 7 + 8 + 9, 0.0, 0.0]
    assert got.minimum.tolist() == [5.0, np.inf, np.inf] and got.maximum.tolist() == [9.0, -np.inf, -np.inf]
    t.close()
    empty = ScoreTrack(0)
    assert empty.aggregate([0], [10]).count.tolist() == [0]
    empty.close()


# ----------------------------------------------------- the device entry point --
@pytest.mark.parametrize("knob", [None, 0, 128])
def test_aggregate_dev_with_guarded_buffers_on_a_callers_stream(world, knob):
    """device pointers of natural alignment only (4 bytes), every output between guard bytes, the inputs copied and the work
    queued on a non-blocking stream of the caller's: the guards stay intact and the results equal the host form's and the model's"""
    from test_gpu_device_entry_points import Guarded, Stream

    n = 1000
    s32, e32 = _ffi().as_i32(np.clip(world["s"], -(2**31), 2**31 - 1)), _ffi().as_i32(np.clip(world["e"], -(2**31), 2**31 - 1))
    t, dm = device_track(world["track"]), device_mask(world["mask"])
    set_knob(knob)
    st = Stream()
    try:
        for mask, want in ((None, world["plain"]), (dm, world["masked"])):
            src_s, src_e = Guarded.holding(s32), Guarded.holding(e32)
            ds, de = Guarded(n * 4, mis=4), Guarded(n * 4, mis=12)
            outs = [Guarded(n * 4, mis=m) for m in (4, 8, 12, 0)]
            st.copy_d2d(ds.ptr, src_s.ptr, n * 4)
            st.copy_d2d(de.ptr, src_e.ptr, n * 4)
            t.aggregate_ptrs(mask, ds.ptr, de.ptr, n, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, stream=st.s)
            st.sync()
            got = []
            for g, dt, name in zip(outs, (np.int32, np.float32, np.float32, np.float32), ("count", "sum", "min", "max")):
                raw = g.check(n * 4, name)
                got.append(g.payload(raw, dt, n))
            assert_same(got, want, ("dev", knob, mask is not None))
            for g, a in ((ds, s32), (de, e32)):
                assert np.array_equal(g.payload(g.check(n * 4, "input"), np.int32, n), a)
            # n = 0 launches nothing and touches nothing
            t.aggregate_ptrs(mask, ds.ptr, de.ptr, 0, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, stream=st.s)
    finally:
        st.close()
        t.close()


def test_aggregate_dev_on_torch_tensors():
    """ScoreTrack.aggregate_dev (torch tensors, torch's current stream) equals ScoreTrack.aggregate on the synthetic case; in a
    process of its own: torch brings its own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from bxmi import wiggle
from bxmi.scores import ScoreTrack
from bxmi.bitset import DeviceBitSet
golden = sys.argv[2]
spans = wiggle.read_spans_file(golden + "/syn.wig.gz")
rows = [l.split() for l in open(golden + "/syn.bed")]
for chrom, (s, e, v) in spans.items():
    t = ScoreTrack(int(e.max()))
    t.set_spans(s, e, v)
    m = DeviceBitSet(int(e.max()))
    m.set_ranges(np.array([64, 1000], dtype=np.int32), np.array([64, 5000], dtype=np.int32))
    qs = np.array([int(r[1]) for r in rows if r[0] == chrom], dtype=np.int32)
    qe = np.array([int(r[2]) for r in rows if r[0] == chrom], dtype=np.int32)
    for mask in (None, m):
        host = t.aggregate(qs, qe, mask=mask)
        dev = t.aggregate_dev(torch.from_numpy(qs).cuda(), torch.from_numpy(qe).cuda(), mask=mask)
        torch.cuda.synchronize()
        for a, b in zip(host, dev):
            assert a.tobytes() == b.cpu().numpy().tobytes(), chrom
    t.close()
print("aggregate_dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), GOLDEN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "aggregate_dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
