"""
Site profiles on the device (bxmi_scores_profile*, bxmi.scores.profile / profile_dev / ScoreTrack.profile,
bxmi.cli.bed_bigwig_profile) against tests/profile_model.py -- itself pinned to the reference's recorded results by
tests/test_profile_model_golden.py -- and, for the command line, against the recorded text.  Every comparison of totals is byte
for byte (NaN compared as NaN), every comparison of valid is of int32 arrays.

`scores.profile_chain` forces every column onto the ordered chain (1) or keeps every column off it (-1, wrong on purpose); what
it was before a test is put back afterwards.

The hand-made columns of test_chain_is_what_makes_the_totals_right: three successive rows hold 1e30f, 1.0f, -1e30f, whose ordered
float64 sum is 0.0.  Without the chain (-1) the column inside one chunk comes out as 1.0, because the partial pass keeps even and
odd rows apart (1e30 - 1e30, then + 1.0).  The column whose three rows straddle a chunk boundary comes out as 0.0 with or without
the chain: whichever chunk holds the 1.0 also holds 1e30 or -1e30, which absorbs it in ANY chunked evaluation, so no design with
chunks of consecutive rows can make that column show 1.0.  A third column makes the boundary visible instead: 1e30 ends a chunk,
-1e30 and 1.0 start the next; ordered 1.0, chunked 0.0.
"""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import profile_model as M
from test_profile_model_golden import GOLDEN, PROFILES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_scores_profile_dev",)
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "profile.hpp")) as _f:
    CHUNK = int(re.search(r"constexpr int PF_CHUNK = (\d+);", _f.read()).group(1))
WIDTHS = (1, 10, 64, 70, 130)
EINVAL = 1


def _ffi():
    from bxmi import _ffi

    return _ffi


DEFAULT_CHAIN = _ffi().options()["scores.profile_chain"]


def set_chain(v):
    _ffi().call("bxmi_set_option", b"scores.profile_chain", int(v))


@pytest.fixture(autouse=True)
def _chain_back():
    yield
    set_chain(DEFAULT_CHAIN)


def device_tracks(arrays):
    from bxmi.scores import ScoreTrack

    out = []
    for a in arrays:
        t = ScoreTrack(len(a))
        if len(a):
            t.write(0, a)
        out.append(t)
    return out


def assert_same(got, want, what):
    totals, valid = np.asarray(got[0]), np.asarray(got[1])
    assert totals.dtype == np.float64 and valid.dtype == np.int32, what
    assert np.array_equal(valid, want[1]), (what, np.nonzero(valid != want[1])[0][:8])
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(totals), nan), (what, "nan")
    bad = np.nonzero((totals.view(np.uint64) != want[0].view(np.uint64)) & ~nan)[0]
    assert len(bad) == 0, (what, bad[:8], totals[bad[:4]], want[0][bad[:4]])


def three_decimal_track(rng, size, nan=0.1):
    t = (rng.integers(0, 1001, size=size) / 1000.0).astype(np.float32)
    t[rng.random(size) < nan] = np.nan
    return t


# ------------------------------------------------------------ widths and chunk boundaries --
_shape = {}


def shape_case(width, n):
    """(track, starts, the model's answer), once per shape: windows inside, hanging off both ends and wholly outside the track"""
    if (width, n) not in _shape:
        rng = np.random.default_rng(1000 * width + n)
        track = three_decimal_track(rng, 3001)
        starts = rng.integers(-width - 5, len(track) + 5, size=n).astype(np.int32)
        if n > 3:
            starts[:4] = (-width, -width + 1, len(track) - 1, len(track))
        _shape[(width, n)] = (track, starts, M.profile([track], np.zeros(n, dtype=np.int32), starts, width))
    return _shape[(width, n)]


@pytest.mark.parametrize("chain", (0, 1))
@pytest.mark.parametrize("n", (0, 1, CHUNK - 1, CHUNK, CHUNK + 1))
@pytest.mark.parametrize("width", WIDTHS)
def test_widths_and_chunk_boundaries(width, n, chain):
    """three-decimal scores: with the option at 0 no column needs the chain, at 1 every column runs it; both are the model's bits"""
    track, starts, want = shape_case(width, n)
    (t,) = device_tracks([track])
    set_chain(chain)
    got = t.profile(starts, width)
    assert_same(got, want, (width, n, chain))
    assert got.chain_columns == (width if chain and n else 0)
    t.close()


@pytest.mark.parametrize("chain", (0, 1))
def test_window_starts_at_the_ends_of_int32(chain):
    from bxmi import scores

    rng = np.random.default_rng(5)
    width = 70
    track = three_decimal_track(rng, 200)
    lo, hi = -2 ** 31, 2 ** 31 - 1
    starts = np.array([lo, lo + width, lo + width - 1, hi, hi - 1, hi - width, hi - width // 2, 0, 199, -69, -70, 130, 131], dtype=np.int32)
    track_of = np.zeros(len(starts), dtype=np.int32)
    (t,) = device_tracks([track])
    set_chain(chain)
    assert_same(scores.profile([t], track_of, starts, width), M.profile([track], track_of, starts, width), chain)
    t.close()


# ------------------------------------------------------------ several tracks, interleaved --
@pytest.mark.parametrize("chain", (0, 1))
def test_three_tracks_interleaved_row_by_row(chain):
    """one chain per column over the rows in the order given, whatever track each row reads; a track of size 0; rows without a track"""
    from bxmi import scores

    rng = np.random.default_rng(11)
    width, n = 70, CHUNK + 37
    wide = (rng.standard_normal(1234) * np.exp2(rng.integers(-30, 31, size=1234))).astype(np.float32)
    wide[rng.random(1234) < 0.1] = np.nan
    tracks = [three_decimal_track(rng, 500), np.zeros(0, dtype=np.float32), wide]
    track_of = rng.integers(-1, 3, size=n).astype(np.int32)
    track_of[:6] = (0, 1, 2, -1, 2, 0)
    starts = rng.integers(-80, 1300, size=n).astype(np.int32)
    want = M.profile(tracks, track_of, starts, width)
    dev = device_tracks(tracks)
    set_chain(chain)
    got = scores.profile(dev, track_of, starts, width)
    assert_same(got, want, chain)
    assert got.chain_columns > 0  # (the wide-range track makes the columns order-sensitive)
    # no tracks at all: zeros, whichever way they were summed (forced, all 9 columns run the chain over rows without a score)
    none = scores.profile([], np.full(5, -1, dtype=np.int32), np.arange(5, dtype=np.int32), 9)
    assert not none.totals.any() and not np.signbit(none.totals).any() and not none.valid.any()
    assert none.chain_columns == (9 if chain else 0)
    for t in dev:
        t.close()


# ------------------------------------------------------------ special values --
@pytest.mark.parametrize("chain", (0, 1))
def test_special_values(chain):
    """row i reads track[8 i : 8 i + 8], so column j of the profile is written down here as a column"""
    nan, inf = np.nan, np.inf
    columns = [
        (nan, nan, nan, nan),             # nothing: +0.0, valid 0
        (0.0, -0.0, -0.0, nan),           # zeros of both signs are scores: +0.0, valid 3
        (nan, -0.0, nan, nan),            # +0.0 + -0.0 = +0.0
        (1e-45, 3e-39, -1e-45, 1e-45),    # denormals
        (inf, 1.0, 2.0, nan),             # inf
        (inf, -inf, 1.0, nan),            # NaN
        (1e-45, 1.0, 1e30, -1e30),        # 200 binary orders of magnitude apart
        (0.5, 0.25, nan, 0.125),
    ]
    track = np.array(columns, dtype=np.float32).T.copy().reshape(-1)
    starts = np.arange(4, dtype=np.int32) * 8
    want = M.profile([track], np.zeros(4, dtype=np.int32), starts, 8)
    assert np.isnan(want[0][5]) and want[0][4] == inf and list(want[1]) == [0, 3, 1, 4, 3, 3, 4, 3]
    (t,) = device_tracks([track])
    set_chain(chain)
    got = t.profile(starts, 8)
    assert_same(got, want, chain)
    assert not np.signbit(got.totals[:3]).any()
    if chain == 0:
        assert got.chain_columns >= 3  # the two columns with an inf and the wide one cannot be summed in parallel
    t.close()


# ------------------------------------------------------------ the exact path --
def test_three_decimal_scores_never_need_the_chain():
    rng = np.random.default_rng(3)
    width, n = 130, 4096
    track = three_decimal_track(rng, 50000, nan=0.05)
    starts = rng.integers(-40, len(track) - 60, size=n).astype(np.int32)
    want = M.profile([track], np.zeros(n, dtype=np.int32), starts, width)
    (t,) = device_tracks([track])
    got = t.profile(starts, width)
    assert got.chain_columns == 0
    assert_same(got, want, "parallel")
    set_chain(1)
    forced = t.profile(starts, width)
    assert forced.chain_columns == width
    assert forced.totals.tobytes() == got.totals.tobytes() and np.array_equal(forced.valid, got.valid)
    t.close()


# ------------------------------------------------------------ the chain path --
_wide = {}


def wide_case():
    if not _wide:
        case = M.wide_range_case()
        _wide["case"], _wide["want"] = case, M.profile(*case)
    return _wide["case"], _wide["want"]


def test_wide_range_scores_take_the_chain():
    (tracks, track_of, starts, width), want = wide_case()
    (t,) = device_tracks(tracks)
    got = t.profile(starts, width)
    assert got.chain_columns > 0
    assert_same(got, want, "chain")
    set_chain(-1)
    off = t.profile(starts, width)
    assert off.chain_columns == 0 and np.array_equal(off.valid, want[1])
    # this case can see the chain: without it most columns carry other bits
    assert np.mean(off.totals.view(np.uint64) != want[0].view(np.uint64)) >= 0.5
    t.close()


def test_chain_is_what_makes_the_totals_right():
    """the hand-made columns of the module docstring; row i reads track[3 i : 3 i + 3]"""
    n = CHUNK + 3
    cols = np.full((n, 3), np.nan, dtype=np.float32)
    cols[0:3, 0] = (1e30, 1.0, -1e30)                   # three successive rows inside the first chunk
    cols[CHUNK - 1:CHUNK + 2, 1] = (1e30, 1.0, -1e30)   # the same three rows across the chunk boundary
    cols[CHUNK - 1:CHUNK + 2, 2] = (1e30, -1e30, 1.0)   # 1e30 ends a chunk, -1e30 and 1.0 start the next
    track = cols.reshape(-1)
    starts = (np.arange(n) * 3).astype(np.int32)
    want = M.profile([track], np.zeros(n, dtype=np.int32), starts, 3)
    assert list(want[0]) == [0.0, 0.0, 1.0] and list(want[1]) == [3, 3, 3]
    (t,) = device_tracks([track])
    try:
        got = t.profile(starts, 3)
        assert_same(got, want, "default")
        assert got.chain_columns == 3
        set_chain(1)
        assert_same(t.profile(starts, 3), want, "forced")
        set_chain(-1)
        off = t.profile(starts, 3)
        assert off.chain_columns == 0 and list(off.valid) == [3, 3, 3]
        assert list(off.totals) == [1.0, 0.0, 0.0]
    finally:
        set_chain(DEFAULT_CHAIN)
        t.close()


# ------------------------------------------------------------ device entry points --
def test_profile_dev_equals_profile():
    """profile_dev on torch tensors -- slices that start 4 bytes into their allocation, torch's current stream and a stream of the
    caller's, an empty batch -- equals profile, itself compared with the model here; in a process of its own: torch brings its own
    HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import profile_model as M
from bxmi import scores
chunk = int(sys.argv[3])
rng = np.random.default_rng(21)
width, n = 70, chunk + 5
three = (rng.integers(0, 1001, size=900) / 1000.0).astype(np.float32)
three[rng.random(900) < 0.1] = np.nan
tracks = [three, (rng.standard_normal(700) * np.exp2(rng.integers(-30, 31, size=700))).astype(np.float32)]
track_of = rng.integers(-1, 2, size=n).astype(np.int32)
starts = rng.integers(-80, 950, size=n).astype(np.int32)
dev = []
for a in tracks:
    t = scores.ScoreTrack(len(a))
    t.write(0, a)
    dev.append(t)
host = scores.profile(dev, track_of, starts, width)
want = M.profile(tracks, track_of, starts, width)
assert host.totals.tobytes() == want[0].tobytes() and np.array_equal(host.valid, want[1]) and host.chain_columns > 0
d_track = torch.from_numpy(np.concatenate([[7], track_of]).astype(np.int32)).cuda()[1:]
d_start = torch.from_numpy(np.concatenate([[7, 7, 7], starts]).astype(np.int32)).cuda()[3:]
assert d_track.data_ptr() % 16 and d_start.data_ptr() % 16
torch.cuda.synchronize()

def same(res, what):
    assert res.totals.dtype == torch.float64 and res.valid.dtype == torch.int32, what
    assert res.totals.cpu().numpy().tobytes() == host.totals.tobytes(), what
    assert np.array_equal(res.valid.cpu().numpy(), host.valid), what
    assert int(res.chain_columns.item()) == host.chain_columns, what

res = scores.profile_dev(dev, d_track, d_start, width)
torch.cuda.synchronize()
same(res, "current stream")
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    res = scores.profile_dev(dev, d_track, d_start, width)
side.synchronize()
same(res, "side stream")
res = scores.profile_dev(dev, d_track[:0], d_start[:0], width, stream=side.cuda_stream)
side.synchronize()
assert not res.totals.cpu().numpy().any() and not res.valid.cpu().numpy().any() and int(res.chain_columns.item()) == 0
for t in dev:
    t.close()
print("profile_dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests"), str(CHUNK)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "profile_dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


def test_bad_arguments_are_einval():
    import ctypes as C

    from bxmi import scores

    ffi = _ffi()
    (t,) = device_tracks([np.zeros(10, dtype=np.float32)])
    one = np.zeros(1, dtype=np.int32)
    out_t, out_v = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.int32)
    handles = (C.c_void_p * 1)(t._h.value)

    def host(n_tracks, track_of, n, width):
        return ffi.load().bxmi_scores_profile(handles, n_tracks, ffi.ptr(track_of), ffi.ptr(one), n, width, ffi.ptr(out_t), ffi.ptr(out_v), None)

    assert host(1, one, 1, 4) == 0
    for args, word in (((1, one, 1, 0), "width"), ((1, one, 1, -3), "width"), ((1, one, -1, 4), "n ="), ((-1, one, 1, 4), "n_tracks"),
                       ((1, one + 1, 1, 4), "track_of[0]"), ((0, one, 1, 4), "track_of[0]")):
        assert host(*args) == EINVAL, args
        assert word in ffi.load().bxmi_last_error().decode(), (args, ffi.load().bxmi_last_error())
    for width, n, n_tracks in ((0, 1, 1), (4, -1, 1), (4, 1, -1)):
        with pytest.raises(ffi.BxmiError) as e:
            ffi.call("bxmi_scores_profile_dev", handles, n_tracks, None, None, n, width, None, None, None, None)
        assert e.value.code == EINVAL
    with pytest.raises(ffi.BxmiError):
        scores.profile([t], [1], [0], 4)
    with pytest.raises(ffi.BxmiError):
        t.profile([0], 0)
    t.close()


# ------------------------------------------------------------ the track table --
TABLE_TRACKS = (0, 1, 15, 16, 17, 33)  # around the 16 tracks one launch of the table kernel carries; 16 itself: the spare entry alone in a launch
_table = {}


def table_case(n_tracks):
    """(tracks: track k is 8 floats of value k + 1; one window per track at 2 and two rows without a track; the device form's rows:
    one more, naming the track behind the last; the model's answer, the same for both), once per n_tracks"""
    if n_tracks not in _table:
        arrays = [np.full(8, k + 1, dtype=np.float32) for k in range(n_tracks)]
        track_of = np.array(list(range(n_tracks)) + [-1, -1], dtype=np.int32)
        starts = np.full(len(track_of) + 1, 2, dtype=np.int32)
        want = M.profile(arrays, np.append(track_of, -1), starts, 4)
        assert list(want[0]) == [n_tracks * (n_tracks + 1) / 2.0] * 4 and list(want[1]) == [n_tracks] * 4
        _table[n_tracks] = (arrays, track_of, starts[:-1], np.append(track_of, n_tracks).astype(np.int32), starts, want)
    return _table[n_tracks]


def profile_dev_raw(tracks, track_of, starts, width):
    """bxmi_scores_profile_dev on arrays in device memory, on the null stream -> (totals, valid) as numpy arrays"""
    ffi = _ffi()
    bufs = [ffi.DeviceArray.from_numpy(track_of), ffi.DeviceArray.from_numpy(starts), ffi.DeviceArray(8 * width), ffi.DeviceArray(4 * width)]
    ffi.call("bxmi_scores_profile_dev", ffi.handles(tracks), len(tracks), bufs[0].ptr, bufs[1].ptr, len(track_of), width, bufs[2].ptr,
             bufs[3].ptr, None, None)
    ffi.call("bxmi_synchronize", None)
    out = bufs[2].to_numpy(np.float64, width), bufs[3].to_numpy(np.int32, width)
    for b in bufs:
        b.free()
    return out


@pytest.mark.parametrize("n_tracks", TABLE_TRACKS)
def test_track_table_beyond_one_launch(n_tracks):
    """every track's entry and the spare entry behind them arrive, however many launches the table takes: host form and device form"""
    from bxmi import scores

    arrays, track_of, starts, dev_track_of, dev_starts, want = table_case(n_tracks)
    dev = device_tracks(arrays)
    assert_same(scores.profile(dev, track_of, starts, 4), want, ("host", n_tracks))
    assert_same(profile_dev_raw(dev, dev_track_of, dev_starts, 4), want, ("device", n_tracks))
    for t in dev:
        t.close()


def test_track_table_is_reused_by_a_call_with_fewer_tracks():
    """17 tracks, then 1 track on the same stream: the spare entry now sits where track 1's entry was, so a row naming track 5 has no
    score (not track 5's of the call before); then the 17 again"""
    arrays, _, _, dev_track_of, dev_starts, want = table_case(17)
    dev = device_tracks(arrays)
    assert_same(profile_dev_raw(dev, dev_track_of, dev_starts, 4), want, "17 tracks")
    one = M.profile(arrays[:1], np.array([0, -1], dtype=np.int32), dev_starts[:2], 4)
    assert list(one[0]) == [1.0] * 4 and list(one[1]) == [1] * 4
    assert_same(profile_dev_raw(dev[:1], np.array([0, 5], dtype=np.int32), dev_starts[:2], 4), one, "1 track after 17")
    assert_same(profile_dev_raw(dev, dev_track_of, dev_starts, 4), want, "17 tracks again")
    for t in dev:
        t.close()


def test_library_scratch_follows_the_device():
    """one profile and one summary call on device 0, on device 1, on device 0 again, tracks made on the device that uses them: the
    library's scratch (buffers and stream) is dropped and made again at each change.  One pass."""
    import summary_model as SM
    from bxmi import scores, summary

    ffi = _ffi()
    if ffi.device_count() < 2:
        pytest.skip("one device visible: the scratch never changes device")
    arrays, track_of, starts, _, _, want = table_case(17)
    spans = [(np.array([0, 4], dtype=np.int32), np.array([4, 8], dtype=np.int32), np.array([k + 1, 2 * k + 3], dtype=np.float32)) for k in range(9)]
    s_track_of, s_starts, s_ends = np.array(list(range(9)) + [-1], dtype=np.int32), np.zeros(10, dtype=np.int32), np.full(10, 8, dtype=np.int32)
    s_want = SM.summarize(spans, s_track_of, s_starts, s_ends, 2)
    try:
        for device in (0, 1, 0):
            ffi.call("bxmi_set_device", device)
            dev, sdev = device_tracks(arrays), [summary.SpanTrack(*t) for t in spans]
            assert_same(scores.profile(dev, track_of, starts, 4), want, ("profile on device", device))
            got = summary.summarize(sdev, s_track_of, s_starts, s_ends, 2)
            assert all(SM.same_bits(g, w) for g, w in zip(got, s_want)), ("summary on device", device)
            for t in dev + sdev:
                t.close()
    finally:
        ffi.call("bxmi_set_device", 0)


# ------------------------------------------------------------ the command line --
def run_cli(score_file, padding, bed):
    from bxmi.cli import bed_bigwig_profile

    out = io.StringIO()
    with open(os.path.join(GOLDEN, bed)) as f:
        bed_bigwig_profile.main([os.path.join(GOLDEN, score_file), str(padding)], stdin=f, out=out)
    return out.getvalue()


@pytest.mark.parametrize("name", sorted(PROFILES))
def test_command_line_prints_the_recorded_text(name):
    case = PROFILES[name]
    with open(os.path.join(GOLDEN, case["text"])) as f:
        assert run_cli(case["scores"], case["padding"], case["bed"]) == f.read()


def test_command_line_reads_wiggle_too():
    """bg.wig is bg.bw's track as wiggle text (tests/test_bigwig_reader.py): every recorded window lies below its largest span end"""
    for name in ("bg", "bg.gap"):
        case = PROFILES[name]
        with open(os.path.join(GOLDEN, case["text"])) as f:
            assert run_cli("bg.wig", case["padding"], case["bed"]) == f.read()


def test_command_line_as_a_process():
    """python -m bxmi.cli.bed_bigwig_profile score_file padding < bed, with a comment line, an unknown chromosome and a window that
    starts below zero in the BED: rows the reference crashes on have no data here"""
    case = PROFILES["two.z"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    with open(os.path.join(GOLDEN, case["bed"])) as f:
        bed = f.read()
    cmd = [sys.executable, "-m", "bxmi.cli.bed_bigwig_profile", os.path.join(GOLDEN, case["scores"]), str(case["padding"])]
    got = subprocess.run(cmd, input="# sites\n" + bed + "chrNone\t5\t9\n", env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    with open(os.path.join(GOLDEN, case["text"])) as f:
        assert got == f.read()
    # a window that starts below zero counts where it has data
    tracks = {c: M.fill_spans(size, spans) for (c, size), spans in zip((("chrA", 100), ("chrBB", 50)), _two_spans())}
    rows = M.bed_rows(os.path.join(GOLDEN, case["bed"])) + [("chrA", 2, 4)]
    chroms, starts, width = M.centred_windows(rows, case["padding"])
    names = list(tracks)
    want = M.text(*M.profile([tracks[c] for c in names], [names.index(c) for c in chroms], starts, width))
    got = subprocess.run(cmd, input=bed + "chrA\t2\t4\n", env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert got == want and starts[-1] < 0


def _two_spans():
    from bxmi import bigwig

    spans = bigwig.read_spans_file(os.path.join(GOLDEN, "two.z.bw"))
    return spans["chrA"], spans["chrBB"]
