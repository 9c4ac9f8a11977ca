"""
Binned bigWig summaries on the device (bxmi_spans_*, bxmi.summary.summarize / summarize_dev / stats, bx.bbi.bigwig_file,
bxmi.cli.bigwig_summary) against the results recorded from the reference (tests/golden/summary) and, beyond them, against
tests/summary_model.py -- itself pinned to those results by tests/test_summary_model_golden.py.  Every comparison is byte for byte,
NaN compared as NaN.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import summary_model as M
from summary_cases import (CHUNK, SLAB_SIZE, TOP_SIZES, assert_planes, assert_slabs, chunk_track, differential_case, empty_planes, random_track, slab_batch,
                           top_case)
from test_summary_model_golden import FILES, path_of, recorded, spans

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_spans_summarize_dev",)
SIZES = (1, 3, 63, 64, 65, 200)
EINVAL = 1
KIND_ROW = {"mean": 0, "max": 1, "min": 2, "coverage": 3, "std": 4}  # rows of the recorded query arrays (summary_model.QUERY_KEYS)


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", sorted(FILES))
def test_summarize_gives_the_recorded_arrays(name):
    """all regions of one file that share a size go through ONE call, rows the reference answers with None included"""
    from bxmi import summary

    tracks = summary.SpanTrack.from_bigwig(path_of(name))
    order = list(tracks)
    cases = FILES[name]["cases"]
    for size in sorted({c["size"] for c in cases}):
        ks = [k for k, c in enumerate(cases) if c["size"] == size]
        rows = [cases[k] for k in ks]
        track_of = [order.index(c["chrom"]) if c["chrom"] in order else -1 for c in rows]
        got = summary.summarize([tracks[c] for c in order], track_of, [c["start"] for c in rows], [c["end"] for c in rows], size)
        want = np.stack([recorded(name, k)[1] if not cases[k]["none"] else empty_planes(size) for k in ks], axis=1)
        assert_planes(got, want, (name, size))
    for chrom, t in tracks.items():
        s, e, _ = spans(name)[chrom]
        assert t.n == len(s) and t.ordered == bool(np.all(np.diff(s) >= 0) and np.all(np.diff(e) >= 0))
        t.close()


@pytest.mark.parametrize("name", sorted(FILES))
def test_drop_in_gives_the_recorded_answers(name):
    import bx.bbi.bigwig_file as drop_in

    with open(path_of(name), "rb") as f:
        bw = drop_in.BigWigFile(f)
    for k, case in enumerate(FILES[name]["cases"]):
        _, planes, query = recorded(name, k)
        args = (case["start"], case["end"], case["size"])
        sd = bw.summarize_from_full(case["chrom"].encode() if k % 2 else case["chrom"], *args)
        if case["none"]:
            assert sd is None and bw.summarize(case["chrom"], *args) is None and bw.query(case["chrom"], *args) is None
            continue
        assert (sd.start, sd.end, sd.size) == args
        assert_planes([getattr(sd, p) for p in M.PLANES], planes, (name, case))
        if case["zoom"]:
            with pytest.raises(NotImplementedError, match="summarize_from_full"):
                bw.query(case["chrom"], *args)
            continue
        assert_planes([getattr(bw.summarize(case["chrom"], *args), p) for p in M.PLANES], planes, (name, case, "summarize"))
        rows = bw.query(case["chrom"], *args)
        assert len(rows) == case["size"] and set(rows[0]) == set(M.QUERY_KEYS)
        for key, want in zip(M.QUERY_KEYS, query):
            assert M.same_bits([float(r[key]) for r in rows], want), (name, case, key)
    bw.close()


def expected_text(name, ks, kind):
    lines = []
    for k in ks:
        case, _, query = recorded(name, k)
        cells = ["n/a"] * case["size"] if case["none"] else ["%.17g" % x for x in query[KIND_ROW[kind]]]
        lines.append("\t".join([case["chrom"], str(case["start"]), str(case["end"])] + cells) + "\n")
    return "".join(lines)


@pytest.mark.parametrize("name", sorted(FILES))
def test_command_line_prints_the_recorded_values(name):
    from bxmi.cli import bigwig_summary

    cases = FILES[name]["cases"]
    kinds = list(KIND_ROW)
    for n_size, size in enumerate(sorted({c["size"] for c in cases})):
        ks = [k for k, c in enumerate(cases) if c["size"] == size and c["start"] <= c["end"]]  # (a BED row cannot hold start > end)
        if not ks:
            continue
        bed = "# regions\n" + "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks)
        for kind in (kinds if n_size == 0 else [kinds[n_size % len(kinds)]]):
            out = io.StringIO()
            bigwig_summary.main([path_of(name), str(size)] + (["-t", kind] if kind != "mean" else []), stdin=io.StringIO(bed), out=out)
            assert out.getvalue() == expected_text(name, ks, kind), (name, size, kind)


def test_command_line_as_a_process():
    name = "straddle.bw"
    cases = FILES[name]["cases"]
    ks = [k for k, c in enumerate(cases) if c["size"] == 64]
    bed = "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks) + "chrNone\t5\t9\n"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cmd = [sys.executable, "-m", "bxmi.cli.bigwig_summary", path_of(name), "64", "-t", "std"]
    got = subprocess.run(cmd, input=bed, env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    assert got == expected_text(name, ks, "std") + "chrNone\t5\t9\t" + "\t".join(["n/a"] * 64) + "\n"


# ------------------------------------------------------------ a seeded differential against the model --
@pytest.mark.parametrize("size", SIZES + (2,))
def test_differential_against_the_model(size):
    from bxmi import summary

    tracks, track_of, starts, ends, want = differential_case(size)
    dev = [summary.SpanTrack(*t) for t in tracks]
    assert [t.ordered for t in dev] == [True, True, False, True, True] and [t.n for t in dev] == [len(t[0]) for t in tracks]
    got = summary.summarize(dev, track_of, starts, ends, size)
    assert_planes(got, want, size)
    # mean, coverage and standard deviation of the rows that have a region
    rows = np.nonzero(starts < ends)[0]
    mine = summary.stats(summary.Summary(*[p[rows] for p in got]), starts[rows], ends[rows], size)
    theirs = M.stats([p[rows] for p in want], starts[rows], ends[rows], size)
    for key, g, w in zip(("mean", "coverage", "std_dev"), mine, theirs):
        assert M.same_bits(g, w), (size, key)
    for t in dev:
        t.close()


def test_chunk_boundaries_carry_the_accumulators():
    """one bin over runs around the chunk size: a wave that dropped its accumulators between chunks would lose all but the last"""
    from bxmi import summary

    track = chunk_track()
    runs = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7, 4 * CHUNK + 63]
    starts = np.array([3 * 7 + 1] * len(runs), dtype=np.int32)  # (the first item is clipped by one base)
    ends = (3 * 7 + 3 * np.array(runs)).astype(np.int32)
    t = summary.SpanTrack(*track)
    for size in (1, 2, 3):
        want = M.summarize([track], np.zeros(len(runs), dtype=np.int32), starts, ends, size)
        got = summary.summarize([t], np.zeros(len(runs), dtype=np.int32), starts, ends, size)
        assert_planes(got, want, size)
        if size == 1:
            assert list(got.valid_count[:, 0]) == [float(3 * r - 1) for r in runs]
    # the same items as a track that is NOT ordered (reversed): the general path walks all of them, in that order
    back = tuple(a[::-1].copy() for a in track)
    tb = summary.SpanTrack(*back)
    assert t.ordered and not tb.ordered
    want = M.summarize([back], np.zeros(len(runs), dtype=np.int32), starts, ends, 3)
    assert_planes(summary.summarize([tb], np.zeros(len(runs), dtype=np.int32), starts, ends, 3), want, "reversed track")
    t.close()
    tb.close()


def test_no_regions_and_bad_arguments():
    import ctypes as C

    from bxmi import _ffi as ffi
    from bxmi import summary

    t = summary.SpanTrack([0, 10], [10, 20], [1.0, 2.0])
    res = summary.summarize([t], [], [], [], 7)
    assert all(p.shape == (0, 7) and p.dtype == np.float64 for p in res)
    none = summary.summarize([], [-1, -1], [0, 5], [10, 6], 3)  # no tracks at all: empty rows
    assert_planes(none, np.stack([empty_planes(3)] * 2, axis=1), "no tracks")
    for args, word in ((([t], [0], [0], [10], 0), "size"), (([t], [0], [0], [10], -2), "size"), (([t], [0], [-1], [10], 2), "negative"),
                       (([t], [0], [0], [-10], 2), "negative"), (([t], [1], [0], [10], 2), "track_of[0]"), (([], [0], [0], [10], 2), "track_of[0]")):
        with pytest.raises(ffi.BxmiError) as e:
            summary.summarize(*args)
        assert e.value.code == EINVAL and word in str(e.value), (args[1:], str(e.value))
    with pytest.raises(ffi.BxmiError) as e:
        summary.SpanTrack([5, -1], [6, 3], [1.0, 1.0])
    assert e.value.code == EINVAL
    handles = (C.c_void_p * 1)(t._h.value)
    for size, n, n_tracks in ((0, 1, 1), (4, -1, 1), (4, 1, -1), (4, 1, 1)):  # (the last: NULL arrays)
        with pytest.raises(ffi.BxmiError) as e:
            ffi.call("bxmi_spans_summarize_dev", handles, n_tracks, None, None, None, n, size, None, None, None, None, None, None)
        assert e.value.code == EINVAL
    ffi.call("bxmi_spans_summarize_dev", handles, 1, None, None, None, 0, 4, None, None, None, None, None, None)  # n == 0: no launch
    t.close()


# ------------------------------------------------------------ the track table --
TABLE_TRACKS = (0, 1, 7, 8, 9, 17)  # around the 8 tracks one launch of the table kernel carries; 8 itself: the spare entry alone in a launch
_table = {}


def table_case(n_tracks):
    """(tracks: track k holds (0, 4, k + 1) and (4, 8, 2 k + 3); one region [0, 8) per track and one row without a track; the device
    form's track_of: one more row, naming the track behind the last; the model's answer for the device form's rows), once per n_tracks"""
    if n_tracks not in _table:
        tracks = [(np.array([0, 4], dtype=np.int32), np.array([4, 8], dtype=np.int32), np.array([k + 1, 2 * k + 3], dtype=np.float32))
                  for k in range(n_tracks)]
        track_of = np.array(list(range(n_tracks)) + [-1], dtype=np.int32)
        starts, ends = np.zeros(len(track_of) + 1, dtype=np.int32), np.full(len(track_of) + 1, 8, dtype=np.int32)
        want = M.summarize(tracks, np.append(track_of, -1), starts, ends, 2)
        _table[n_tracks] = (tracks, track_of, np.append(track_of, n_tracks).astype(np.int32), starts, ends, want)
    return _table[n_tracks]


def summarize_dev_raw(tracks, track_of, starts, ends, size):
    """bxmi_spans_summarize_dev on arrays in device memory, on the null stream -> five [n, size] numpy arrays"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    rows = [ffi.DeviceArray.from_numpy(a) for a in (track_of, starts, ends)]
    planes = [ffi.DeviceArray(8 * n * size) for _ in range(5)]
    ffi.call("bxmi_spans_summarize_dev", ffi.handles(tracks), len(tracks), *[a.ptr for a in rows], n, size, *[a.ptr for a in planes], None)
    ffi.call("bxmi_synchronize", None)
    out = [a.to_numpy(np.float64, n * size).reshape(n, size) for a in planes]
    for a in rows + planes:
        a.free()
    return out


@pytest.mark.parametrize("size", TOP_SIZES)
def test_items_that_end_at_the_top_of_int32(size):
    """an ordered and an unordered track whose last end is 2^31 - 1, regions in their last 100000 bases and up to 2^31 - 1: host
    and device form"""
    from bxmi import summary

    tracks, track_of, starts, ends, want = top_case(size)
    dev = [summary.SpanTrack(*t) for t in tracks]
    assert [t.ordered for t in dev] == [True, False]
    assert_planes(summary.summarize(dev, track_of, starts, ends, size), want, size)
    assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (size, "device form"))
    for t in dev:
        t.close()


def test_host_form_goes_through_more_than_one_slab():
    """2 slabs + 5 rows of 3000 bins: three turns of the host form's slab loop, the middle slab full, the last one short, each
    copied back behind the one before.  Every cell equals the device form's, which has no slabs and which the other tests of this
    file pin to the model; a sample of rows -- those around both slab edges among them, which differ pairwise -- is compared
    with the model itself (summary_cases.assert_slabs)"""
    from bxmi import summary

    rng = np.random.default_rng(83)
    tracks = [random_track(rng, 5000), random_track(rng, 5000)]
    slab, track_of, starts, ends = slab_batch(84, 2, [int(t[1].max()) for t in tracks])
    dev = [summary.SpanTrack(*t) for t in tracks]
    host = summary.summarize(dev, track_of, starts, ends, SLAB_SIZE)
    device = summarize_dev_raw(dev, track_of, starts, ends, SLAB_SIZE)
    assert_slabs(host, device, lambda rows: M.summarize(tracks, track_of[rows], starts[rows], ends[rows], SLAB_SIZE), slab, len(track_of))
    del host, device
    for t in dev:
        t.close()


@pytest.mark.parametrize("n_tracks", TABLE_TRACKS)
def test_track_table_beyond_one_launch(n_tracks):
    """every track's entry and the spare entry behind them arrive, however many launches the table takes: host form (without the row
    the host form refuses) and device form, whose row naming the track behind the last is an empty row"""
    from bxmi import summary

    tracks, track_of, dev_track_of, starts, ends, want = table_case(n_tracks)
    dev = [summary.SpanTrack(*t) for t in tracks]
    assert_planes(summary.summarize(dev, track_of, starts[:-1], ends[:-1], 2), [p[:-1] for p in want], ("host", n_tracks))
    got = summarize_dev_raw(dev, dev_track_of, starts, ends, 2)
    assert_planes(got, want, ("device", n_tracks))
    assert_planes([p[-1:] for p in got], empty_planes(2)[:, None, :], ("the row behind the last track", n_tracks))
    for k in range(n_tracks):
        assert [p[k].tolist() for p in got[:3]] == [[4.0, 4.0], [k + 1.0, 2 * k + 3.0], [k + 1.0, 2 * k + 3.0]]
    for t in dev:
        t.close()


def test_track_table_is_reused_by_a_call_with_fewer_tracks():
    """17 tracks, then 1 track on the same stream: the spare entry now sits where track 1's entry was, so a row naming track 5 is an
    empty row (not track 5's of the call before); then the 17 again"""
    from bxmi import summary

    tracks, _, dev_track_of, starts, ends, want = table_case(17)
    dev = [summary.SpanTrack(*t) for t in tracks]
    assert_planes(summarize_dev_raw(dev, dev_track_of, starts, ends, 2), want, "17 tracks")
    one = M.summarize(tracks[:1], np.array([0, -1], dtype=np.int32), starts[:2], ends[:2], 2)
    assert_planes(summarize_dev_raw(dev[:1], np.array([0, 5], dtype=np.int32), starts[:2], ends[:2], 2), one, "1 track after 17")
    assert_planes(summarize_dev_raw(dev, dev_track_of, starts, ends, 2), want, "17 tracks again")
    for t in dev:
        t.close()


# ------------------------------------------------------------ the kinds of track share the table --
def kinds_case():
    """(9 span tracks, 2 zoom level parts, 17 bed tracks; per kind the 6 rows' track_of; starts, ends; window starts): tracks of at
    most CHUNK + 7 items -- a whole one goes through LDS in two chunks -- one per kind with 0 items, one span track not ordered;
    every batch has a row without a track (-1)"""
    from bxmi.bigwig import ZoomArrays

    rng = np.random.default_rng(9)
    top = CHUNK + 7

    def span(n, back=False):
        k = np.arange(n, dtype=np.int32)
        s, e, v = 2 + 3 * k, 3 + 3 * k + k % 3, rng.standard_normal(n).astype(np.float32)
        return (s[::-1].copy(), e[::-1].copy(), v) if back else (s, e, v)

    def level(n):
        k = np.arange(n, dtype=np.int32)
        sums = rng.standard_normal(n).astype(np.float32)
        first = np.append(np.arange(0, n, 5, dtype=np.int64), n) if n else np.zeros(1, np.int64)
        return ZoomArrays(3 * k, 3 * k + 3, (1 + k % 3).astype(np.uint32), sums - 1, sums + 1, sums, sums * sums,
                          (3 * first[:-1]).astype(np.int32), (3 * first[1:]).astype(np.int32), first)

    def bed(n):
        k = np.arange(n, dtype=np.int32)
        return 3 * k, 3 * k + 1 + (7 * k) % 11  # (ends that descend: records that nest)

    spans_ = [span(top), span(0), span(1), span(5), span(64), span(100, back=True), span(CHUNK), span(3), span(top)]
    zooms = [level(top), level(0)]
    beds = [bed(n) for n in (top, 0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 64, 65, 89, 144, CHUNK, top)]
    starts = np.array([0, 1, 5, 0, 7, 3 * CHUNK - 30], dtype=np.int32)
    ends = np.array([3 * top + 5, 200, 50, 900, 7 + 65 * 4 + 3, 3 * CHUNK + 40], dtype=np.int32)
    track_of = {"spans": [0, 8, -1, 1, 5, 6], "zoom": [0, 0, -1, 1, 0, 0], "beds": [16, 0, -1, 1, 14, 15], "one": [0, -1, 0, 0, -1, 0]}
    windows = np.array([0, 3 * CHUNK - 2, -3, 100, 7, 50], dtype=np.int32)
    return spans_, zooms, beds, {k: np.array(v, dtype=np.int32) for k, v in track_of.items()}, starts, ends, windows


def test_kinds_share_the_table_back_to_back():
    """the library's one track table is rewritten by every call with entries of that call's kind, which differ in size: spans (9
    tracks: a pack of 8 and one more), zoom (2), beds (17), the per-base matrix over the 9 span tracks, spans again (1 track) --
    one call after the other, once through the host forms and once through the device forms queued on ONE stream with nothing
    waited for in between.  Every answer is the model's, byte for byte"""
    import arrays_model
    import bed_cases
    import zoom_model
    from bxmi import _ffi as ffi
    from bxmi import summary

    spans_, zooms, beds, track_of, starts, ends, windows = kinds_case()
    width, n = 5, len(starts)
    dev = {"spans": [summary.SpanTrack(*t) for t in spans_], "zoom": [summary.ZoomTrack(z) for z in zooms],
           "beds": [summary.BedTrack(*t) for t in beds]}
    dev["one"] = dev["spans"][:1]
    symbols = {"spans": "bxmi_spans_summarize_dev", "zoom": "bxmi_zoom_summarize_dev", "beds": "bxmi_beds_summarize_dev", "one": "bxmi_spans_summarize_dev"}
    want_matrix = arrays_model.matrix(spans_, track_of["spans"], windows, width)
    for size in (3, 65):  # one group of bins, and two
        want = {"spans": M.summarize(spans_, track_of["spans"], starts, ends, size),
                "zoom": zoom_model.summarize(zooms, track_of["zoom"], starts, ends, size),
                "beds": bed_cases.model(beds, track_of["beds"], starts, ends, size),
                "one": M.summarize(spans_[:1], track_of["one"], starts, ends, size)}
        # the host forms
        assert_planes(summary.summarize(dev["spans"], track_of["spans"], starts, ends, size), want["spans"], ("host", "spans", size))
        assert_planes(summary.summarize_zoom(dev["zoom"], track_of["zoom"], starts, ends, size), want["zoom"], ("host", "zoom", size))
        assert_planes(summary.summarize_beds(dev["beds"], track_of["beds"], starts, ends, size), want["beds"], ("host", "beds", size))
        arrays_model.assert_same(summary.matrix(dev["spans"], track_of["spans"], windows, width), want_matrix, ("host", "matrix", size))
        assert_planes(summary.summarize(dev["one"], track_of["one"], starts, ends, size), want["one"], ("host", "one span track", size))
        # the device forms: everything allocated and copied first, then the five calls queued on the null stream, then one wait
        d_rows = {k: ffi.DeviceArray.from_numpy(v) for k, v in track_of.items()}
        d_starts, d_ends, d_windows = (ffi.DeviceArray.from_numpy(a) for a in (starts, ends, windows))
        d_planes = {k: [ffi.DeviceArray(8 * n * size) for _ in range(5)] for k in symbols}
        d_matrix = ffi.DeviceArray(4 * n * width)
        for k in ("spans", "zoom", "beds", "matrix", "one"):
            if k == "matrix":
                ffi.call("bxmi_spans_arrays_dev", ffi.handles(dev["spans"]), len(dev["spans"]), d_rows["spans"].ptr, d_windows.ptr, n, width, None,
                         n * width, d_matrix.ptr, None)
            else:
                ffi.call(symbols[k], ffi.handles(dev[k]), len(dev[k]), d_rows[k].ptr, d_starts.ptr, d_ends.ptr, n, size,
                         *[a.ptr for a in d_planes[k]], None)
        ffi.call("bxmi_synchronize", None)
        for k in symbols:
            assert_planes([a.to_numpy(np.float64, n * size).reshape(n, size) for a in d_planes[k]], want[k], ("device", k, size))
        arrays_model.assert_same(d_matrix.to_numpy(np.float32, n * width).reshape(n, width), want_matrix, ("device", "matrix", size))
        for a in list(d_rows.values()) + [d_starts, d_ends, d_windows, d_matrix] + [a for planes in d_planes.values() for a in planes]:
            a.free()
    for t in dev["spans"] + dev["zoom"] + dev["beds"]:
        t.close()


# ------------------------------------------------------------ device entry point --
def test_summarize_dev_equals_summarize_and_the_recorded_arrays():
    """summarize_dev on torch tensors -- every recorded case, a seeded batch on slices that start 4 bytes into their allocation,
    torch's current stream and a stream of the caller's, an empty batch, the torch form of stats -- in a process of its own: torch
    brings its own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import summary_model as M
from test_summary_model_golden import FILES, path_of, recorded
from summary_cases import differential_case, empty_planes
from bxmi import summary

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

checked = 0
for name in sorted(FILES):
    tracks = summary.SpanTrack.from_bigwig(path_of(name))
    order = list(tracks)
    cases = FILES[name]["cases"]
    for size in sorted({c["size"] for c in cases}):
        ks = [k for k, c in enumerate(cases) if c["size"] == size and not c["none"]]
        if not ks:
            continue
        rows = [cases[k] for k in ks]
        args = [np.array(x) for x in ([order.index(c["chrom"]) for c in rows], [c["start"] for c in rows], [c["end"] for c in rows])]
        res = summary.summarize_dev([tracks[c] for c in order], *[dev_i32(a, 0) for a in args], size)
        torch.cuda.synchronize()
        want = np.stack([recorded(name, k)[1] for k in ks], axis=1)
        query = np.stack([recorded(name, k)[2] for k in ks], axis=1)
        for p, g, w in zip(M.PLANES, res, want):
            assert g.dtype == torch.float64 and M.same_bits(g.cpu().numpy(), w), (name, size, p)
        mean, coverage, std = summary.stats(res, dev_i32(args[1], 0), dev_i32(args[2], 0), size)
        # (torch's float64 division and square root on the device are the IEEE ones: tools/bench_summary.py's docstring has the probe)
        for key, g, w in (("mean", mean, query[0]), ("coverage", coverage, query[3]), ("std_dev", std, query[4])):
            assert g.is_cuda and M.same_bits(g.cpu().numpy(), w), (name, size, key)
        checked += len(ks)
    for t in tracks.values():
        t.close()
assert checked >= 60, checked

size = 65
tracks, track_of, starts, ends, want = differential_case(size)
dev = [summary.SpanTrack(*t) for t in tracks]
host = summary.summarize(dev, track_of, starts, ends, size)
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
assert all(x.data_ptr() % 16 for x in d)
torch.cuda.synchronize()

def same(res, what):
    for p, g, h, w in zip(M.PLANES, res, host, want):
        assert M.same_bits(g.cpu().numpy(), h) and M.same_bits(h, w), (what, p)

res = summary.summarize_dev(dev, *d, size)
torch.cuda.synchronize()
same(res, "current stream")
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    res = summary.summarize_dev(dev, *d, size)
side.synchronize()
same(res, "side stream")
# entries the device form cannot refuse are empty rows: a track index beyond the list, a negative coordinate
odd = summary.summarize_dev(dev, dev_i32(np.array([9, 0, 0]), 0), dev_i32(np.array([0, -5, 0]), 0), dev_i32(np.array([50, 50, -1]), 0), 4, stream=side.cuda_stream)
side.synchronize()
for g, w in zip(odd, np.stack([empty_planes(4)] * 3, axis=1)):
    assert M.same_bits(g.cpu().numpy(), w)
res = summary.summarize_dev(dev, d[0][:0], d[1][:0], d[2][:0], size, stream=side.cuda_stream)
side.synchronize()
assert all(tuple(g.shape) == (0, size) for g in res)
for t in dev:
    t.close()
print("summarize_dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "summarize_dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
