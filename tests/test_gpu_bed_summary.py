"""
bigBed coverage summaries on the device (bxmi_beds_*, bxmi.summary.summarize_beds / summarize_beds_dev / BedSet,
bx.bbi.bigbed_file, bxmi.cli.bigbed_summary) against the results recorded from the reference (tests/golden/bigbed) and, beyond
them, against tests/summary_model.py over the same records as items of value 1 -- itself pinned to those results by
tests/test_bigbed_model_golden.py.  Every comparison is byte for byte, NaN compared as NaN.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import summary_model as M
from bed_cases import (CHUNK, FILES, ROOT, SIZES, TOP_SIZES, WINDOW, assert_planes, by_size, chunk_cases, differential_case, empty_planes, items, model,
                       nested_track, path_of, recorded, recorded_batch, top_case, window_cases, with_ones)
from summary_cases import SLAB_SIZE, assert_slabs, slab_batch

pytestmark = pytest.mark.gpu

# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_beds_summarize_dev",)
EINVAL = 1
KIND_ROW = {"mean": 0, "max": 1, "min": 2, "coverage": 3, "std": 4}  # rows of the recorded query arrays (summary_model.QUERY_KEYS)

sys.path.insert(0, os.path.join(ROOT, "tools"))


def summarize_dev_raw(tracks, track_of, starts, ends, size):
    """bxmi_beds_summarize_dev on arrays in device memory, on the null stream -> five [n, size] numpy arrays"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts, ends)]
    planes = [ffi.DeviceArray(8 * n * size) for _ in range(5)]
    ffi.call("bxmi_beds_summarize_dev", ffi.handles(tracks), len(tracks), *[a.ptr for a in rows], n, size, *[a.ptr for a in planes], None)
    ffi.call("bxmi_synchronize", None)
    out = [a.to_numpy(np.float64, n * size).reshape(n, size) for a in planes]
    for a in rows + planes:
        a.free()
    return out


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", sorted(FILES))
def test_summarize_beds_gives_the_recorded_arrays(name):
    """all regions of one file that share a size go through ONE call of each form, rows the reference answers with None included"""
    from bxmi import summary

    tracks = summary.BedTrack.from_bigbed(path_of(name))
    order = list(tracks)
    assert order == list(FILES[name]["chroms"])
    for size, ks, track_of, starts, ends in by_size(name):
        want = recorded_batch(name, ks, size)
        assert_planes(summary.summarize_beds([tracks[c] for c in order], track_of, starts, ends, size), want, (name, size))
        assert_planes(summarize_dev_raw([tracks[c] for c in order], track_of, starts, ends, size), want, (name, size, "device form"))
    for chrom, t in tracks.items():
        s, _, _ = items(name)[chrom]
        assert t.n == len(s) and t.sorted is True
        t.close()


@pytest.mark.parametrize("name", sorted(FILES))
def test_bed_set_answers_as_the_references_summarize(name):
    """a mixed batch: rows from a zoom level and rows from the records in one BedSet.summarize; zoom=False is summarize_from_full"""
    from bxmi import summary

    beds = summary.BedSet.from_bigbed(path_of(name))
    assert beds.chroms == list(FILES[name]["chroms"]) and beds.reductions == FILES[name]["reductions"] and not beds.not_ordered
    with open(path_of(name), "rb") as f:
        twin = summary.BedSet.from_bigbed(data=f.read())
    for size, ks, _, starts, ends in by_size(name):
        chroms = [FILES[name]["cases"][k]["chrom"] for k in ks]
        assert_planes(beds.summarize(chroms, starts, ends, size), recorded_batch(name, ks, size, which=2), (name, size, "summarize"))
        assert_planes(twin.summarize(chroms, starts, ends, size, zoom=False), recorded_batch(name, ks, size), (name, size, "from full"))
    beds.close()
    twin.close()


@pytest.mark.parametrize("name", sorted(FILES))
def test_drop_in_gives_the_recorded_answers(name):
    import bx.bbi.bigbed_file as drop_in

    with open(path_of(name), "rb") as f:
        bb = drop_in.BigBedFile(f)
    for k, case in enumerate(FILES[name]["cases"]):
        _, full, picked, query = recorded(name, k)
        args = (case["start"], case["end"], case["size"])
        sd = bb.summarize_from_full(case["chrom"].encode() if k % 2 else case["chrom"], *args)
        if case["none"]:
            assert sd is None and bb.summarize(case["chrom"], *args) is None and bb.query(case["chrom"], *args) is None
            continue
        assert (sd.start, sd.end, sd.size) == args
        assert_planes([getattr(sd, p) for p in M.PLANES], full, (name, case))
        assert_planes([getattr(bb.summarize(case["chrom"] if k % 2 else case["chrom"].encode(), *args), p) for p in M.PLANES], picked, (name, case, "summarize"))
        rows = bb.query(case["chrom"], *args)
        assert len(rows) == case["size"] and set(rows[0]) == set(M.QUERY_KEYS)
        assert type(rows[0]["std_dev"]) is float and all(type(rows[0][key]) is np.float64 for key in ("mean", "max", "min", "coverage"))
        for key, want in zip(M.QUERY_KEYS, query):
            assert M.same_bits([float(r[key]) for r in rows], want), (name, case, key)
    bb.close()
    assert bb.summarize_from_full("chrNone", 0, 10, 2) is None


def expected_text(name, ks, kind, full=False):
    lines = []
    for k in ks:
        case, planes, _, query = recorded(name, k)
        if case["none"]:
            cells = ["n/a"] * case["size"]
        else:
            values = M.query_region(planes, case["start"], case["end"], case["size"]) if full else query
            cells = ["%.17g" % x for x in values[KIND_ROW[kind]]]
        lines.append("\t".join([case["chrom"], str(case["start"]), str(case["end"])] + cells) + "\n")
    return "".join(lines)


@pytest.mark.parametrize("name", sorted(FILES))
def test_command_line_prints_the_recorded_values(name):
    from bxmi.cli import bigbed_summary

    cases = FILES[name]["cases"]
    kinds = ["coverage", "mean", "min", "max", "std"]
    for n_size, size in enumerate(sorted({c["size"] for c in cases})):
        ks = [k for k, c in enumerate(cases) if c["size"] == size and c["start"] <= c["end"]]  # (a BED row cannot hold start > end)
        if not ks:
            continue
        bed = "# regions\n" + "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks)
        for kind in (kinds if n_size == 0 else [kinds[n_size % len(kinds)]]):
            for full in (False, True):
                out = io.StringIO()
                argv = [path_of(name), str(size)] + (["-t", kind] if kind != "coverage" else []) + (["-f"] if full else [])
                bigbed_summary.main(argv, stdin=io.StringIO(bed), out=out)
                assert out.getvalue() == expected_text(name, ks, kind, full), (name, size, kind, full)


def test_command_line_as_a_process():
    name = "zoom.bb"
    cases = FILES[name]["cases"]
    ks = [k for k, c in enumerate(cases) if c["size"] == 100]
    assert {cases[k]["level"] for k in ks} == {None, 0, 1}
    bed = "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks) + "chrNone\t5\t9\n"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cmd = [sys.executable, "-m", "bxmi.cli.bigbed_summary", path_of(name), "100"]
    got = subprocess.run(cmd, input=bed, env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    assert got == expected_text(name, ks, "coverage") + "chrNone\t5\t9\t" + "\t".join(["n/a"] * 100) + "\n"


def test_a_level_that_is_not_ordered_is_refused(tmp_path):
    import bx.bbi.bigbed_file as drop_in
    import write_bigbed_fixture as W
    import write_bigwig_zoom_fixture as Z
    from bxmi import summary

    path = str(tmp_path / "unordered.bb")
    W.write_bigbed(path, [("chrU", 200)], [[(0, 0, 100, "u")]], [dict(reduction=8, records=Z.level_records(41, 0, 8, 0, 20)[::-1], per_block=6, fanout=3)])
    beds = summary.BedSet.from_bigbed(path)
    assert len(beds.not_ordered) == 1
    with pytest.raises(NotImplementedError, match="not ordered"):
        beds.summarize(["chrU"], [0], [160], 4)
    want = model([items_of(path)["chrU"][:2]], [0], [0], [160], 4)
    assert_planes(beds.summarize(["chrU"], [0], [160], 4, zoom=False), want, "from full")
    assert_planes(beds.summarize(["chrU"], [0], [30], 4), model([items_of(path)["chrU"][:2]], [0], [0], [30], 4), "no level picked")
    beds.close()
    with open(path, "rb") as f:
        bb = drop_in.BigBedFile(f)
    with pytest.raises(NotImplementedError, match="not ordered"):
        bb.summarize("chrU", 0, 160, 4)
    bb.close()


def items_of(path):
    from bxmi import bigbed

    return bigbed.read_items_file(path)


# ------------------------------------------------------------ a seeded differential against the model --
@pytest.mark.parametrize("size", SIZES)
def test_differential_against_the_model(size):
    from bxmi import summary

    tracks, track_of, starts, ends, want = differential_case(size)
    dev = [summary.BedTrack(*t) for t in tracks]
    assert [t.sorted for t in dev] == [True, True, True, True, False, True] and [t.n for t in dev] == [len(t[0]) for t in tracks]
    host_track_of = np.where(track_of >= len(tracks), -1, track_of)  # (the host form refuses an index beyond the list; the device form cannot)
    got = summary.summarize_beds(dev, host_track_of, starts, ends, size)
    assert_planes(got, want, size)
    assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (size, "device form"))
    # the same records as a span track with values of 1: identical planes, whichever path that takes
    spans = [summary.SpanTrack(*with_ones(t)) for t in tracks]
    assert_planes(summary.summarize(spans, host_track_of, starts, ends, size), got, (size, "span tracks of ones"))
    rows = np.nonzero(starts < ends)[0]
    mine = summary.stats(summary.Summary(*[p[rows] for p in got]), starts[rows], ends[rows], size)
    theirs = M.stats([p[rows] for p in want], starts[rows], ends[rows], size)
    for key, g, w in zip(("mean", "coverage", "std_dev"), mine, theirs):
        assert M.same_bits(g, w), (size, key)
    for t in dev + spans:
        t.close()


def test_chunk_edges():
    """runs of BD_CHUNK - 1, BD_CHUNK, BD_CHUNK + 1 and 3 BD_CHUNK + 7 records from mid-chunk, across and at an aligned boundary; a
    skipped chunk between two that count; a bin whose records all lie in the second chunk; the same records shuffled"""
    from bxmi import summary

    assert CHUNK >= 64
    seen = set()
    for label, tracks, track_of, starts, ends, size, want in chunk_cases():
        dev = [summary.BedTrack(*t) for t in tracks]
        seen.add(dev[0].sorted)
        assert_planes(summary.summarize_beds(dev, track_of, starts, ends, size), want, label)
        assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (label, "device form"))
        for t in dev:
            t.close()
    assert seen == {True, False}


def test_chunk_windows():
    """runs of more than WINDOW chunks, whose chunks the wave tests in a second and a third window: aligned and unaligned runs of
    63 to 129 chunks, chunks to stage that lie far apart in two windows, the general walk over 151 chunks, and 200 regions all over
    a track of 4097 chunks whose first record spans everything (bed_cases.window_cases)"""
    from bxmi import summary

    assert WINDOW == 64
    seen, most = set(), 0
    for label, tracks, track_of, starts, ends, size, want in window_cases():
        dev = [summary.BedTrack(*t) for t in tracks]
        seen.add(dev[0].sorted)
        most = max(most, dev[0].n)
        assert_planes(summary.summarize_beds(dev, track_of, starts, ends, size), want, label)
        assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (label, "device form"))
        for t in dev:
            t.close()
    assert seen == {True, False} and most > 64 * WINDOW * CHUNK


@pytest.mark.parametrize("size", TOP_SIZES)
def test_records_that_end_at_the_top_of_int32(size):
    """tracks whose furthest end is 2^31 - 1, regions in their last 100000 bases and up to 2^31 - 1: host and device form"""
    from bxmi import summary

    tracks, track_of, starts, ends, want = top_case(size)
    dev = [summary.BedTrack(*t) for t in tracks]
    assert [t.sorted for t in dev] == [True, True]
    assert_planes(summary.summarize_beds(dev, track_of, starts, ends, size), want, size)
    assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (size, "device form"))
    for t in dev:
        t.close()


def test_host_form_goes_through_more_than_one_slab():
    """slab + 5 rows of 3000 bins: the host form's second slab, copied back behind the first.  Every cell equals the device
    form's, which has no slabs and which the other tests of this file pin to the model; a sample of rows -- those around the slab
    edge among them, which differ pairwise -- is compared with the model itself (summary_cases.assert_slabs)"""
    from bxmi import summary

    rng = np.random.default_rng(81)
    tracks = [nested_track(rng, 3000), nested_track(rng, 3000)]
    slab, track_of, starts, ends = slab_batch(82, 1, [int(t[1].max()) for t in tracks])
    dev = [summary.BedTrack(*t) for t in tracks]
    host = summary.summarize_beds(dev, track_of, starts, ends, SLAB_SIZE)
    device = summarize_dev_raw(dev, track_of, starts, ends, SLAB_SIZE)
    assert_slabs(host, device, lambda rows: model(tracks, track_of[rows], starts[rows], ends[rows], SLAB_SIZE), slab, len(track_of))
    del host, device
    for t in dev:
        t.close()


def test_no_regions_and_bad_arguments():
    import ctypes as C

    from bxmi import _ffi as ffi
    from bxmi import summary

    t = summary.BedTrack([0, 10], [10, 20])
    none = summary.BedTrack([], [])
    assert (t.n, t.sorted, none.n, none.sorted) == (2, True, 0, True)
    res = summary.summarize_beds([t], [], [], [], 7)
    assert all(p.shape == (0, 7) and p.dtype == np.float64 for p in res)
    empty = summary.summarize_beds([], [-1, -1], [0, 5], [10, 6], 3)  # no tracks at all: empty rows
    assert_planes(empty, np.stack([empty_planes(3)] * 2, axis=1), "no tracks")
    assert_planes(summary.summarize_beds([none, t], [0, 1], [0, 0], [20, 20], 2), model([(np.zeros(0, np.int32),) * 2, ([0, 10], [10, 20])], [0, 1], [0, 0], [20, 20], 2),
                  "a track without records")
    for args, word in ((([t], [0], [0], [10], 0), "size"), (([t], [0], [0], [10], -2), "size"), (([t], [0], [-1], [10], 2), "negative"),
                       (([t], [0], [0], [-10], 2), "negative"), (([t], [1], [0], [10], 2), "track_of[0]"), (([], [0], [0], [10], 2), "track_of[0]")):
        with pytest.raises(ffi.BxmiError) as e:
            summary.summarize_beds(*args)
        assert e.value.code == EINVAL and word in str(e.value), (args[1:], str(e.value))
    with pytest.raises(ffi.BxmiError) as e:
        summary.BedTrack([5, -1], [6, 3])
    assert e.value.code == EINVAL
    handles = (C.c_void_p * 1)(t._h.value)
    for size, n, n_tracks in ((0, 1, 1), (4, -1, 1), (4, 1, -1), (4, 1, 1)):  # (the last: NULL arrays)
        with pytest.raises(ffi.BxmiError) as e:
            ffi.call("bxmi_beds_summarize_dev", handles, n_tracks, None, None, None, n, size, None, None, None, None, None, None)
        assert e.value.code == EINVAL
    ffi.call("bxmi_beds_summarize_dev", handles, 1, None, None, None, 0, 4, None, None, None, None, None, None)  # n == 0: no launch
    # entries the device form cannot refuse are empty rows: a track index beyond the list, a negative coordinate
    odd = summarize_dev_raw([t], [9, 0, 0, 0], [0, -5, 0, 0], [50, 50, -1, 20], 4)
    assert_planes([p[:3] for p in odd], np.stack([empty_planes(4)] * 3, axis=1), "rows the device form cannot refuse")
    assert odd[0][3].tolist() == [5.0, 5.0, 5.0, 5.0]
    t.close()
    none.close()


def test_summarize_beds_dev_on_torch_tensors():
    """summarize_beds_dev on torch tensors -- the recorded straddle file, a seeded batch on slices that start 4 bytes into their
    allocation, torch's current stream and a stream of the caller's, an empty batch, the torch form of stats -- in a process of its
    own: torch brings its own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import summary_model as M
from bed_cases import FILES, by_size, differential_case, path_of, recorded_batch
from bxmi import summary

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

name = "straddle.bb"
tracks = summary.BedTrack.from_bigbed(path_of(name))
for size, ks, track_of, starts, ends in by_size(name):
    res = summary.summarize_beds_dev(tracks.values(), *[dev_i32(np.array(a), 0) for a in (track_of, starts, ends)], size)
    torch.cuda.synchronize()
    want = recorded_batch(name, ks, size)
    query = recorded_batch(name, ks, size, which=3)
    for p, g, w in zip(M.PLANES, res, want):
        assert g.dtype == torch.float64 and M.same_bits(g.cpu().numpy(), w), (name, size, p)
    mean, coverage, std = summary.stats(res, dev_i32(np.array(starts), 0), dev_i32(np.array(ends), 0), size)
    for key, g, w in (("mean", mean, query[0]), ("coverage", coverage, query[3]), ("std_dev", std, query[4])):
        assert g.is_cuda and M.same_bits(g.cpu().numpy(), w), (name, size, key)
for t in tracks.values():
    t.close()

size = 65
tracks, track_of, starts, ends, want = differential_case(size)
dev = [summary.BedTrack(*t) for t in tracks]
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
assert all(x.data_ptr() % 16 for x in d)
torch.cuda.synchronize()

def same(res, what):
    for p, g, w in zip(M.PLANES, res, want):
        assert M.same_bits(g.cpu().numpy(), w), (what, p)

res = summary.summarize_beds_dev(dev, *d, size)
torch.cuda.synchronize()
same(res, "current stream")
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    res = summary.summarize_beds_dev(dev, *d, size)
side.synchronize()
same(res, "side stream")
res = summary.summarize_beds_dev(dev, d[0][:0], d[1][:0], d[2][:0], size, stream=side.cuda_stream)
side.synchronize()
assert all(tuple(g.shape) == (0, size) for g in res)
try:
    summary.summarize_beds_dev(dev, d[0].cpu(), d[1].cpu(), d[2].cpu(), size)
    raise SystemExit("host tensors were accepted")
except ValueError:
    pass
for t in dev:
    t.close()
print("summarize_beds_dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "summarize_beds_dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
