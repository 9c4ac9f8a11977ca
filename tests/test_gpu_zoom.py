"""
bigWig summaries answered from zoom levels on the device (bxmi_zoom_*, bxmi.summary.ZoomTrack / summarize_zoom / summarize_zoom_dev /
TrackSet, bx.bbi.bigwig_file.BigWigFile(use_zoom=True), bxmi.cli.bigwig_summary -z) against the results recorded from the reference
(tests/golden/zoom) and, beyond them, against tests/zoom_model.py -- itself pinned to those results by
tests/test_zoom_model_golden.py.  Every comparison is byte for byte, NaN compared as NaN, except where the reference's own tests
compare with a tolerance: those use the reference's.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import zoom_model as M
from summary_cases import SLAB_SIZE, TOP_SIZES, assert_slabs, slab_batch
from zoom_cases import (CHUNK, FILES, GOLDEN, SIZES, assert_planes, chunk_level, differential_case, empty_planes, levels, path_of, random_level, recorded, top_case,
                        zoom_cases)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_zoom_summarize_dev",)
EINVAL = 1
KIND_ROW = {"mean": 0, "max": 1, "min": 2, "coverage": 3, "std": 4}  # rows of the recorded query arrays (QUERY_KEYS)


def want_planes(name, ks):
    cases = FILES[name]["cases"]
    return np.stack([recorded(name, k)[1] if not cases[k]["none"] else empty_planes(cases[k]["size"]) for k in ks], axis=1)


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", sorted(FILES))
def test_summarize_zoom_gives_the_recorded_arrays(name):
    """all zoom regions of one file that share a size go through ONE call whose table lists every (chromosome, level) track"""
    from bxmi import summary

    per_chrom = summary.ZoomTrack.from_bigwig(path_of(name))
    order = list(per_chrom)
    n_levels = len(FILES[name]["reductions"])
    tracks = [t for chrom in order for t in per_chrom[chrom]]
    assert len(tracks) == len(order) * n_levels
    for (chrom, k), t in zip(((c, k) for c in order for k in range(n_levels)), tracks):
        z = levels(name)[k][1][chrom]
        assert (t.n, t.n_leaves) == (len(z.start), len(z.leaf_lo))
    cases = FILES[name]["cases"]
    for size in sorted({cases[k]["size"] for k in zoom_cases(name)}):
        ks = [k for k in zoom_cases(name) if cases[k]["size"] == size]
        rows = [cases[k] for k in ks]
        track_of = [order.index(c["chrom"]) * n_levels + c["level"] for c in rows]
        got = summary.summarize_zoom(tracks, track_of, [c["start"] for c in rows], [c["end"] for c in rows], size)
        assert_planes(got, want_planes(name, ks), (name, size))
    for t in tracks:
        t.close()


@pytest.mark.parametrize("name", sorted(FILES))
def test_track_set_answers_mixed_batches_as_the_reference(name):
    """every case of a file that shares a size in one TrackSet.summarize: rows from different levels, rows from full data and rows
    the reference answers with None; zoom=False is the full-data answer, which these files' levels contradict"""
    from bxmi import summary

    ts = summary.TrackSet.from_bigwig(path_of(name))
    assert ts.reductions == FILES[name]["reductions"] and not ts.not_ordered
    cases = FILES[name]["cases"]
    for size in sorted({c["size"] for c in cases}):
        ks = [k for k, c in enumerate(cases) if c["size"] == size]
        rows = [cases[k] for k in ks]
        args = ([c["chrom"] for c in rows], [c["start"] for c in rows], [c["end"] for c in rows], size)
        got = ts.summarize(*args)
        assert_planes(got, want_planes(name, ks), (name, size))
        index = np.array([ts.chroms.index(c["chrom"]) if c["chrom"] in ts.chroms else -1 for c in rows])
        assert_planes(ts.summarize(index, *args[1:], zoom=True), got, (name, size, "chromosomes by position"))
        full = ts.summarize(*args, zoom=False)
        assert_planes(full, summary.summarize(ts.spans.values(), index, *args[1:]), (name, size, "zoom=False"))
        zoomed = [i for i, c in enumerate(rows) if c["level"] is not None]
        if name != "test.bw" and zoomed:
            assert not all(M.same_bits(a[zoomed], b[zoomed]) for a, b in zip(full, got)), (name, size)
    ts.close()


@pytest.mark.parametrize("name", sorted(FILES))
def test_drop_in_with_use_zoom_gives_the_recorded_answers(name):
    import bx.bbi.bigwig_file as drop_in

    with open(path_of(name), "rb") as f:
        bw = drop_in.BigWigFile(f, use_zoom=True)
        f.seek(0)
        plain = drop_in.BigWigFile(f)
    for k, case in enumerate(FILES[name]["cases"]):
        _, planes, query = recorded(name, k)
        args = (case["start"], case["end"], case["size"])
        chrom = case["chrom"].encode() if k % 2 else case["chrom"]
        if case["none"]:
            assert bw.summarize(chrom, *args) is None and bw.query(chrom, *args) is None
            continue
        sd = bw.summarize(chrom, *args)
        assert (sd.start, sd.end, sd.size) == args
        assert_planes([getattr(sd, p) for p in M.PLANES], planes, (name, case))
        rows = bw.query(chrom, *args)
        assert len(rows) == case["size"] and set(rows[0]) == set(M.QUERY_KEYS)
        for key, want in zip(M.QUERY_KEYS, query):
            assert M.same_bits([float(r[key]) for r in rows], want), (name, case, key)
        if case["level"] is not None:  # without the keyword nothing has changed
            with pytest.raises(NotImplementedError, match="summarize_from_full"):
                plain.summarize(chrom, *args)
            with pytest.raises(NotImplementedError, match="summarize_from_full"):
                plain.query(chrom, *args)
    bw.close()
    plain.close()


def expected_text(name, ks, kind):
    lines = []
    for k in ks:
        case, _, query = recorded(name, k)
        cells = ["n/a"] * case["size"] if case["none"] else ["%.17g" % x for x in query[KIND_ROW[kind]]]
        lines.append("\t".join([case["chrom"], str(case["start"]), str(case["end"])] + cells) + "\n")
    return "".join(lines)


@pytest.mark.parametrize("name", sorted(FILES))
def test_command_line_with_z_prints_the_recorded_values(name):
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
            bigwig_summary.main([path_of(name), str(size), "-z"] + (["-t", kind] if kind != "mean" else []), stdin=io.StringIO(bed), out=out)
            assert out.getvalue() == expected_text(name, ks, kind), (name, size, kind)
    # without -z: the answer from full data, as before
    ks = [k for k in zoom_cases(name) if cases[k]["size"] == cases[zoom_cases(name)[0]]["size"]]
    bed = "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks)
    out = io.StringIO()
    bigwig_summary.main([path_of(name), str(cases[ks[0]]["size"]), "-t", "max"], stdin=io.StringIO(bed), out=out)
    if name != "test.bw":
        assert out.getvalue() != expected_text(name, ks, "max")
    assert "nan" not in out.getvalue()  # full data has no NaN max: an empty bin there is -inf


def test_command_line_with_z_as_a_process():
    name = "leaves.bw"
    cases = FILES[name]["cases"]
    ks = [k for k, c in enumerate(cases) if c["size"] == 64]
    bed = "".join("%s\t%d\t%d\n" % (cases[k]["chrom"], cases[k]["start"], cases[k]["end"]) for k in ks) + "chrNone\t5\t9\n"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cmd = [sys.executable, "-m", "bxmi.cli.bigwig_summary", path_of(name), "64", "-z", "-t", "std"]
    got = subprocess.run(cmd, input=bed, env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    assert got == expected_text(name, ks, "std") + "chrNone\t5\t9\t" + "\t".join(["n/a"] * 64) + "\n"


# ------------------------------------------------------------ the reference's own tests --
def allclose(a, b, tol=0.00001):
    """bigwig_tests.py:17-22: like numpy.allclose but NaN == NaN"""
    d = np.absolute(np.asarray(a) - np.asarray(b))
    return bool(np.all(np.isnan(d) | (d < tol)))


@pytest.fixture(scope="module")
def reference_file():
    import bx.bbi.bigwig_file as drop_in

    with open(path_of("test.bw"), "rb") as f:
        bw = drop_in.BigWigFile(f, use_zoom=True)
    yield bw
    bw.close()


def test_expectation_file_line_by_line(reference_file):
    """bigwig_tests.py:88-107 over the reference's test.expectation, through the drop-in"""
    with open(os.path.join(GOLDEN, "test.expectation")) as f:
        lines = f.readlines()
    assert len(lines) == 24
    checked = set()
    for line in lines:
        fields = line.split()
        chrom, start, end, n, t = fields[0], int(fields[1]), int(fields[2]), int(fields[3]), fields[4]
        values = [float(v.replace("n/a", "NaN")) for v in fields[5:]]
        with np.errstate(all="ignore"):
            sd = reference_file.summarize(chrom, start, end, n)
            if t == "mean":
                assert allclose(sd.sum_data / sd.valid_count, values), line[:60]
            elif t == "min":
                assert allclose(sd.min_val, values), line[:60]
            elif t == "max":
                assert allclose(sd.max_val, values), line[:60]
        checked.add(t)
    assert {"mean", "min", "max"} <= checked


MEANS = [-0.17557571594973645, -0.054009292602539061, -0.056892242431640622, -0.03650328826904297, 0.036112907409667966, 0.0064466032981872557,
         0.036949024200439454, 0.076638259887695306, 0.043518108367919923, 0.01554749584197998]


def test_constants_of_the_references_tests(reference_file):
    """bigwig_tests.py:29-87: numpy.allclose for the means, equality for min and max"""
    bw = reference_file
    assert np.allclose([float(x["mean"]) for x in bw.query("chr1", 10000, 20000, 10)], MEANS)
    sd = bw.summarize("chr1", 10000, 20000, 10)
    assert np.allclose(sd.sum_data / sd.valid_count, MEANS)
    data = bw.query("chr1", 10000, 20000, 1)
    assert [float(x["max"]) for x in data] == [0.289000004529953] and [float(x["min"]) for x in data] == [-3.9100000858306885]
    leaf = bw.query("chr1", 11000, 11005, 5)
    assert np.allclose([float(x["mean"]) for x in leaf], [0.050842501223087311, -2.4589500427246094, 0.050842501223087311, 0.050842501223087311,
                                                         0.050842501223087311])
    data = bw.query("chr1", 11000, 11005, 1)
    assert [float(x["max"]) for x in data] == [0.050842501223087311] and [float(x["min"]) for x in data] == [-2.4589500427246094]
    assert bw.query("chr2", 0, 10000, 10) is None


def test_without_the_keyword_the_drop_in_still_raises():
    import bx.bbi.bigwig_file as drop_in

    with open(path_of("test.bw"), "rb") as f:
        bw = drop_in.BigWigFile(f)
    assert bw.use_zoom is False
    with pytest.raises(NotImplementedError, match="summarize_from_full"):
        bw.summarize("chr1", 10000, 20000, 10)
    with pytest.raises(NotImplementedError, match="summarize_from_full"):
        bw.query("chr1", 10000, 20000, 10)
    assert bw.summarize_from_full("chr1", 10000, 20000, 10).valid_count.sum() > 0
    bw.close()


# ------------------------------------------------------------ a seeded differential against the model --
@pytest.mark.parametrize("size", SIZES)
def test_differential_against_the_model(size):
    """several tracks and levels in one call"""
    from bxmi import summary

    tracks, track_of, starts, ends, want = differential_case(size)
    dev = [summary.ZoomTrack(z) for z in tracks]
    assert [(t.n, t.n_leaves) for t in dev] == [(len(z.start), len(z.leaf_lo)) for z in tracks]
    assert_planes(summary.summarize_zoom(dev, track_of, starts, ends, size), want, size)
    for t in dev:
        t.close()


def test_chunk_boundaries_carry_the_accumulators():
    """one bin over runs around the chunk size: a wave that dropped its accumulators between chunks would lose all but the last"""
    from bxmi import summary

    track = chunk_level()
    runs = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7, 4 * CHUNK + 63]
    starts = np.array([3 * 7 + 1] * len(runs), dtype=np.int32)  # (the first record is overlapped in 2 of its 3 bases)
    ends = (3 * 7 + 3 * np.array(runs)).astype(np.int32)
    zeros = np.zeros(len(runs), dtype=np.int32)
    t = summary.ZoomTrack(track)
    for size in (1, 2, 3):
        assert_planes(summary.summarize_zoom([t], zeros, starts, ends, size), M.summarize([track], zeros, starts, ends, size), size)
    t.close()


def summarize_dev_raw(tracks, track_of, starts, ends, size):
    """bxmi_zoom_summarize_dev on arrays in device memory, on the null stream -> five [n, size] numpy arrays"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    rows = [ffi.DeviceArray.from_numpy(np.asarray(a, dtype=np.int32)) for a in (track_of, starts, ends)]
    planes = [ffi.DeviceArray(8 * n * size) for _ in range(5)]
    ffi.call("bxmi_zoom_summarize_dev", ffi.handles(tracks), len(tracks), *[a.ptr for a in rows], n, size, *[a.ptr for a in planes], None)
    ffi.call("bxmi_synchronize", None)
    out = [a.to_numpy(np.float64, n * size).reshape(n, size) for a in planes]
    for a in rows + planes:
        a.free()
    return out


def test_device_form_and_its_unchecked_rows():
    """the device form equals the host form; rows it cannot refuse -- a track beyond the list, a negative coordinate -- are empty
    rows; 9 tracks take two launches of the table kernel, and the spare entry behind them arrives"""
    from bxmi import summary

    size = 65
    tracks, track_of, starts, ends, want = differential_case(size)
    dev = [summary.ZoomTrack(z) for z in tracks]
    assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, "device form")
    odd = summarize_dev_raw(dev, [len(dev), 0, 0, 3], [0, -5, 0, 0], [50, 50, -1, 30], 4)
    want_odd = M.summarize(tracks, [-1, -1, -1, 3], [0, 0, 0, 0], [50, 50, 50, 30], 4)
    assert_planes(odd, want_odd, "rows the device form cannot refuse")
    assert_planes([p[:3] for p in odd], np.stack([empty_planes(4)] * 3, axis=1), "empty rows")
    many = dev[:4] + dev[:4] + [dev[3]]
    got = summarize_dev_raw(many, [8, 9, 4, -1], [0, 0, 600, 0], [30, 30, 2600, 30], 4)
    assert_planes(got, M.summarize(tracks, [3, -1, 0, -1], [0, 0, 600, 0], [30, 30, 2600, 30], 4), "nine tracks")
    for t in dev:
        t.close()


@pytest.mark.parametrize("size", TOP_SIZES)
def test_records_that_end_at_the_top_of_int32(size):
    """a level whose last record and last leaf end at 2^31 - 1, regions in its last 100000 bases and up to 2^31 - 1: host and
    device form"""
    from bxmi import summary

    tracks, track_of, starts, ends, want = top_case(size)
    dev = [summary.ZoomTrack(z) for z in tracks]
    assert_planes(summary.summarize_zoom(dev, track_of, starts, ends, size), want, size)
    assert_planes(summarize_dev_raw(dev, track_of, starts, ends, size), want, (size, "device form"))
    for t in dev:
        t.close()


def test_host_form_goes_through_more_than_one_slab():
    """slab + 5 rows of 3000 bins: the host form's second slab, copied back behind the first.  Every cell equals the device
    form's, which has no slabs and which the other tests of this file pin to the model; a sample of rows -- those around the slab
    edge among them, which differ pairwise -- is compared with the model itself (summary_cases.assert_slabs)"""
    from bxmi import summary

    rng = np.random.default_rng(85)
    tracks = [random_level(rng, 3000, 16), random_level(rng, 3000, 16, first=300)]
    slab, track_of, starts, ends = slab_batch(86, 1, [int(z.end.max()) for z in tracks])
    dev = [summary.ZoomTrack(z) for z in tracks]
    host = summary.summarize_zoom(dev, track_of, starts, ends, SLAB_SIZE)
    device = summarize_dev_raw(dev, track_of, starts, ends, SLAB_SIZE)
    assert_slabs(host, device, lambda rows: M.summarize(tracks, track_of[rows], starts[rows], ends[rows], SLAB_SIZE), slab, len(track_of))
    del host, device
    for t in dev:
        t.close()


def test_no_regions_bad_arguments_and_levels_that_are_not_ordered():
    from bxmi import _ffi as ffi
    from bxmi import bigwig, summary

    t = summary.ZoomTrack(chunk_level())
    res = summary.summarize_zoom([t], [], [], [], 7)
    assert all(p.shape == (0, 7) and p.dtype == np.float64 for p in res)
    none = summary.summarize_zoom([], [-1, -1], [0, 5], [10, 6], 3)  # no tracks at all: empty rows
    assert_planes(none, np.stack([empty_planes(3)] * 2, axis=1), "no tracks")
    for args, word in ((([t], [0], [0], [10], 0), "size"), (([t], [0], [-1], [10], 2), "negative"), (([t], [1], [0], [10], 2), "track_of[0]")):
        with pytest.raises(ffi.BxmiError) as e:
            summary.summarize_zoom(*args)
        assert e.value.code == EINVAL and word in str(e.value), (args[1:], str(e.value))
    t.close()
    (_, per), = bigwig.read_zoom_file(os.path.join(GOLDEN, "unordered.z.bw"))
    with pytest.raises(ffi.BxmiError) as e:
        summary.ZoomTrack(per["chrU"])
    assert e.value.code == EINVAL and "record starts are not non-decreasing" in str(e.value)
    ts = summary.TrackSet.from_bigwig(os.path.join(GOLDEN, "unordered.z.bw"))
    assert ts.zoom == [None] and 0 in ts.not_ordered
    with pytest.raises(NotImplementedError, match="summarize_from_full"):
        ts.summarize(["chrU"], [0], [160], 4)
    full = ts.summarize(["chrU", "chrU"], [0, 0], [160, 40], 4, zoom=False)  # full data answers; so does a row that picks no level
    assert_planes(ts.summarize(["chrU"], [0], [40], 4), [p[1:] for p in full], "a row without a level")
    assert full.valid_count[0].tolist() == [40.0, 40.0, 20.0, 0.0]
    ts.close()


# ------------------------------------------------------------ device entry point --
def test_summarize_zoom_dev_equals_summarize_zoom_and_the_recorded_arrays():
    """summarize_zoom_dev on torch tensors -- every recorded zoom case, a seeded batch on slices that start 4 bytes into their
    allocation, torch's current stream and a stream of the caller's, an empty batch -- in a process of its own: torch brings its own
    HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import zoom_model as M
from zoom_cases import FILES, differential_case, path_of, recorded, zoom_cases
from bxmi import summary

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

checked = 0
for name in sorted(FILES):
    per_chrom = summary.ZoomTrack.from_bigwig(path_of(name))
    order = list(per_chrom)
    n_levels = len(FILES[name]["reductions"])
    tracks = [t for chrom in order for t in per_chrom[chrom]]
    cases = FILES[name]["cases"]
    for size in sorted({cases[k]["size"] for k in zoom_cases(name)}):
        ks = [k for k in zoom_cases(name) if cases[k]["size"] == size]
        rows = [cases[k] for k in ks]
        args = [np.array(x) for x in ([order.index(c["chrom"]) * n_levels + c["level"] for c in rows], [c["start"] for c in rows], [c["end"] for c in rows])]
        res = summary.summarize_zoom_dev(tracks, *[dev_i32(a, 0) for a in args], size)
        torch.cuda.synchronize()
        want = np.stack([recorded(name, k)[1] for k in ks], axis=1)
        for p, g, w in zip(M.PLANES, res, want):
            assert g.dtype == torch.float64 and M.same_bits(g.cpu().numpy(), w), (name, size, p)
        checked += len(ks)
    for t in tracks:
        t.close()
assert checked >= 40, checked

size = 64
tracks, track_of, starts, ends, want = differential_case(size)
dev = [summary.ZoomTrack(z) for z in tracks]
host = summary.summarize_zoom(dev, track_of, starts, ends, size)
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
assert all(x.data_ptr() % 16 for x in d)
torch.cuda.synchronize()

def same(res, what):
    for p, g, h, w in zip(M.PLANES, res, host, want):
        assert M.same_bits(g.cpu().numpy(), h) and M.same_bits(h, w), (what, p)

res = summary.summarize_zoom_dev(dev, *d, size)
torch.cuda.synchronize()
same(res, "current stream")
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    res = summary.summarize_zoom_dev(dev, *d, size)
side.synchronize()
same(res, "side stream")
res = summary.summarize_zoom_dev(dev, d[0][:0], d[1][:0], d[2][:0], size, stream=side.cuda_stream)
side.synchronize()
assert all(tuple(g.shape) == (0, size) for g in res)
for t in dev:
    t.close()
print("summarize_zoom_dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "summarize_zoom_dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
