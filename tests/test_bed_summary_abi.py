"""CPU-only: the bed-track entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so, with the shape of
the span-track ones; their arguments are checked before any device call; bed_summary.hpp is compiled inside summary.hip under the
pragma that turns contraction off and has no value array; the chunk size is where the tests read it; the Python layers, the drop-in
and the command line import without a device; the drop-in's ``get`` -- host code -- gives the recorded lists."""
import ctypes as C
import os
import re

import pytest

from bed_cases import CHUNK, FILES, ROOT, path_of

NAMES = ("bxmi_beds_create", "bxmi_beds_destroy", "bxmi_beds_info", "bxmi_beds_summarize", "bxmi_beds_summarize_dev")
CSRC = os.path.join(ROOT, "bx-python_amd", "csrc")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    top = header.split("#ifndef BXMI_H")[0]
    assert "lib/bx/bbi/bigbed_file.pyx" in top and "bxmi_beds_*" in top  # the reference mapping of the top comment
    for name in NAMES:
        assert name in _ffi.EXPORTED and hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(re.findall(r",", decl)) + 1 == len(_ffi._SIGNATURES[name]), name
    host, dev = _ffi._SIGNATURES["bxmi_beds_summarize"], _ffi._SIGNATURES["bxmi_beds_summarize_dev"]
    assert dev[:-1] == host and dev[-1] is C.c_void_p
    assert host == _ffi._SIGNATURES["bxmi_spans_summarize"] and dev == _ffi._SIGNATURES["bxmi_spans_summarize_dev"]  # the same shape
    decl = re.search(r"int bxmi_beds_summarize_dev\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl).strip().endswith("void *stream")
    assert re.findall(r"double \*(\w+)", decl) == ["valid", "min", "max", "sum", "sumsq"]
    assert "value" not in re.search(r"int bxmi_beds_create\(([^;]*)\);", header).group(1)


def test_arguments_are_checked_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    for n, size in ((1, 0), (1, -4), (-1, 5)):
        assert lib.bxmi_beds_summarize(None, 0, None, None, None, n, size, None, None, None, None, None) == _ffi.EINVAL
        assert lib.bxmi_beds_summarize_dev(None, 0, None, None, None, n, size, None, None, None, None, None, None) == _ffi.EINVAL
    assert lib.bxmi_beds_summarize(None, 1, None, None, None, 1, 5, None, None, None, None, None) == _ffi.EINVAL  # a NULL track list
    handles = (C.c_void_p * 1)(None)
    assert lib.bxmi_beds_summarize(handles, 1, None, None, None, 1, 5, None, None, None, None, None) == _ffi.EINVAL
    assert b"NULL handle" in lib.bxmi_last_error()
    assert lib.bxmi_beds_summarize(None, 0, None, None, None, 0, 5, None, None, None, None, None) == _ffi.OK  # n == 0: nothing to do
    assert lib.bxmi_beds_info(None, None, None) == _ffi.EINVAL
    # a region with a negative coordinate, a row naming a track beyond the list: refused by the host form before any device call
    planes = [(C.c_double * 2)() for _ in range(5)]
    row = lambda *v: (C.c_int32 * 1)(*v)  # noqa: E731
    for track_of, start, end, word in ((-1, -1, 10, b"negative"), (-1, 0, -10, b"negative"), (0, 0, 10, b"track_of[0]")):
        assert lib.bxmi_beds_summarize(None, 0, row(track_of), row(start), row(end), 1, 2, *planes) == _ffi.EINVAL
        assert word in lib.bxmi_last_error()
    out = C.c_void_p()
    bad = (C.c_int32 * 2)(4, -1)
    fine = (C.c_int32 * 2)(5, 9)
    assert lib.bxmi_beds_create(bad, fine, 2, C.byref(out)) == _ffi.EINVAL and b"negative" in lib.bxmi_last_error() and not out.value
    assert lib.bxmi_beds_create(fine, bad, 2, C.byref(out)) == _ffi.EINVAL
    assert lib.bxmi_beds_create(fine, fine, -1, C.byref(out)) == _ffi.EINVAL and lib.bxmi_beds_create(None, None, 1, C.byref(out)) == _ffi.EINVAL
    assert lib.bxmi_beds_create(fine, fine, 2, None) == _ffi.EINVAL
    assert lib.bxmi_beds_destroy(None) == _ffi.OK


def test_header_is_compiled_in_the_summary_unit_without_contraction():
    unit = open(os.path.join(CSRC, "summary.hip")).read()
    assert unit.index("#pragma clang fp contract(off)") < unit.index('#include "summary.hpp"') < unit.index('#include "bed_summary.hpp"')
    text = open(os.path.join(CSRC, "bed_summary.hpp")).read()
    assert "contract" in text.lower()
    track = re.search(r"struct BdTrack \{(.*?)\};", text, re.S).group(1)
    assert "float" not in track and "value" not in track and re.findall(r"\*(\w+);", track) == ["start", "end", "reach", "creach"]
    kernel = text[text.index("void bd_summary_kernel"):]
    assert "float " not in kernel and "l_val" not in kernel  # no value array exists or is read


def test_chunk_constant_is_where_the_tests_read_it():
    assert CHUNK % 64 == 0 and 64 <= CHUNK <= 1024  # whole waves of loads; a few KiB of LDS


def test_layers_import_without_a_device():
    import bx.bbi.bigbed_file as drop_in
    from bxmi import bigbed, summary
    from bxmi.cli import bigbed_summary

    assert callable(summary.summarize_beds) and callable(summary.summarize_beds_dev) and callable(summary.BedTrack.from_bigbed)
    assert callable(summary.BedSet.from_bigbed) and callable(summary.BedSet.summarize) and callable(summary.TrackSet.summarize)
    assert callable(bigbed.read_items_file) and callable(bigbed.read_zoom_file)
    assert callable(bigbed_summary.main) and bigbed_summary.KINDS[0] == "coverage" and set(bigbed_summary.KINDS) == {"coverage", "mean", "min", "max", "std"}
    for method in ("open", "close", "summarize", "summarize_from_full", "query", "get"):
        assert callable(getattr(drop_in.BigBedFile, method)), method


@pytest.mark.parametrize("name", sorted(n for n in FILES if FILES[n]["gets"]))
def test_drop_in_get_gives_the_recorded_lists(name):
    """host code: with a bytes chromosome -- all the reference takes -- every interval's chrom, start, end, strand and fields are the
    recorded ones, the bytes-chrom quirk included; with str the same records, their chromosome a str"""
    import bx.bbi.bigbed_file as drop_in
    from bx.intervals.io import GenomicInterval

    with open(path_of(name), "rb") as f:
        bb = drop_in.BigBedFile(f)
    for entry in FILES[name]["gets"]:
        args = (entry["start"], entry["end"])
        got, as_str = bb.get(entry["chrom"].encode(), *args), bb.get(entry["chrom"], *args)
        if entry["rows"] is None:
            assert got is None and as_str is None, entry
            continue
        assert len(got) == len(as_str) == len(entry["rows"]) and all(isinstance(iv, GenomicInterval) for iv in got), entry
        for iv, other, want in zip(got, as_str, entry["rows"]):
            assert (repr(iv.chrom), iv.start, iv.end, iv.strand, iv.fields) == (want["chrom"], want["start"], want["end"], want["strand"], want["fields"])
            assert isinstance(iv.chrom, bytes) and iv.fields[0] == "b'%s'" % entry["chrom"]
            assert (other.chrom, other.start, other.end, other.strand, other.fields[1:]) == (entry["chrom"], iv.start, iv.end, iv.strand, iv.fields[1:])
    assert bb.zoom_levels == len(FILES[name]["reductions"])
    with pytest.raises(OverflowError):
        bb.get("chrA", -1, 10)
    with pytest.raises(OverflowError):
        bb.summarize_from_full("chrA", 0, 2 ** 32, 10)
    with pytest.raises(ValueError):
        bb.query("chrA", 0, 2 ** 31, 10)
    with pytest.raises(ValueError):
        bb.query("chrA", -1, 10, 10)
    assert bb.summarize("chrNone", 0, 100, 5) is None and bb.query(b"chrNone", 0, 100, 5) is None and bb.summarize_from_full("chrA", 5, 5, 1) is None


def test_get_includes_what_the_reference_includes():
    """records are not clipped; a zero-length record strictly inside the region is included, one at its edge is not"""
    import bx.bbi.bigbed_file as drop_in

    with open(path_of("genes.bb"), "rb") as f:
        bb = drop_in.BigBedFile(f)
    assert [(iv.start, iv.end) for iv in bb.get("chrA", 124, 126)] == [(120, 980), (120, 400), (120, 131), (125, 125)]
    assert (125, 125) not in [(iv.start, iv.end) for iv in bb.get("chrA", 125, 126)]
    assert [iv.fields[3:] for iv in bb.get("chrBB", 41, 42)] == [["geneD", "100", "-"], [""]]
