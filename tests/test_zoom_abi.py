"""CPU-only: the zoom-track entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; the device
variant has the host form's arguments followed by the stream; the kernel's header is compiled inside summary.hip, under its
contraction pragma; bxmi_zoom_create refuses, before any device call, every level that is not ordered -- each condition on its own
-- and bxmi_zoom_summarize* check their arguments as bxmi_spans_summarize* do; the Python layers, the drop-in's keyword and the
command line's flag exist without a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bxmi_zoom_create", "bxmi_zoom_destroy", "bxmi_zoom_info", "bxmi_zoom_summarize", "bxmi_zoom_summarize_dev")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    top = header.split("#ifndef BXMI_H")[0]
    assert "cirtree_file.pyx" in top and "bxmi_zoom_*" in top  # the reference mapping of the top comment
    for name in NAMES:
        assert name in _ffi.EXPORTED and hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(re.findall(r",", decl)) + 1 == len(_ffi._SIGNATURES[name]), name
    host, dev = _ffi._SIGNATURES["bxmi_zoom_summarize"], _ffi._SIGNATURES["bxmi_zoom_summarize_dev"]
    assert dev[:-1] == host and dev[-1] is C.c_void_p
    assert host == _ffi._SIGNATURES["bxmi_spans_summarize"] and dev == _ffi._SIGNATURES["bxmi_spans_summarize_dev"]  # the same shape
    decl = re.search(r"int bxmi_zoom_summarize_dev\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl).strip().endswith("void *stream")
    assert [w for w in re.findall(r"double \*(\w+)", decl)] == ["valid", "min", "max", "sum", "sumsq"]


def test_kernel_header_is_compiled_without_contraction():
    unit = open(os.path.join(ROOT, "bx-python_amd", "csrc", "summary.hip")).read()
    assert unit.index("#pragma clang fp contract(off)") < unit.index('#include "summary.hpp"') < unit.index('#include "zoom_summary.hpp"')
    text = open(os.path.join(ROOT, "bx-python_amd", "csrc", "zoom_summary.hpp")).read()
    assert "contract" in text.lower() and "as_global(" in text
    m = re.search(r"constexpr int ZM_CHUNK = (\d+);", text)
    assert m and int(m.group(1)) % 64 == 0 and 64 <= int(m.group(1)) <= 1024  # whole waves of loads; a few KiB of LDS


def level(n=4, n_leaves=2):
    """an ordered level of n records in n_leaves leaves, as the arguments of bxmi_zoom_create (numpy arrays)"""
    start = np.arange(n, dtype=np.int32) * 10
    first = np.linspace(0, n, n_leaves + 1).astype(np.int64)
    return dict(start=start, end=start + 10, valid=np.full(n, 10, dtype=np.uint32), min=np.zeros(n, np.float32), max=np.ones(n, np.float32),
                sum=np.ones(n, np.float32), sumsq=np.ones(n, np.float32), leaf_lo=start[first[:-1]].copy(), leaf_hi=(start + 10)[first[1:] - 1].copy(),
                leaf_first=first, n=n, n_leaves=n_leaves)


def create(a, out=True):
    from bxmi import _ffi

    lib = _ffi.load()
    h = C.c_void_p()
    rc = lib.bxmi_zoom_create(*[_ffi.ptr(a[k]) for k in ("start", "end", "valid", "min", "max", "sum", "sumsq")], a["n"],
                              _ffi.ptr(a["leaf_lo"]), _ffi.ptr(a["leaf_hi"]), _ffi.ptr(a["leaf_first"]), a["n_leaves"], C.byref(h) if out else None)
    return rc, lib.bxmi_last_error().decode()


def test_create_refuses_each_condition_on_its_own():
    """every refusal comes before the first device call, so none of this needs a device"""
    from bxmi import _ffi

    def broken(key, index, value):
        a = level()
        a[key][index] = value
        return create(a)

    # (each change breaks ONE condition: the comments say why the others still hold)
    for (key, index, value), word in (
            (("start", 2, 5), "record starts are not non-decreasing"),   # 0, 10, 5, 30: ends 10 .. 40 still rise, 5 <= 30
            (("end", 1, 5), "start > end"),                              # [10, 5)
            (("end", 2, 25), "record ends are not non-decreasing"),      # ends 10, 20, 25, 40 rise ... see below
            (("start", 0, -3), "negative coordinate"),
            (("leaf_lo", 1, -5), "negative coordinate"),
            (("leaf_hi", 0, 50), "leaf_hi is not non-decreasing"),       # 50, 40
            (("leaf_lo", 0, 30), "leaf_lo is not non-decreasing"),       # 30, 20
            (("leaf_first", 0, 1), "leaf_first"),
            (("leaf_first", 2, 3), "leaf_first"),
            (("leaf_first", 1, 5), "leaf_first")):
        if (key, index, value) == ("end", 2, 25):
            a = level()
            a["end"][:] = (10, 30, 25, 40)  # starts 0 .. 30 rise, every start <= end, the ends do not
            rc, message = create(a)
        else:
            rc, message = broken(key, index, value)
        assert rc == _ffi.EINVAL and word in message, ((key, index, value), message)
    a = level()
    assert create(a, out=False)[0] == _ffi.EINVAL
    for key in ("start", "sumsq", "leaf_hi", "leaf_first"):
        a = level()
        a[key] = None
        assert create(a)[0] == _ffi.EINVAL, key
    lib = _ffi.load()
    assert lib.bxmi_zoom_create(None, None, None, None, None, None, None, -1, None, None, _ffi.ptr(np.zeros(1, np.int64)), 0, C.byref(C.c_void_p())) == _ffi.EINVAL
    assert lib.bxmi_zoom_info(None, None, None) == _ffi.EINVAL


def test_summarize_arguments_are_checked_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    for n, size in ((1, 0), (1, -4), (-1, 5)):
        assert lib.bxmi_zoom_summarize(None, 0, None, None, None, n, size, None, None, None, None, None) == _ffi.EINVAL
        assert lib.bxmi_zoom_summarize_dev(None, 0, None, None, None, n, size, None, None, None, None, None, None) == _ffi.EINVAL
    assert lib.bxmi_zoom_summarize(None, -1, None, None, None, 1, 5, None, None, None, None, None) == _ffi.EINVAL
    assert b"n_tracks" in lib.bxmi_last_error()
    assert lib.bxmi_zoom_summarize(None, 1, None, None, None, 1, 5, None, None, None, None, None) == _ffi.EINVAL  # NULL track list
    assert lib.bxmi_zoom_summarize(None, 0, None, None, None, 1, 5, None, None, None, None, None) == _ffi.EINVAL  # NULL arrays
    assert lib.bxmi_zoom_summarize(None, 0, None, None, None, 0, 5, None, None, None, None, None) == _ffi.OK  # n == 0: nothing to do
    assert lib.bxmi_zoom_summarize_dev(None, 0, None, None, None, 0, 5, None, None, None, None, None, None) == _ffi.OK
    # the host form looks at its rows: a track beyond the list, a negative coordinate
    rows = [np.array(x, dtype=np.int32) for x in ([0], [0], [10])]
    out = [np.zeros(2) for _ in range(5)]
    assert lib.bxmi_zoom_summarize(None, 0, *[_ffi.ptr(a) for a in rows], 1, 2, *[_ffi.ptr(a) for a in out]) == _ffi.EINVAL
    assert b"track_of[0]" in lib.bxmi_last_error()
    rows[0][0], rows[1][0] = -1, -7
    assert lib.bxmi_zoom_summarize(None, 0, *[_ffi.ptr(a) for a in rows], 1, 2, *[_ffi.ptr(a) for a in out]) == _ffi.EINVAL
    assert b"negative" in lib.bxmi_last_error()


def test_layers_exist_without_a_device():
    import bx.bbi.bigwig_file as drop_in
    from bxmi import bigwig, summary
    from bxmi.cli import bigwig_summary

    for name in ("ZoomTrack", "TrackSet", "summarize_zoom", "summarize_zoom_dev", "pick_level", "pick_levels"):
        assert callable(getattr(summary, name)), name
    assert callable(summary.ZoomTrack.from_bigwig) and callable(summary.TrackSet.from_bigwig) and callable(bigwig.read_zoom_file)
    assert inspect.signature(summary.TrackSet.summarize).parameters["zoom"].default is True
    assert inspect.signature(drop_in.BigWigFile.__init__).parameters["use_zoom"].default is False
    assert "-z" in bigwig_summary.__doc__
    for text in (summary.__doc__, drop_in.__doc__, bigwig_summary.__doc__):
        assert "compatibility" in text and "flip later" in text
    with open(os.path.join(ROOT, "tests", "golden", "zoom", "unordered.z.bw"), "rb") as f:
        bw = drop_in.BigWigFile(f, use_zoom=True)
    try:
        bw.summarize("chrU", 0, 160, 4)  # step 40: the level of reduction 8, whose records descend
    except NotImplementedError as e:
        assert "summarize_from_full" in str(e) and "record starts" in str(e)
    else:
        raise AssertionError("an unordered level was answered")
