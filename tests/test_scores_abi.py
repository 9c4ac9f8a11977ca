"""CPU-only: the score-track entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; the device
variant's signature ends in the stream; the knob is listed; the Python layers and the command line import without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bxmi_scores_create", "bxmi_scores_destroy", "bxmi_scores_info", "bxmi_scores_values_dev", "bxmi_scores_write", "bxmi_scores_read",
         "bxmi_scores_set_spans", "bxmi_scores_aggregate", "bxmi_scores_aggregate_dev")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    assert "typedef struct bxmi_scores bxmi_scores_t;" in header
    assert "scripts/aggregate_scores_in_intervals.py" in header.split("#ifndef BXMI_H")[0]  # the reference mapping of the top comment
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _ffi.EXPORTED, name
        assert hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(re.findall(r",", decl)) + 1 == len(_ffi._SIGNATURES[name]), name
    host, dev = _ffi._SIGNATURES["bxmi_scores_aggregate"], _ffi._SIGNATURES["bxmi_scores_aggregate_dev"]
    assert dev[:-1] == host and dev[-1] is C.c_void_p  # the same arguments, then the stream
    decl = re.search(r"int bxmi_scores_aggregate_dev\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl).strip().endswith("void *stream")


def test_the_knob_is_an_option():
    from bxmi import _ffi

    opts = _ffi.options()
    assert opts.get("scores.wave_min_len", 0) > 0
    before = opts["scores.wave_min_len"]
    try:
        _ffi.call("bxmi_set_option", b"scores.wave_min_len", 128)
        v = C.c_int64(0)
        _ffi.call("bxmi_get_option", b"scores.wave_min_len", C.byref(v))
        assert v.value == 128 and _ffi.options()["scores.wave_min_len"] == 128
    finally:
        _ffi.call("bxmi_set_option", b"scores.wave_min_len", before)


def test_python_layers_import():
    from bxmi import scores, wiggle
    from bxmi.cli import aggregate_scores_in_intervals as cli

    for m in ("write", "read", "set_spans", "aggregate", "aggregate_dev", "aggregate_ptrs", "close"):
        assert callable(getattr(scores.ScoreTrack, m, None)), m
    assert callable(scores.format_row) and callable(wiggle.read_spans) and callable(wiggle.read_spans_file) and callable(cli.main)
    assert scores.format_row("c", 1, 2, 0, 0.0, 0.0, 0.0) == "c\t1\t2\tnan\tnan\tnan"


def test_binned_directories_are_refused_by_name(capsys):
    import pytest

    from bxmi.cli import aggregate_scores_in_intervals as cli

    with pytest.raises(SystemExit) as e:
        cli.main(["-b", "scores_dir", "intervals.bed"])
    assert e.value.code != 0
    assert "not supported" in capsys.readouterr().err
