"""CPU-only: the pwm entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; the device variants have
the host forms' arguments followed by the stream; every refusal of bxmi_pwm_create and every argument error of the scoring calls is
answered before any device call, with its message; the Python layer and the command line import without a device; the constants
the tests read out of pwm.hpp are where they look for them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pwm_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bxmi_pwm_create", "bxmi_pwm_destroy", "bxmi_pwm_info", "bxmi_twobit_pwm_scores", "bxmi_twobit_pwm_scores_dev", "bxmi_twobit_pwm_best",
         "bxmi_twobit_pwm_best_dev")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    top = header.split("#ifndef BXMI_H")[0]
    assert "lib/bx/motif/_pwm.pyx:23-55" in top and "pwm.py:141-149" in top and "bxmi_twobit_pwm_*" in top
    for name in NAMES:
        assert name in _ffi.EXPORTED and hasattr(lib, name), name
        decl = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(re.findall(r",", decl)) + 1 == len(_ffi._SIGNATURES[name]), name
    for host_name in ("bxmi_twobit_pwm_scores", "bxmi_twobit_pwm_best"):
        host, dev = _ffi._SIGNATURES[host_name], _ffi._SIGNATURES[host_name + "_dev"]
        assert dev[:-1] == host and dev[-1] is C.c_void_p
        decl = lambda n: re.sub(r"\s+", " ", re.search(r"int %s\(([^;]*)\);" % n, header).group(1)).strip()  # noqa: E731
        assert decl(host_name + "_dev") == decl(host_name) + ", void *stream"
    flat = re.sub(r"[\s*]+", " ", header)
    # the rows are those of bxmi_twobit_bases; the NaN, the unspecified NaN and the one-call-at-a-time rule are documented
    assert "int do_mask, const bxmi_pwm_t *pwm, float *out" in re.sub(r"\s+", " ", header)
    assert "0x7FC00000" in header and "unspecified sign and payload" in flat and "one 2bit call (bases, composition, pwm) at a time" in flat
    assert "T C A G N t c a g n" in header and "-inf entries are legitimate and exact" in flat


def test_unit_is_built_from_the_kernel_header():
    unit = open(os.path.join(ROOT, "bx-python_amd", "csrc", "sequence.hip")).read()
    assert unit.index('#include "twobit.hpp"') < unit.index('#include "pwm.hpp"')
    for word in ("pw_scores_kernel<true>", "pw_scores_kernel<false>", "pw_unpack_kernel", "PW_SLAB"):
        assert word in unit, word
    text = open(os.path.join(ROOT, "bx-python_amd", "csrc", "pwm.hpp")).read()
    for word in ("TbTrack", "tb_word", "tb_covered", "sm_first_above", "sa_row_of", "store_int4", "#ifndef PW_WAVE_MAX64", "#ifndef PW_ATOMIC_MAX64"):
        assert word in text, word
    # the floats of the 2bit unit live in pwm.hpp: twobit.hpp is still integers only, and the build is still plain -O3
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", open(os.path.join(ROOT, "bx-python_amd", "csrc", "twobit.hpp")).read()))
    build = open(os.path.join(ROOT, "bx-python_amd", "csrc", "build.sh")).read()
    assert "-O3" in build and "fast-math" not in build and "-ffp-contract" not in build and "denormal" not in build and "pwm" not in build


def test_constants_are_where_the_tests_read_them():
    text = open(os.path.join(ROOT, "bx-python_amd", "csrc", "pwm.hpp")).read()
    threads, tile, width_max, cols_max, mats_max = P.kernel_constants()
    assert (P.THREADS, P.TILE, P.WIDTH_MAX, P.COLS_MAX, P.MATS_MAX) == (threads, tile, width_max, cols_max, mats_max)
    assert (threads, width_max, cols_max) == (256, 256, 16) and mats_max >= 2
    assert width_max * cols_max * 4 == 16 * 1024  # the largest matrix is 16 KiB of LDS
    assert re.search(r"constexpr unsigned PW_NAN = 0x7FC00000u;", text) and P.NAN_BITS == 0x7FC00000 and np.isnan(P.NAN)
    assert P.bits(np.float32(np.nan))[0] == P.NAN_BITS  # numpy's nan
    unit = open(os.path.join(ROOT, "bx-python_amd", "csrc", "sequence.hip")).read()
    assert re.search(r"constexpr int64_t PW_SLAB = \(int64_t\)PW_TILE << 12;", unit) and P.PW_SLAB == tile << 12
    from bxmi import motif

    assert motif.LETTERS == P.LETTERS == "TCAGNtcagn"


def test_create_refuses_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    p = _ffi.ptr
    values = np.zeros((600, 16), dtype=np.float32)
    acgt = np.array([3, 1, 0, 2, -1, -1, -1, -1, -1, -1], dtype=np.int8)

    def create(mat_off, n_cols=4, letters=acgt, n_mats=None, vals=values):
        off = np.array(mat_off, dtype=np.int32)
        h = C.c_void_p(12345)
        rc = lib.bxmi_pwm_create(p(vals), p(off), len(off) - 1 if n_mats is None else n_mats, n_cols, p(letters), C.byref(h))
        assert h.value is None  # *out is cleared whatever happens
        return rc

    def refused(rc, word):
        assert rc == _ffi.EINVAL and word in lib.bxmi_last_error(), (rc, word, lib.bxmi_last_error())

    refused(create([0], n_mats=0), b"n_mats = 0 outside [1, %d]" % P.MATS_MAX)
    refused(create(list(range(P.MATS_MAX + 2))), b"n_mats = %d outside" % (P.MATS_MAX + 1))
    refused(create([0, 4], n_cols=0), b"n_cols = 0 outside [1, 16]")
    refused(create([0, 4], n_cols=17), b"n_cols = 17 outside [1, 16]")
    refused(create([0, 0]), b"matrix 0 has width 0 outside [1, 256]")
    refused(create([0, 4, 4 + P.WIDTH_MAX + 1]), b"matrix 1 has width 257 outside [1, 256]")
    refused(create([1, 4]), b"mat_off[0] = 1, must be 0")
    refused(create([0, 9, 4]), b"mat_off descends at matrix 1")
    refused(create([0, 4], letters=np.array([4, 1, 0, 2, -1, -1, -1, -1, -1, -1], dtype=np.int8)), b"letter_col[0] = 4 outside [-1, n_cols = 4)")
    refused(create([0, 4], letters=np.array([3, 1, 0, 2, -1, -1, -1, -1, -1, -2], dtype=np.int8)), b"letter_col[9] = -2 outside")
    refused(create([0, 4], vals=None), b"NULL array")
    refused(create([0, 4], letters=None), b"NULL array")
    h = C.c_void_p(12345)
    refused(lib.bxmi_pwm_create(p(values), None, 1, 4, p(acgt), C.byref(h)), b"NULL array")
    refused(lib.bxmi_pwm_create(p(values), p(np.array([0, 4], dtype=np.int32)), 1, 4, p(acgt), None), b"out is NULL")
    refused(lib.bxmi_pwm_info(None, None, None, None), b"NULL handle")
    assert lib.bxmi_pwm_destroy(None) == _ffi.OK


def test_arguments_are_checked_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    track_of, start = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    out = np.full(64, 7, dtype=np.float32)
    pos = np.full(64, 7, dtype=np.int32)
    p = _ffi.ptr

    def offsets(*values):
        return np.array(values, dtype=np.int64)

    def refused(rc, word):
        assert rc == _ffi.EINVAL and word in lib.bxmi_last_error(), (rc, word, lib.bxmi_last_error())

    # no handle can be made without a device: every check of the rows comes before the handle is looked at, and a NULL one is refused
    forms = {
        "scores": lambda n, width, off, total, pwm=None: lib.bxmi_twobit_pwm_scores(None, 0, p(track_of), p(start), n, width, p(off), total, 1, pwm, p(out)),
        "scores_dev": lambda n, width, off, total, pwm=None: lib.bxmi_twobit_pwm_scores_dev(None, 0, p(track_of), p(start), n, width, p(off), total, 1, pwm,
                                                                                           p(out), None),
        "best": lambda n, width, off, total, pwm=None: lib.bxmi_twobit_pwm_best(None, 0, p(track_of), p(start), n, width, p(off), total, 1, pwm, p(out), p(pos)),
        "best_dev": lambda n, width, off, total, pwm=None: lib.bxmi_twobit_pwm_best_dev(None, 0, p(track_of), p(start), n, width, p(off), total, 1, pwm, p(out),
                                                                                       p(pos), None),
    }
    for name, form in forms.items():
        refused(form(3, 0, None, 0), b"width")                      # width < 1 with NULL offsets
        refused(form(3, -2, None, -6), b"width")
        refused(form(3, 4, offsets(0, 1, 2, 3), 3), b"width")       # width != 0 with offsets
        refused(form(3, 4, None, 11), b"total")                     # total != n * width
        refused(form(-1, 4, None, -4), b"n =")                      # negative n
        refused(form(3, 0, offsets(0, 1, 2, 3), -1), b"total")
        refused(form(3, 4, None, 12), b"NULL matrix set")
        refused(form(0, 4, None, 0), b"NULL matrix set")
        assert name.encode() in lib.bxmi_last_error()
    refused(lib.bxmi_twobit_pwm_scores(None, -1, p(track_of), p(start), 3, 4, None, 12, 1, None, p(out)), b"n_tracks")
    handles = (C.c_void_p * 1)(None)
    refused(lib.bxmi_twobit_pwm_best(handles, 1, p(track_of), p(start), 3, 4, None, 12, 1, None, p(out), p(pos)), b"NULL handle")
    refused(lib.bxmi_twobit_pwm_scores(None, 1, p(track_of), p(start), 3, 4, None, 12, 1, None, p(out)), b"NULL track list")
    assert (out == 7).all() and (pos == 7).all()


def test_layers_import_without_a_device(tmp_path):
    from bxmi import motif, sequence
    from bxmi.cli import twobit_pwm_scores as cli

    for name in ("scores", "score_matrix", "best", "scores_dev", "score_matrix_dev", "best_dev"):
        assert callable(getattr(motif, name)) and callable(getattr(sequence.TwoBitSet, name)), name
    assert callable(motif.MatrixSet.close) and motif.MatrixSet._destroy == "bxmi_pwm_destroy"
    m = motif.ScoringMatrix("ACGT", [[1, 2, 3, 4], [5, 6, 7, 8]])
    assert m.width == 2 and m.values.dtype == np.float32 and m.char_to_index.dtype == np.int16 and m.char_to_index.shape == (256,)
    assert m.reverse_complement().values.tolist() == [[8, 7, 6, 5], [4, 3, 2, 1]]
    mixed = motif.ScoringMatrix("TA", [[1, 2]])
    assert mixed.sorted_alphabet == ["A", "T"] and mixed.values.tolist() == [[2, 1]] and mixed.char_to_index[ord("T")] == 1
    path = tmp_path / "m.txt"
    path.write_text("ACGT\n1 2 3 4\n-inf 0 1e-40 2\n")
    with open(path) as f:
        read = motif.read_matrix(f)
    assert read.width == 2 and np.isneginf(read.values[1, 0]) and read.values[1, 2] == np.float32(1e-40)
    with pytest.raises(ValueError):
        motif.MatrixSet([])
    for argv in ([], ["a.2bit"], ["a.2bit", "m.txt", "x"], ["a.2bit", "m.txt", "-x"], ["-b", "-u"]):
        with pytest.raises(SystemExit) as e:  # the usage text, before any file is opened
            cli.main(argv)
        assert "usage: twobit_pwm_scores seq.2bit matrix.txt [-r] [-b] [-u]" in str(e.value), argv
