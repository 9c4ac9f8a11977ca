"""CPU-only: the six stranded pwm entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; each is its
unstranded sibling with `const int8_t *strand_or_null` after `start`, the device variant the host form followed by the stream; every
refusal -- the siblings' and the strand entry that is neither 0 nor 1, which names its row -- is answered before any device call
with the outputs untouched; the Python layers take `strands`; `motif.site_starts` is exact; both command lines know -s."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import pwm_strand_model as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = ("bxmi_twobit_pwm_scores", "bxmi_twobit_pwm_best", "bxmi_twobit_pwm_hits")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    decl = lambda n: re.sub(r"\s+", " ", re.search(r"int %s\(([^;]*)\);" % n, header).group(1)).strip()  # noqa: E731
    for sibling in SIBLINGS:
        for tail in ("", "_dev"):
            name, plain = sibling + "_strand" + tail, sibling + tail
            assert name in _ffi.EXPORTED and hasattr(lib, name), name
            assert len(re.findall(r",", decl(name))) + 1 == len(_ffi._SIGNATURES[name]), name
            assert decl(name) == decl(plain).replace("const int32_t *start,", "const int32_t *start, const int8_t *strand_or_null,", 1), name
            at = decl(plain).split(",").index(" const int32_t *start") + 1
            sig = list(_ffi._SIGNATURES[plain])
            assert _ffi._SIGNATURES[name] == sig[:at] + [C.c_void_p] + sig[at:], name
        host, dev = _ffi._SIGNATURES[sibling + "_strand"], _ffi._SIGNATURES[sibling + "_strand_dev"]
        assert dev[:-1] == host and dev[-1] is C.c_void_p
        assert decl(sibling + "_strand_dev") == decl(sibling + "_strand") + ", void *stream"
    flat = re.sub(r"[\s*]+", " ", header)
    assert "not there yet" not in flat
    for words in ("AS WRITTEN, ON THAT STRING", "letter_col is applied to the COMPLEMENTED letter", "need not be closed under complement",
                  "FIRST W - 1 genomic positions", "start + len - W - pos", "FIRST offset in the strand's string", "offset in the strand's string)",
                  "descending matrix row", "ANY NON-ZERO ENTRY IS MINUS", "NULL means all plus", "naming the row"):
        assert words in flat, words


def test_unit_launches_the_stranded_kernels():
    csrc = os.path.join(ROOT, "bx-python_amd", "csrc")
    unit = open(os.path.join(csrc, "sequence.hip")).read()
    for word in ("pw_scores_strand_kernel<true>", "pw_scores_strand_kernel<false>", "pw_hits_strand_kernel<FILL>", "pw_scores_kernel<true>",
                 "pw_scores_kernel<false>", "pw_hits_kernel<FILL>", "stage_strand(S, strand, rows.r0, rows.m", "stage_strand(S, strand, 0, n"):
        assert word in unit, word
    assert unit.count("strand_check(who, strand, n)") >= 6  # letters, counts, k-mers and the three pwm host forms
    scores = open(os.path.join(csrc, "pwm.hpp")).read()
    hits = open(os.path.join(csrc, "pwm_hits.hpp")).read()
    for word in ("template <bool STRAND>", "pw_stage_columns", "tb_minus<STRAND>", "tb_complement(", "pw_scores_body<false, BEST>", "pw_scores_body<true, BEST>"):
        assert word in scores, word
    for word in ("pw_stage_columns<STRAND>", "tb_minus<STRAND>", "pw_hits_body<false, FILL>", "pw_hits_body<true, FILL>"):
        assert word in hits, word
    # the staging stands once: the hits kernel has no loads or searches of its own any more
    code = re.sub(r"//.*", "", hits)
    assert "tb_word" not in code and "sm_first_above" not in code and "tb_covered" not in code


def test_arguments_are_checked_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    p = _ffi.ptr
    track_of, start = np.full(3, -1, dtype=np.int32), np.zeros(3, dtype=np.int32)
    plus, bad, worse = np.zeros(3, dtype=np.int8), np.array([0, 1, 2], dtype=np.int8), np.array([-1, 0, 3], dtype=np.int8)
    out = np.full(64, 9, dtype=np.float32)
    top, at = np.full(8, 9, dtype=np.float32), np.full(8, 9, dtype=np.int32)
    mat_hits = np.full(3, 9, dtype=np.int64)
    rows, pos, score = np.full(8, 9, dtype=np.int32), np.full(8, 9, dtype=np.int32), np.full(8, 9, dtype=np.float32)
    least = np.zeros(2, dtype=np.float32)
    pwm = C.c_void_p(0)  # (no matrix set can be made without a device: the calls below are refused before they look at one)

    def offsets(*values):
        return np.array(values, dtype=np.int64)

    def refused(rc, word):
        assert rc == _ffi.EINVAL and word in lib.bxmi_last_error(), (rc, word, lib.bxmi_last_error())

    def scores(strand=plus, n=3, width=4, off=None, total=12, n_tracks=0, tracks=None, t=track_of, o=out, dev=False):
        tail = (None,) if dev else ()
        fn = lib.bxmi_twobit_pwm_scores_strand_dev if dev else lib.bxmi_twobit_pwm_scores_strand
        return fn(tracks, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, pwm, p(o), *tail)

    def best(strand=plus, n=3, width=4, off=None, total=12, n_tracks=0, tracks=None, t=track_of, dev=False):
        tail = (None,) if dev else ()
        fn = lib.bxmi_twobit_pwm_best_strand_dev if dev else lib.bxmi_twobit_pwm_best_strand
        return fn(tracks, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, pwm, p(top), p(at), *tail)

    def hits(strand=plus, n=3, width=4, off=None, total=12, n_tracks=0, tracks=None, t=track_of, cap=8, thr=least, mh=mat_hits, dev=False):
        tail = (None,) if dev else ()
        fn = lib.bxmi_twobit_pwm_hits_strand_dev if dev else lib.bxmi_twobit_pwm_hits_strand
        return fn(tracks, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, pwm, p(thr), cap, p(mh), p(rows), p(pos), p(score), *tail)

    # the siblings' refusals fire with a strand array and without, in the host and the device forms, and name the entry point
    for strand in (plus, bad, None):
        for form in (scores, best, hits):
            for dev in (False, True):
                refused(form(strand, width=0, total=0, dev=dev), b"width")
                refused(form(strand, total=11, dev=dev), b"total")
                refused(form(strand, n=-1, total=-4, dev=dev), b"n =")
                refused(form(strand, n_tracks=-1, dev=dev), b"n_tracks")
                refused(form(strand, n_tracks=1, dev=dev), b"NULL track list")
                refused(form(strand, dev=dev), b"NULL matrix set")
        refused(hits(strand, thr=None), b"NULL threshold")
        refused(hits(strand, mh=None), b"NULL mat_hits")
        refused(hits(strand, cap=-1), b"cap")
    refused(scores(plus, total=11), b"bxmi_twobit_pwm_scores_strand:")
    refused(best(plus, total=11, dev=True), b"bxmi_twobit_pwm_best_strand_dev:")
    refused(hits(plus, total=11, dev=True), b"bxmi_twobit_pwm_hits_strand_dev:")
    assert (out == 9).all() and (top == 9).all() and (at == 9).all() and (mat_hits == 9).all() and (rows == 9).all() and (pos == 9).all() and (score == 9).all()


def test_a_bad_strand_entry_is_refused_by_the_host_forms_with_the_outputs_untouched():
    """needs a matrix set, so a device; without one the refusal of the NULL set comes first (above) -- here the order of the checks
    is read from the unit: strand_check stands before the lock, the table and every launch in each host form"""
    unit = open(os.path.join(ROOT, "bx-python_amd", "csrc", "sequence.hip")).read()
    for form in ("pwm_scores_host", "pwm_best_host", "pwm_hits_host"):
        body = unit[unit.index("static int %s(" % form):]
        body = body[:body.index("\n}\n")]
        check = body.index("strand_check(who, strand, n)")
        assert check < body.index("std::lock_guard") and check < body.index("sequence_fill_table") and check < body.index("g_sequence.enter")
        if form == "pwm_hits_host":
            assert check < body.index("mat_hits[m] = 0")  # the counts are not zeroed either
    for form in ("pwm_scores_dev", "pwm_best_dev", "pwm_hits_dev"):
        body = unit[unit.index("static int %s(" % form):]
        assert "strand_check" not in body[:body.index("\n}\n")]  # the device forms cannot read it: any non-zero entry is minus


def test_python_layers_take_strands():
    from bxmi import motif, sequence

    for name in ("scores", "score_matrix", "best", "hits", "scores_dev", "score_matrix_dev", "best_dev", "hits_dev"):
        for fn in (getattr(motif, name), getattr(sequence.TwoBitSet, name)):
            params = inspect.signature(fn).parameters
            assert params["strands"].default is None and list(params)[-1] == "strands", name  # last: every positional call means what it meant
    assert motif._strands is sequence._strands and motif._strands_dev is sequence._strands_dev
    name, *args = motif._stranded("bxmi_twobit_pwm_hits_dev", np.zeros(2, dtype=np.int8), tuple("abcdefg"))
    assert name == "bxmi_twobit_pwm_hits_strand_dev" and args[:4] == list("abcd") and args[5:] == list("efg")
    assert motif._stranded("bxmi_twobit_pwm_best", None, ("a", "b")) == ("bxmi_twobit_pwm_best", "a", "b")
    with pytest.raises(ValueError):
        motif.site_starts([1, 2], [5, 5], [0, 0], 2, ["+", "x"])


def test_site_starts():
    from bxmi import motif

    starts, lengths = np.array([10, 10, 100]), np.array([5, 5, 30])
    got = motif.site_starts(starts, lengths, [0, 3, 7], 2, ["-", "+", "-"])
    assert got.dtype == np.int64 and got.tolist() == [13, 13, 121]
    assert motif.site_starts(starts, lengths, [0, 3, 7], 2).tolist() == [10, 13, 107]  # no strands: all plus
    assert motif.site_starts(starts, lengths, [-1, -1, 0], 4, [1, 0, 1]).tolist() == [-1, -1, 126]
    pos = np.array([[0, 1, 2], [3, -1, 28]])  # as `best` gives them: [n_mats, n]
    minus = [True, False, True]
    assert np.array_equal(motif.site_starts(starts, lengths, pos, 2, minus), PS.site_starts(starts, lengths, pos, 2, minus))
    # the window of a minus site, reverse-complemented, is the window of the strand's string
    import strand_model as S

    rng = np.random.default_rng(3)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 60)]
    start, length, width = 7, 40, 6
    row = S.reverse_complement(text[start:start + length])
    for at in (0, 5, length - width):
        site = int(motif.site_starts([start], [length], [at], width, ["-"])[0])
        assert np.array_equal(S.reverse_complement(text[site:site + width]), row[at:at + width])


def test_command_lines_know_the_strand_flag():
    from bxmi.cli import twobit_pwm_hits as hits_cli
    from bxmi.cli import twobit_pwm_scores as scores_cli

    for argv in ([], ["a.2bit", "m.txt", "-x"], ["a.2bit", "m.txt", "-s", "-x"], ["a.2bit", "-s"], ["-s", "-b"]):
        with pytest.raises(SystemExit) as e:
            scores_cli.main(argv)
        assert "usage: twobit_pwm_scores seq.2bit matrix.txt [-r] [-b] [-u] [-s] < bed_file.bed" in str(e.value) and "column 6" in str(e.value), argv
    for argv in ([], ["a.2bit", "m.txt", "-s"], ["a.2bit", "m.txt", "x", "-s"], ["a.2bit", "m.txt", "nan", "-s"], ["-s", "m.txt", "3"]):
        with pytest.raises(SystemExit) as e:
            hits_cli.main(argv)
        assert "usage: twobit_pwm_hits seq.2bit matrix.txt THRESHOLD [-r] [-u] [-s] < bed_file.bed" in str(e.value) and "column 6" in str(e.value), argv
    for main, argv in ((scores_cli.main, ["/nonexistent/a.2bit", "/nonexistent/m.txt", "-s"]), (scores_cli.main, ["/nonexistent/a.2bit", "/nonexistent/m.txt", "-b", "-s", "-r"]),
                       (hits_cli.main, ["/nonexistent/a.2bit", "/nonexistent/m.txt", "-3.5", "-s"]), (hits_cli.main, ["/nonexistent/a.2bit", "/nonexistent/m.txt", "1", "-r", "-s", "-u"])):
        with pytest.raises(Exception) as e:  # -s is accepted: the next thing either tool does is open the matrix file
            main(argv)
        assert not isinstance(e.value, SystemExit), argv


def test_layers_import_without_a_device():
    import bx.seq.twobit as drop_in
    from bxmi import motif  # noqa: F401

    assert callable(motif.site_starts)
    assert not hasattr(drop_in.TwoBitFile, "strand")  # the drop-in stays as it is
