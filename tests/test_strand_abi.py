"""CPU-only: the six strand entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; each is its
unstranded sibling with `const int8_t *strand_or_null` after `start`, the device variant the host form followed by the stream; every
refusal -- the siblings' and the strand entry that is neither 0 nor 1, which names its row -- is answered before any device call
with the outputs untouched; the Python layers take `strands`, refuse a bad one with ValueError and import without a device; both
command lines know -s and still refuse -x; the pure helper of the column permutation is exact."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import kmer_model as K
import strand_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = ("bxmi_twobit_bases", "bxmi_twobit_composition", "bxmi_twobit_kmer_counts")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    top = header.split("#ifndef BXMI_H")[0]
    assert "seq.py:108-109" in top and "seq.py:9-14" in top and "bxmi_twobit_*_strand" in top
    decl = lambda n: re.sub(r"\s+", " ", re.search(r"int %s\(([^;]*)\);" % n, header).group(1)).strip()  # noqa: E731
    for sibling in SIBLINGS:
        for tail in ("", "_dev"):
            name, plain = sibling + "_strand" + tail, sibling + tail
            assert name in _ffi.EXPORTED and hasattr(lib, name), name
            assert len(re.findall(r",", decl(name))) + 1 == len(_ffi._SIGNATURES[name]), name
            # the sibling with the strand after `start`, in the header and in the binding
            assert decl(name) == decl(plain).replace("const int32_t *start,", "const int32_t *start, const int8_t *strand_or_null,", 1), name
            at = decl(plain).split(",").index(" const int32_t *start") + 1
            sig = list(_ffi._SIGNATURES[plain])
            assert _ffi._SIGNATURES[name] == sig[:at] + [C.c_void_p] + sig[at:], name
        host, dev = _ffi._SIGNATURES[sibling + "_strand"], _ffi._SIGNATURES[sibling + "_strand_dev"]
        assert dev[:-1] == host and dev[-1] is C.c_void_p
        assert decl(sibling + "_strand_dev") == decl(sibling + "_strand") + ", void *stream"
    flat = re.sub(r"[\s*]+", " ", header)
    for words in ("ANY NON-ZERO ENTRY IS MINUS", "pad is never complemented", "code ^ 2", "A, C, G, T of a minus row are T, G, C, A of the plus row",
                  "NULL means all plus", "shortens a minus row at its start", "naming the row", "text.translate(DNA_COMP)[::-1]"):
        assert words in flat, words


def test_unit_launches_the_stranded_kernels():
    unit = open(os.path.join(ROOT, "bx-python_amd", "csrc", "sequence.hip")).read()
    for word in ("tb_bases_strand_kernel", "tb_composition_strand_kernel", "km_counts_strand_kernel", "tb_bases_kernel", "tb_composition_kernel",
                 "km_counts_kernel", "stage_strand", "strand_check"):
        assert word in unit, word
    layer = open(os.path.join(ROOT, "bx-python_amd", "csrc", "twobit.hpp")).read()
    for word in ("tb_minus", "tb_letters_minus", "tb_complement", "template <bool STRAND>", "tb_bases_body<false>", "tb_bases_body<true>",
                 "tb_composition_body<false>", "seq.py:108-109"):
        assert word in layer, word
    kmer = open(os.path.join(ROOT, "bx-python_amd", "csrc", "kmer.hpp")).read()
    for word in ("km_counts_body<false>", "km_counts_body<true>", "tb_minus<STRAND>", "km_reverse4"):
        assert word in kmer, word


def test_arguments_are_checked_before_any_device_call():
    from bxmi import _ffi

    lib = _ffi.load()
    p = _ffi.ptr
    track_of, start, end = np.full(3, -1, dtype=np.int32), np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32)
    plus, bad, worse = np.zeros(3, dtype=np.int8), np.array([0, 1, 2], dtype=np.int8), np.array([-1, 0, 3], dtype=np.int8)
    out = np.full(64, 9, dtype=np.uint8)
    six = np.full((3, 6), 7, dtype=np.int32)
    counts = np.full(3 * 16, 7, dtype=np.int32)
    acgt = K.digits8(K.table_of(K.MAPPINGS["acgt"][0]))

    def offsets(*values):
        return np.array(values, dtype=np.int64)

    def refused(rc, word):
        assert rc == _ffi.EINVAL and word in lib.bxmi_last_error(), (rc, word, lib.bxmi_last_error())

    def bases(strand=plus, n=3, width=4, off=None, total=12, pad=78, n_tracks=0, tracks=None, t=track_of, o=out):
        return lib.bxmi_twobit_bases_strand(tracks, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, pad, p(o))

    def bases_dev(strand=plus, n=3, width=4, off=None, total=12, pad=78, n_tracks=0, tracks=None, t=track_of, o=out):
        return lib.bxmi_twobit_bases_strand_dev(tracks, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, pad, p(o), None)

    def comp(strand=plus, n=3, n_tracks=0, e=end, o=six):
        return lib.bxmi_twobit_composition_strand(None, n_tracks, p(track_of), p(start), p(strand), p(e), n, 1, p(o))

    def comp_dev(strand=plus, n=3, n_tracks=0, e=end, o=six):
        return lib.bxmi_twobit_composition_strand_dev(None, n_tracks, p(track_of), p(start), p(strand), p(e), n, 1, p(o), None)

    def kmer(strand=plus, n=3, width=4, off=None, total=12, k=2, radix=4, digits=acgt, n_tracks=0, o=counts, t=track_of):
        return lib.bxmi_twobit_kmer_counts_strand(None, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, k, radix, p(digits), p(o))

    def kmer_dev(strand=plus, n=3, width=4, off=None, total=12, k=2, radix=4, digits=acgt, n_tracks=0, o=counts, t=track_of):
        return lib.bxmi_twobit_kmer_counts_strand_dev(None, n_tracks, p(t), p(start), p(strand), n, width, p(off), total, 1, k, radix, p(digits), p(o), None)

    # a strand entry that is neither 0 nor 1: the host forms name the row (rows without a track: nothing else is wrong with the batch)
    for form in (bases, comp, kmer):
        refused(form(strand=bad), b"strand[2] = 2 of row 2")
        refused(form(strand=worse), b"strand[0] = -1 of row 0")
    assert lib.bxmi_last_error().startswith(b"bxmi_twobit_kmer_counts_strand:")
    # the siblings' refusals still fire, with a strand array and without
    for strand in (plus, None):
        for form in (bases, bases_dev, kmer, kmer_dev):
            refused(form(strand, width=0, total=0), b"width")
            refused(form(strand, off=offsets(0, 1, 2, 3), total=3), b"width")
            refused(form(strand, total=11), b"total")
            refused(form(strand, n=-1, total=-4), b"n =")
            refused(form(strand, n_tracks=-1), b"n_tracks")
            refused(form(strand, n_tracks=1), b"NULL track list")
        for form in (bases, bases_dev):
            refused(form(strand, pad=256), b"pad")
            refused(form(strand, o=None), b"NULL")
        for form in (comp, comp_dev):
            refused(form(strand, n=-1), b"n =")
            refused(form(strand, n=2 ** 31), b"n =")
            refused(form(strand, n_tracks=2), b"NULL track list")
            refused(form(strand, e=None), b"NULL")
            refused(form(strand, o=None), b"NULL")
        for form in (kmer, kmer_dev):
            refused(form(strand, k=0), b"k = 0, must be at least 1")
            refused(form(strand, radix=5), b"radix = 5 outside [2, 4]")
            refused(form(strand, k=8), b"bins")
            refused(form(strand, digits=np.array([4, 0, 0, 0, 0, 0, 0, 0], dtype=np.int8)), b"digits[0] = 4")
            refused(form(strand, digits=None), b"NULL digits")
            refused(form(strand, o=None), b"NULL counts")
        # what only the host forms can read
        refused(bases(strand, width=0, off=offsets(0, 5, 4, 9), total=9), b"descends")
        refused(kmer(strand, width=0, off=offsets(0, 2, 4, 9), total=8), b"row_off[n]")
        named = np.zeros(3, dtype=np.int32)
        refused(bases(strand, t=named), b"track_of[0] = 0, but there are 0 tracks")
        refused(kmer(strand, t=named), b"track_of[0] = 0, but there are 0 tracks")
    # the error names the entry point that was called
    refused(bases_dev(plus, total=11), b"bxmi_twobit_bases_strand_dev:")
    refused(comp_dev(plus, n=-1), b"bxmi_twobit_composition_strand_dev:")
    # nothing to do: no launch, no device
    for form in (bases, bases_dev, kmer, kmer_dev):
        assert form(plus, n=0, total=0) == _ffi.OK and form(None, n=0, total=0) == _ffi.OK
    assert comp(plus, n=0) == _ffi.OK and comp_dev(None, n=0) == _ffi.OK
    assert bases(bad, n=0, total=0) == _ffi.OK  # (no row, no entry to refuse)
    assert (out == 9).all() and (six == 7).all() and (counts == 7).all()


def test_python_layers_take_strands_and_refuse_bad_ones():
    from bxmi import kmers, sequence

    for name in ("sequences", "strings", "matrix", "composition", "matrix_dev", "sequences_dev", "composition_dev"):
        for fn in (getattr(sequence, name), getattr(sequence.TwoBitSet, name)):
            assert inspect.signature(fn).parameters["strands"].default is None, name
    for name in ("counts", "count_matrix", "counts_dev", "count_matrix_dev"):
        for fn in (getattr(kmers, name), getattr(sequence.TwoBitSet, "kmer_" + name)):
            assert inspect.signature(fn).parameters["strands"].default is None, name
    # the keyword comes last: every positional call of before means what it meant
    assert list(inspect.signature(sequence.matrix_dev).parameters)[-3:] == ["stream", "out", "strands"]
    assert list(inspect.signature(kmers.counts).parameters)[-2:] == ["drop_last", "strands"]
    parse = sequence._strands
    assert parse(None, 3) is None
    for given in (["+", "-", "+"], [0, 1, 0], [False, True, False], np.array([0, 1, 0]), np.array([False, True, False]), np.array(["+", "-", "+"]),
                  ("+", 1, False)):
        got = parse(given, 3)
        assert got.dtype == np.int8 and got.tolist() == [0, 1, 0], given
    assert parse([], 0).shape == (0,)
    for given in (["+", "-", "."], ["+", "-", "minus"], [0, 1, 2], [0, 1, -1], [0, 1, 0.5], [0, 1, None], ["+", "-"], ["+"] * 4, [b"+", b"-", b"x"]):
        with pytest.raises(ValueError):
            parse(given, 3)


def test_command_lines_know_the_strand_flag():
    from bxmi.cli import twobit_intervals_to_fasta as fasta
    from bxmi.cli import twobit_kmer_counts as kmer_cli

    for argv in ([], ["a.2bit", "-x"], ["a.2bit", "-s", "-x"], ["-s"], ["a.2bit", "b.2bit", "-s"]):
        with pytest.raises(SystemExit) as e:  # the usage text, before the file is opened
            fasta.main(argv)
        assert "usage: twobit_intervals_to_fasta seq.2bit [-c] [-u] [-s] < bed_file.bed" in str(e.value) and "column 6" in str(e.value), argv
    for argv in ([], ["a.2bit", "3", "-x"], ["a.2bit", "3", "-s", "-x"], ["a.2bit", "-s"], ["-s", "-c"]):
        with pytest.raises(SystemExit) as e:
            kmer_cli.main(argv)
        assert "usage: twobit_kmer_counts seq.2bit K [-u] [-i] [-c] [-o out.npy] [-s] < bed_file.bed" in str(e.value) and "column 6" in str(e.value), argv
    # -s is accepted: the next thing either tool does is open the file
    for main, argv in ((fasta.main, ["/nonexistent/a.2bit", "-s"]), (fasta.main, ["/nonexistent/a.2bit", "-c", "-s", "-u"]),
                       (kmer_cli.main, ["/nonexistent/a.2bit", "3", "-s"]), (kmer_cli.main, ["/nonexistent/a.2bit", "3", "-i", "-c", "-s"])):
        with pytest.raises(Exception) as e:
            main(argv)
        assert not isinstance(e.value, SystemExit), argv


def test_the_column_permutation_of_the_minus_strand():
    from bxmi import kmers

    assert kmers.strand_columns(1).tolist() == [3, 2, 1, 0]
    for k in (1, 2, 3, 5):
        rc = kmers.strand_columns(k)
        assert np.array_equal(rc, kmers.reverse_complement_columns(k)) and np.array_equal(rc[rc], np.arange(4 ** k))
        for w in (0, 1, 4 ** k // 3, 4 ** k - 1):
            assert rc[w] == kmers.index_of(S.reverse_complement_str(kmers.word_of(w, k)), "ACGT")
    assert np.array_equal(kmers.strand_columns(3, "ACGT", case_sensitive=False), kmers.strand_columns(3))
    assert kmers.strand_columns(2, "TGCA").tolist() == kmers.strand_columns(2, {"T": 0, "G": 1, "C": 2, "A": 3}).tolist()
    ry = kmers.strand_columns(3, {"A": 0, "G": 0, "C": 1, "T": 1})  # purines and pyrimidines exchange
    assert ry.tolist() == [7, 3, 5, 1, 6, 2, 4, 0]
    # against the model: the minus counts of a text are that gather of its plus counts
    rng = np.random.default_rng(5)
    text = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, 500)]
    for name, (alphabet, case_sensitive) in K.ALPHABETS.items():
        letters, radix = K.MAPPINGS[name]
        table = K.table_of(letters)
        plus, minus = K.count_text(text, 3, radix, table), K.count_text(S.reverse_complement(text), 3, radix, table)
        assert minus.sum() > 0 and np.array_equal(minus, plus[kmers.strand_columns(3, alphabet, case_sensitive)]), name
    for alphabet in ({"A": 0, "C": 1, "T": 2}, {"A": 0, "a": 0, "C": 1, "t": 1, "G": 2, "T": 3}, {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0}):
        with pytest.raises(ValueError):
            kmers.strand_columns(2, alphabet)


def test_layers_import_without_a_device():
    import bx.seq.twobit as drop_in
    from bxmi import kmers, sequence  # noqa: F401
    from bxmi.cli import twobit_intervals_to_fasta, twobit_kmer_counts  # noqa: F401

    assert callable(sequence._strands) and callable(sequence._strands_dev) and callable(kmers.strand_columns)
    assert not hasattr(drop_in.TwoBitFile, "strand")  # the drop-in stays as it is: the reference's TwoBitFile has no strand
