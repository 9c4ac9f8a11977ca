"""CPU-only: the rule tests/build_model.py states -- maximal runs of N / n and of lower case, code 0 under N, zero bits behind the
last base -- is the rule of real files: for every record of the reference's test.fa, testN.fa and testMask.fa the model gives the
arrays bxmi.twobit.read_file reads from the .2bit file beside it (sizes, the four block arrays, the packed bytes)."""
import os

import numpy as np
import pytest

import build_model as B
import twobit_model as M
from bxmi import fasta, nib, twobit


@pytest.mark.parametrize("stem", ("test", "testN", "testMask"))
def test_model_of_fasta_equals_the_2bit_file(stem):
    records = fasta.read_file(os.path.join(M.GOLDEN, stem + ".fa"))
    want = twobit.read_file(os.path.join(M.GOLDEN, stem + ".2bit"))
    assert list(records) == list(want) and len(records) >= 1
    for name, letters in records.items():
        built = B.from_letters(letters)
        assert built.first_other is None, (stem, name)
        assert B.same_arrays(built.seq, want[name]), (stem, name)
        assert len(built.seq.packed) == len(want[name].packed)
        # and back: the letters of the file's arrays are the record's
        assert np.array_equal(M.letters(want[name]), letters), (stem, name)


def test_eight_records_in_all():
    assert sum(len(fasta.read_file(os.path.join(M.GOLDEN, s + ".fa"))) for s in ("test", "testN", "testMask")) == 8


def test_nib_model_round_trip():
    """the nibbles of a record give the arrays of its letters; codes 5-7 are other, with and without the mask bit"""
    letters = fasta.read_file(os.path.join(M.GOLDEN, "test.fa"))
    for text in letters.values():
        for cut in (len(text), len(text) - 1):
            built = B.from_nib(B.to_nib(text[:cut]), cut)
            assert built.first_other is None and B.same_arrays(built.seq, B.from_letters(text[:cut]).seq)
    built = B.from_nib(np.array([0x01, 0x5D, 0x24], dtype=np.uint8), 6)  # T C X x A N
    assert (built.first_other, built.other_value) == (2, 5)
    assert built.seq.n_starts.tolist() == [2, 5] and built.seq.n_sizes.tolist() == [2, 1]
    assert built.seq.m_starts.tolist() == [3] and built.seq.m_sizes.tolist() == [1]


def test_fasta_reader_follows_fastafile():
    got = fasta.read_file(data=b"AC GT\nnn\n>one two\nAC\tG\r\n\nT\n> three\n")
    assert list(got) == ["", "one", "three"]
    assert got[""].tobytes() == b"ACGTnn" and got["one"].tobytes() == b"ACGT" and len(got["three"]) == 0
    with pytest.raises(ValueError):
        fasta.read_file(data=b">a\nAC\n>a\nGT\n")
    with pytest.raises(ValueError):
        fasta.read_file(data=b">\nAC\n>\nGT\n")
    assert fasta.read_file(data=b"") == {}
    import gzip

    assert fasta.read_file(data=gzip.compress(b">z\nACGT"))["z"].tobytes() == b"ACGT"


def test_nib_reader():
    size, nibbles, order = nib.read_file(data=b"\x3a\x3d\xe9\x6b\x03\x00\x00\x00\x01\x20")
    assert (size, nibbles.tolist(), order) == (3, [0x01, 0x20], "<")
    size, nibbles, order = nib.read_file(data=b"\x6b\xe9\x3d\x3a\x00\x00\x00\x02\x4c")
    assert (size, nibbles.tolist(), order) == (2, [0x4C], ">")
    with pytest.raises(Exception, match="Not a NIB file"):
        nib.read_file(data=b"\x00\x00\x00\x00\x00\x00\x00\x00")
    with pytest.raises(ValueError):
        nib.read_file(data=b"\x6b\xe9\x3d\x3a\x00\x00\x00\x05\x4c")
