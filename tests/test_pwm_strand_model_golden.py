"""CPU-only: tests/pwm_strand_model.py -- pwm_model.Matrix.score on strand_model.reverse_complement(row), what the kernel-on-host and
the GPU tests of the stranded pwm calls compare against -- equals what the reference answered for
matrix.score_string(seq.get(s, e).translate(DNA_COMP)[::-1]) (tests/golden/pwm_strand, written by
tools/record_pwm_strand_golden.py), as uint32 bit patterns; and the recordings are what they should be."""
import os

import numpy as np
import pytest

import pwm_model as P
import pwm_strand_model as PS
import twobit_model as M

OPEN_ALPHABETS = ("w20n", "w4n", "w1lc", "w20lc")  # not closed under complement: N has no partner, or T/A differ in case from nothing


@pytest.mark.parametrize("name", M.FILES)
def test_model_equals_the_recorded_scores(name):
    entries = PS.recorded(name)
    kept, of = PS.manifest()["files"][name]["kept"]
    assert len(entries) == kept == len(PS.manifest()["files"][name]["entries"]) and kept > 0
    assert of == len(P.manifest()["files"][name]["entries"]) and kept == of  # the whole cross product fitted: every plus entry has its minus
    for case, text, mat, want in entries:
        row = np.frombuffer(text.encode("ascii"), dtype=np.uint8)
        got = PS.score(P.matrix(mat), row, True)
        assert want.dtype == np.float32 and len(want) == len(text)
        assert np.array_equal(P.bits(got), P.bits(want)), (name, case, mat)
        assert (P.bits(want)[np.isnan(want)] == P.NAN_BITS).all()
        w = P.matrix(mat).width
        assert np.isnan(want[max(len(text) - w + 1, 0):]).all()  # the last W - 1 of the STRAND's string: the first genomic positions


def test_the_recordings_cover_what_they_should():
    used, masks, numbers, differ = set(), set(), {}, 0
    plus = {name: {(e["case"], e["matrix"]): k for k, e in enumerate(P.manifest()["files"][name]["entries"])} for name in M.FILES}
    for name in M.FILES:
        there = P.recorded(name)
        for e, (case, text, mat, want) in zip(PS.manifest()["files"][name]["entries"], PS.recorded(name)):
            used.add(mat)
            masks.add(case["mask"])
            numbers[mat] = numbers.get(mat, 0) + int((~np.isnan(want)).sum())
            differ += not np.array_equal(P.bits(want), P.bits(there[plus[name][(e["case"], e["matrix"])]][3]))
    assert used == set(P.matrix_names()) and set(OPEN_ALPHABETS) <= used and masks == {True, False}
    assert all(numbers[k] > 0 for k in used), numbers
    assert differ > 100  # (the minus answers are not the plus answers)
    limit = max(os.path.getsize(os.path.join(P.GOLDEN, f)) for f in os.listdir(P.GOLDEN))
    for f in os.listdir(PS.GOLDEN):
        assert f.endswith((".npy", ".json")) and os.path.getsize(os.path.join(PS.GOLDEN, f)) <= limit, f


def test_site_starts():
    # ACGTT under a matrix of 2 rows: offset 0 of the minus string AACGT is the window over genomic positions 3, 4 of a row from 10
    assert PS.site_starts([10], [5], [0], 2, [True]).tolist() == [13] and PS.site_starts([10], [5], [3], 2, [True]).tolist() == [10]
    assert PS.site_starts([10, 10], [5, 5], [1, -1], 2, [False, True]).tolist() == [11, -1]
