"""CPU-only: tests/pwm_model.py -- the numpy statement the kernel-on-host and the GPU tests compare against -- equals what the
reference's ScoringMatrix.score_string answered (tests/golden/pwm, written by tools/record_pwm_golden.py), as uint32 bit patterns;
and the recordings are what the issue asks them to be."""
import os

import numpy as np
import pytest

import pwm_model as P
import twobit_model as M


@pytest.mark.parametrize("name", M.FILES)
def test_model_equals_the_recorded_scores(name):
    entries = P.recorded(name)
    assert entries
    for case, text, mat, want in entries:
        got = P.matrix(mat).score(np.frombuffer(text.encode("ascii"), dtype=np.uint8))
        assert want.dtype == np.float32 and len(want) == len(text)
        assert np.array_equal(P.bits(got), P.bits(want)), (name, case, mat)
        # every NaN of the reference is numpy's: the fill, never a result of arithmetic
        assert (P.bits(want)[np.isnan(want)] == P.NAN_BITS).all()
        w = P.matrix(mat).width
        assert np.isnan(want[max(len(text) - w + 1, 0):]).all()


def test_the_recordings_cover_what_they_should():
    _, _, width_max, _, _ = P.kernel_constants()
    mats = {k: P.matrix(k) for k in P.matrix_names()}
    assert {m.width for m in mats.values()} >= {1, 4, 20, width_max}
    assert {"".join(m.alphabet) for m in mats.values()} == {"ACGT", "ACGTN", "ACGTacgt"}
    assert np.isneginf(mats["ninf"].values).any() and not np.isnan(np.concatenate([m.values.ravel() for m in mats.values()])).any()
    d = np.abs(mats["denorm"].values)
    assert ((d > 0) & (d < np.finfo(np.float32).tiny)).all() and not mats["zeros"].values.any()
    used, masks, numbers = set(), set(), {}
    for name in M.FILES:
        for case, _, mat, want in P.recorded(name):
            used.add(mat)
            masks.add(case["mask"])
            numbers[mat] = numbers.get(mat, 0) + int((~np.isnan(want)).sum())
    assert used == set(mats) and masks == {True, False} and all(numbers[k] > 0 for k in mats), numbers
    # -inf scores and denormal scores were recorded, and a lower-case alphabet scored masked letters
    every = [(mat, want) for name in M.FILES for _, _, mat, want in P.recorded(name)]
    assert any(np.isneginf(w).any() for m, w in every if m == "ninf")
    assert any(((np.abs(w) < np.finfo(np.float32).tiny) & (w != 0)).any() for m, w in every if m == "denorm")
    # no new file is larger than the largest of tests/golden/twobit; nothing but data
    limit = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN))
    for f in os.listdir(P.GOLDEN):
        assert f.endswith((".npy", ".json")) and os.path.getsize(os.path.join(P.GOLDEN, f)) <= limit, f


def test_matrix_layout_and_reverse_complement():
    rows = np.arange(12, dtype=np.float32).reshape(3, 4)
    m = P.Matrix("TGCA", rows)
    assert m.sorted_alphabet == list("ACGT") and m.values.tolist() == rows[:, ::-1].tolist()
    assert m.char_to_index[ord("A")] == 0 and m.char_to_index[ord("T")] == 3 and m.char_to_index[ord("a")] == -1 and m.char_to_index.dtype == np.int16
    rc = m.reverse_complement()
    assert rc.values.tolist() == m.values[::-1, ::-1].tolist() and rc.sorted_alphabet == m.sorted_alphabet
    # the package's own class lays a matrix out as the model does, every recorded matrix included, and reads the file format
    from bxmi import motif

    for name in P.matrix_names():
        model = P.matrix(name)
        mine = motif.ScoringMatrix(model.alphabet, model.rows)
        assert P.bits(mine.values).tolist() == P.bits(model.values).tolist() and np.array_equal(mine.char_to_index, model.char_to_index), name
        back = mine.reverse_complement()
        assert P.bits(back.values).tolist() == P.bits(model.reverse_complement().values).tolist(), name
        assert P.bits(motif.ScoringMatrix(back.alphabet, back.values).values).tolist() == P.bits(back.values).tolist()  # `alphabet` describes the rows
    text = ["  # a comment, indented\n", "TGCA\n", "\n"] + [" ".join(repr(float(x)) for x in row) + "\n" for row in rows]
    assert motif.read_matrix(text).values.tolist() == m.values.tolist()
    # the chain is ordered: a sum that float32 rounds differently when reassociated
    chain = P.Matrix("A", [[1e8], [1.0], [-1e8], [1.0]])
    assert chain.score(np.frombuffer(b"AAAA", dtype=np.uint8))[0] == np.float32(1.0)
    assert P.best_of(np.array([np.nan, 2, 5, 5, np.nan], dtype=np.float32)) == (5.0, 2)
    top, at = P.best_of(np.array([np.nan], dtype=np.float32))
    assert np.isnan(top) and at == -1
