"""CPU-only: tests/kmer_model.py -- the numpy statement the kernel-on-host and the GPU tests compare against -- equals what the
reference's count_ngrams(mapping.translate(text), k, radix) answered (tests/golden/kmers, written by tools/record_kmer_golden.py)
when every row loses its last base (drop_last: the reference's loop stops one window early); without drop_last it equals a plain
loop over every window; and the recordings are what the issue asks them to be."""
import os

import numpy as np
import pytest

import kmer_model as K
import twobit_model as M


def as_bytes(text):
    return np.frombuffer(text.encode("ascii"), dtype=np.uint8)


@pytest.mark.parametrize("name", M.FILES)
def test_model_equals_the_recorded_counts_with_drop_last(name):
    entries = K.recorded(name)
    assert entries
    differs = 0
    for case, text, mapping, k, want in entries:
        letters, radix = K.MAPPINGS[mapping]
        table = K.table_of(letters)
        got = K.count_text(as_bytes(text), k, radix, table, drop_last=True)
        assert want.dtype == np.int32 and want.shape == (radix ** k,) and got.dtype == np.int32
        assert np.array_equal(got, want), (name, case, mapping, k)
        every = K.count_text(as_bytes(text), k, radix, table)
        assert 0 <= int(every.sum()) - int(want.sum()) <= 1  # the last window is the only difference
        differs += int(every.sum() != want.sum())
    assert differs > 0  # the quirk shows: some last window is a word


@pytest.mark.parametrize("name", ("test.2bit", "testMask.2bit", "multi.2bit"))
def test_without_drop_last_the_model_is_a_plain_window_loop(name):
    checked = 0
    for case, text, mapping, k, _ in K.recorded(name):
        if len(text) > 400:
            continue
        letters, radix = K.MAPPINGS[mapping]
        table = K.table_of(letters)
        assert np.array_equal(K.count_text(as_bytes(text), k, radix, table), K.count_loop(text.encode("ascii"), k, radix, table)), (name, case, mapping, k)
        checked += 1
    assert checked > 20
    table = K.table_of(K.MAPPINGS["acgt"][0])
    assert K.count_text(as_bytes("ACGTA"), 2, 4, table).tolist() == K.count_loop(b"ACGTA", 2, 4, table).tolist()
    want = np.zeros(16, dtype=np.int32)
    want[[0 + 4 * 1, 1 + 4 * 2, 2 + 4 * 3, 3 + 4 * 0]] = 1  # AC, CG, GT, TA: the first letter least significant
    assert K.count_text(as_bytes("ACGTA"), 2, 4, table).tolist() == want.tolist()
    assert K.count_text(as_bytes("ACNGT"), 2, 4, table).sum() == 2 and K.count_text(as_bytes("AcGT"), 2, 4, table).sum() == 1
    assert K.count_text(as_bytes("A"), 2, 4, table).sum() == 0 and K.count_text(as_bytes(""), 1, 4, table).sum() == 0


def test_the_recordings_cover_what_they_should():
    assert K.KS == (1, 2, 3, 6) and set(K.MAPPINGS) == {"dna", "acgt", "ry"}
    assert K.MAPPINGS["ry"][1] == 2 and K.MAPPINGS["dna"][1] == K.MAPPINGS["acgt"][1] == 4
    dna = K.table_of(K.MAPPINGS["dna"][0])
    assert [int(dna[ord(c)]) for c in "ACGTacgtNn-"] == [0, 1, 2, 3, 0, 1, 2, 3, -1, -1, -1]  # bx.seqmapping.DNA on a 2bit string's letters
    used, masks, windows = set(), set(), {}
    for name in M.FILES:
        pairs = set()
        for case, text, mapping, k, want in K.recorded(name):
            pairs.add((mapping, k))
            masks.add(case["mask"])
            windows[(mapping, k)] = windows.get((mapping, k), 0) + int(want.sum())
        assert pairs == {(m, k) for m in K.MAPPINGS for k in K.KS}, name
        used |= pairs
    assert masks == {True, False} and all(v > 0 for v in windows.values()), windows
    # a masked letter has a digit under "dna" and none under "acgt": the two differ somewhere
    every = [(case, text, mapping, k, want) for name in M.FILES for case, text, mapping, k, want in K.recorded(name)]
    assert any(any(c.islower() for c in text) and want.sum() > 0 for _, text, mapping, _, want in every if mapping == "dna")
    assert any(any(c.islower() for c in text) and "N" not in text and want.sum() < len(text) - k for _, text, mapping, k, want in every if mapping == "acgt")
    # no new file is larger than the largest of tests/golden/twobit; nothing but data
    limit = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN))
    for f in os.listdir(K.GOLDEN):
        assert f.endswith((".npy", ".json")) and os.path.getsize(os.path.join(K.GOLDEN, f)) <= limit, f
