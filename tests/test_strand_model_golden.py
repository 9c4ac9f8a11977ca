"""CPU-only: the model of tests/strand_model.py -- a ten-letter complement table, a reverse, the window loop over the result --
equals every recording of tests/golden/strand: the reference's ``seq.get(s, e).translate(DNA_COMP)[::-1]`` and
``count_ngrams(mapping.translate(that string), k, radix)`` on the recorded regions of every 2bit fixture under both do_mask
settings (tools/record_strand_golden.py).  No answer is skipped: the answers checked are counted against the manifest."""
import numpy as np
import pytest

import kmer_model as K
import strand_model as S
import twobit_model as M


def test_the_complement_table_is_the_reference_s_on_ten_letters():
    assert S.reverse_complement_str("ACGTNacgtn") == "nacgtNACGT"
    assert S.COMPLEMENT[np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)].tobytes() == b"TGCANtgcan"
    others = [c for c in range(256) if chr(c) not in "ACGTNacgtn"]
    assert (S.COMPLEMENT[others] == others).all()  # (pad bytes are nobody's complement)
    assert (S.COMPLEMENT[S.COMPLEMENT] == np.arange(256)).all()


@pytest.mark.parametrize("name", M.FILES)
def test_recorded_letters(name):
    """the model's minus row of every recorded region is the reference's string; it differs from the plus row somewhere"""
    seqs = M.read(name)
    names = list(seqs)
    model = S.Strand([seqs[n] for n in names])
    plus = dict((id(case), text) for case, text in M.recorded(name))
    checked = differ = 0
    for case, want in S.recorded_letters(name):
        s, e = M.case_row(seqs[case["seq"]].size, case)
        got = model.row(names.index(case["seq"]), s, e - s, True, case["mask"]).tobytes().decode()
        assert got == want, (name, case)
        assert S.reverse_complement_str(plus[id(case)]) == want
        differ += want != plus[id(case)]
        checked += 1
    assert checked == len(S.manifest()["files"][name]["strings"]) == sum(text is not None for _, text in M.recorded(name))
    assert differ > checked // 2


@pytest.mark.parametrize("name", M.FILES)
def test_recorded_counts(name):
    """the window loop over the model's minus row, its last letter dropped as the reference's loop drops it"""
    seqs = M.read(name)
    names = list(seqs)
    model = S.Strand([seqs[n] for n in names])
    checked = 0
    for case, mapping, k, want in S.recorded_counts(name):
        letters, radix = K.MAPPINGS[mapping]
        s, e = M.case_row(seqs[case["seq"]].size, case)
        got = model.counts([names.index(case["seq"])], [s], [e - s], [1], k, radix, K.table_of(letters), case["mask"], drop_last=True)[0]
        assert np.array_equal(got, want), (name, case, mapping, k)
        text = model.row(names.index(case["seq"]), s, e - s, True, case["mask"], 0)
        assert np.array_equal(K.count_loop(text[:-1].tobytes(), k, radix, K.table_of(letters)), want)
        checked += 1
    assert checked == len(S.manifest()["files"][name]["entries"]) > 0


def test_a_minus_row_is_the_contract_element_by_element():
    """the model's slice arithmetic against the contract as it is written, with pad on either side, on both, and nowhere"""
    seqs = M.structural_sequences()
    model = S.Strand(seqs)
    for t, start, length in ((0, 100, 40), (0, -7, 20), (0, 20000, 40), (1, -3, 50), (3, 2570, 20), (-1, 5, 9), (2, -2, 3), (0, 3, 0), (1, 5, 1)):
        for do_mask in (True, False):
            got = model.row(t, start, length, True, do_mask, ord("A"))
            assert np.array_equal(got, model.row_loop(t, start, length, do_mask, ord("A"))), (t, start, length)
            plus = model.row(t, start, length, False, do_mask, 0)
            inside = plus != 0
            assert np.array_equal(got, np.where(inside, S.COMPLEMENT[plus], ord("A"))[::-1])  # the plus row reversed, complemented, the pad mirrored


def test_drop_last_shortens_a_minus_row_at_its_start():
    seqs = M.structural_sequences()
    model = S.Strand(seqs)
    table = K.table_of(K.MAPPINGS["dna"][0])
    whole = model.counts([0], [100], [40], [1], 3, 4, table, drop_last=True)
    assert np.array_equal(whole, model.counts([0], [101], [39], [1], 3, 4, table))
    assert not np.array_equal(whole, model.counts([0], [100], [39], [1], 3, 4, table))
