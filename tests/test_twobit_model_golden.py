"""CPU-only: tests/twobit_model.py gives every string tools/record_twobit_golden.py recorded from the reference's bx.seq.twobit
(TwoBitSequence.get and __getitem__, do_mask True and False), byte for byte, and raises what the reference raised with the same
message; no recorded case is left out.  The composition of the model is checked against counts taken from the recorded strings."""
import collections

import numpy as np
import pytest

import twobit_model as M


@pytest.mark.parametrize("name", M.FILES)
def test_every_recorded_case(name):
    seqs = M.read(name)
    whole = M.Letters(seqs.values())
    names = list(seqs)
    cases = M.recorded(name)
    assert len(cases) == len(M.manifest()["files"][name]["cases"]) and len(cases) >= 36
    seen = collections.Counter()
    for case, text in cases:
        kind, got = M.apply_case(whole.of(names.index(case["seq"]), case["mask"]), case)
        if text is None:
            assert (kind, got) == ("error", case["error"]), case
        else:
            assert (kind, got) == ("ok", text), case
        seen[kind] += 1
    assert seen["ok"] and seen["error"]


def test_swap_records_what_blocks_records():
    a, b = M.recorded("blocks.2bit"), M.recorded("swap.2bit")
    assert [(c["args"], c["mask"], t) for c, t in a] == [(c["args"], c["mask"], t) for c, t in b]


def test_fixture_sizes_match_the_manifest():
    for name in M.FILES:
        assert {k: s.size for k, s in M.read(name).items()} == M.manifest()["files"][name]["sizes"], name


@pytest.mark.parametrize("name", ("blocks.2bit", "multi.2bit", "testMask.2bit"))
def test_model_composition_counts_the_recorded_characters(name):
    for do_mask in (True, False):
        seqs, _, track_of, starts, ends, want = M.recorded_rows(name, do_mask)
        got = M.Letters(seqs).composition(track_of, starts, ends, do_mask)
        for row, text in zip(got, want):
            counts = [text.upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in text)]
            assert row.tolist() == counts, text[:40]
        assert (got[:, 4].any() or name == "testMask.2bit") and (got[:, 5].any() == do_mask)


def test_the_references_own_fasta_files_agree():
    """the .fa beside each of the reference's .2bit files holds the same letters (compared in upper case), blanks inside its lines aside"""
    import os

    for stem in ("test", "testN", "testMask"):
        fasta, name = {}, None
        for line in open(os.path.join(M.GOLDEN, stem + ".fa")):
            if line.startswith(">"):
                name = line[1:].split()[0]
                fasta[name] = ""
            elif name:
                fasta[name] += "".join(line.split())
        seqs = M.read(stem + ".2bit")
        assert list(seqs) == list(fasta)
        for k, seq in seqs.items():
            assert M.letters(seq, do_mask=False).tobytes().decode().upper() == fasta[k].upper(), (stem, k)
