"""CPU-only: tests/scores_model.py reproduces, as text, every output the reference's scripts/aggregate_scores_in_intervals.py
recorded under tests/golden/scores (tools/record_scores_golden.py); the synthetic fixture can tell an ordered float32 chain from
other summations; bxmi.wiggle reads the fixtures as the model does, and bxmi.scores.format_row prints as the reference does."""
import json
import os

import numpy as np
import pytest

import scores_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scores")


def _manifest():
    path = os.path.join(GOLDEN, "manifest.json")
    return json.load(open(path)) if os.path.exists(path) else []


MANIFEST = _manifest()
_cache = {}


def golden_lines(name):
    """the lines of a fixture (gzipped or not), read once"""
    if name not in _cache:
        with M.open_text(os.path.join(GOLDEN, name)) as f:
            _cache[name] = f.readlines()
    return _cache[name]


def recorded(case):
    with open(os.path.join(GOLDEN, case["expected"])) as f:
        return f.read()


def model_tracks(name):
    key = ("tracks", name)
    if key not in _cache:
        _cache[key] = M.load_wiggle(golden_lines(name))
    return _cache[key]


def test_manifest_lists_the_four_cases():
    assert [c["expected"] for c in MANIFEST] == ["hand.out", "hand.masked.out", "syn.out", "syn.masked.out"]
    assert [c["mask"] is not None for c in MANIFEST] == [False, True, False, True]


@pytest.mark.parametrize("k", range(4))
def test_model_equals_the_recorded_text(k):
    case = MANIFEST[k]
    mask = golden_lines(case["mask"]) if case["mask"] else None
    got = M.run(golden_lines(case["scores"]), golden_lines(case["intervals"]), mask)
    want = recorded(case)
    assert want.count("\n") == case["lines"]
    assert got.split("\n") == want.split("\n")


def test_hand_case_holds_what_it_is_for():
    text = recorded(MANIFEST[0])
    assert "\t0.33333334\t" in text                       # the float32 quotient, not 0.3333333333333333
    assert "\t100000000\t" in text and text.count("\t-100000000\n") >= 1  # the int sentinels survive
    assert "chr1\t30\t31\t1.0\t1.0\t1.0\n" in text       # 1.0000000596046447754 -> double -> float32 is 1.0
    assert "chrUn\t0\t10\tnan\tnan\tnan\n" in text


def test_synthetic_case_tells_an_ordered_chain_from_a_tree():
    rows = [line.split() for line in golden_lines("syn.bed")]
    for chrom, track in model_tracks("syn.wig.gz").items():
        mine = [(int(r[1]), int(r[2])) for r in rows if r[0] == chrom]
        frac = M.fraction_order_sensitive(track, [s for s, _ in mine], [e for _, e in mine])
        assert frac >= 0.5, (chrom, frac)
    starts = np.array([int(r[1]) for r in rows])
    assert sorted(set(starts % 64)) == list(range(64))
    assert len(set(map(tuple, rows))) < len(rows) and (np.diff(starts) < 0).any()  # duplicates, unsorted


@pytest.mark.parametrize("name", ["hand.wig", "syn.wig.gz"])
def test_wiggle_reader_matches_the_model(name):
    from bxmi import wiggle

    spans = wiggle.read_spans_file(os.path.join(GOLDEN, name))
    model = model_tracks(name)
    assert list(spans) == list(model)
    for chrom, (s, e, v) in spans.items():
        assert s.dtype == np.int64 and e.dtype == np.int64 and v.dtype == np.float32
        track = M.fill(int(e.max()), s, e, v)
        assert track.view(np.uint32).tolist() == model[chrom].view(np.uint32).tolist(), chrom
    assert wiggle.read_spans(golden_lines(name)).keys() == spans.keys()


@pytest.mark.parametrize("k", range(4))
def test_format_row_prints_the_reference_lines(k):
    from bxmi import scores

    case = MANIFEST[k]
    tracks = model_tracks(case["scores"])
    masks = M.load_mask(golden_lines(case["mask"])) if case["mask"] else {}
    out = []
    for line in golden_lines(case["intervals"]):
        f = line.split()
        chrom, s, e = f[0], int(f[1]), int(f[2])
        c, t, a, b = M.aggregate(tracks[chrom], [s], [e], masks.get(chrom)) if chrom in tracks else ([0], [0.0], [0.0], [0.0])
        out.append(scores.format_row(chrom, s, e, c[0], t[0], a[0], b[0]) + "\n")
    assert "".join(out) == recorded(case)
