"""A numpy statement of the strand contract of the pwm calls of include/bxmi.h (bxmi_twobit_pwm_scores_strand, _best_strand,
_hits_strand): the three pwm contracts AS WRITTEN, on the string of the row's strand -- pwm_model.Matrix.score on
strand_model.reverse_complement(row) for a minus row -- with its best hit and its hits, and what the pwm strand tests share: the
recordings of tests/golden/pwm_strand (the reference's matrix.score_string(text.translate(DNA_COMP)[::-1])), the batch model
(pwm_cases.Model over the strand's texts, so that every stand-in of pwm_cases is at hand for minus rows too), the genomic start of
a site.  Nothing here goes through bxmi."""
import json
import os

import numpy as np

import pwm_cases as PC
import pwm_hits_cases as H
import pwm_model as P
import strand_model as S
import twobit_model as M

GOLDEN = os.path.join(M.ROOT, "tests", "golden", "pwm_strand")


def score(mat, row, minus):
    """score_string of the row's strand: float32 [len(row)], offsets in the strand's string"""
    return mat.score(S.reverse_complement(row) if minus else row)


def texts(seqs, track_of, starts, lengths, strands, do_mask=True, letters=None):
    """the string of every row's strand, pad 0 (no column in any alphabet) where a position has no letter"""
    letters = letters or PC.letters_of(seqs)
    minus = S.as_minus(strands, len(track_of))
    rows = letters.rows(track_of, starts, lengths, do_mask)
    return [S.reverse_complement(r) if m else r for r, m in zip(rows, minus)]


class Model:
    """scores / best / hits of a stranded batch; `stand_in`: a pwm_cases.Model with one deliberate change"""

    def __init__(self, stand_in=None):
        self.inner = stand_in or PC.MODEL

    def planes(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, rows=None):
        """(sums, scoreable, offsets) as pwm_cases.Model.planes; rows: the strand's texts when the sequences have their own model"""
        n = len(track_of)
        lengths = [width] * n if lengths is None else lengths
        rows = texts(seqs, track_of, starts, lengths, strands, do_mask) if rows is None else rows
        return self.inner.planes(seqs, mats, track_of, starts, lengths, do_mask=do_mask, texts=rows)

    def scores(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, rows=None):
        acc, ok, _ = self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask, rows)
        return np.where(ok, acc, P.NAN)

    def best(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, rows=None, **_):
        return self.inner.best_of_planes(*self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask, rows))

    def hits(self, seqs, mats, track_of, starts, strands, thresholds, lengths=None, width=0, do_mask=True, rows=None):
        acc, ok, offsets = self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask, rows)
        return H.expected(np.where(ok, acc, P.NAN), offsets, thresholds, ok)


MODEL = Model()


def site_starts(starts, lengths, pos, width, minus):
    """the genomic start of the site at offset `pos` of the strand's string: start + pos, or start + len - W - pos on a minus row"""
    starts, lengths, pos, minus = (np.asarray(a) for a in (starts, lengths, pos, minus))
    return np.where(pos < 0, -1, np.where(minus, starts + lengths - width - pos, starts + pos)).astype(np.int64)


# ---- the recordings ----
_manifest = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def recorded(name):
    """[(twobit case, its PLUS string, matrix name, the reference's float32 scores of the reverse complement)] of a fixture"""
    entry = manifest()["files"][name]
    data = np.load(os.path.join(GOLDEN, entry["scores"]))
    cases = M.recorded(name)
    return [(cases[e["case"]][0], cases[e["case"]][1], e["matrix"], data[e["span"][0]:e["span"][1]]) for e in entry["entries"]]


def recorded_batches(name, do_mask):
    """as pwm_model.recorded_batches, every row a minus row: [(matrix names, seqs list, track_of, starts, ends, want)]"""
    seqs = M.read(name)
    names = list(seqs)
    groups = {}
    for case, text, mat, want in recorded(name):
        if case["mask"] != do_mask:
            continue
        key = "".join(P.matrix(mat).sorted_alphabet)
        g = groups.setdefault(key, {"mats": [], "rows": {}, "want": {}})
        if mat not in g["mats"]:
            g["mats"].append(mat)
        s, e = M.case_row(seqs[case["seq"]].size, case)
        row = g["rows"].setdefault((names.index(case["seq"]), s, e), len(g["rows"]))
        g["want"].setdefault(mat, []).append((row, want))
    out = []
    for g in groups.values():
        t, s, e = zip(*g["rows"])
        out.append((g["mats"], [seqs[n] for n in names], list(t), list(s), list(e), g["want"]))
    return out
