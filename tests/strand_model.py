"""A numpy statement of the strand contract of include/bxmi.h (bxmi_twobit_bases_strand, bxmi_twobit_composition_strand,
bxmi_twobit_kmer_counts_strand), of the reference's SeqFile.reverse_complement around it (text.translate(DNA_COMP)[::-1]), and what
the strand tests share: a ten-letter complement table, a reverse, the window loop over the result, the recordings of
tests/golden/strand.  It builds on twobit_model.Letters and kmer_model.count_text; nothing here goes through bxmi."""
import json
import os

import numpy as np

import kmer_model as K
import twobit_model as M

GOLDEN = os.path.join(M.ROOT, "tests", "golden", "strand")

# the ten letters a 2bit string can hold and their complements: the case follows the base, N stays N
COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip("ACGTNacgtn", "TGCANtgcan"):
    COMPLEMENT[ord(_a)] = ord(_b)


def as_minus(strands, n):
    """bool [n] of a strands argument as bxmi.sequence takes it (None: all plus)"""
    if strands is None:
        return np.zeros(n, dtype=bool)
    return np.array([s in ("-", 1, True) for s in strands], dtype=bool)


def reverse_complement(text):
    """of uint8 letters: every letter's complement, in reverse order"""
    return COMPLEMENT[np.asarray(text, dtype=np.uint8)][::-1]


def reverse_complement_str(text):
    return reverse_complement(np.frombuffer(text.encode(), dtype=np.uint8)).tobytes().decode()


class Strand:
    """the contract over a list of sequences"""

    def __init__(self, seqs):
        self.letters = seqs if isinstance(seqs, M.Letters) else M.Letters(seqs)

    def row(self, t, start, length, minus, do_mask=True, pad=ord("N")):
        """uint8 [length]; the positions outside the sequence hold `pad`, mirrored with the letters and not complemented"""
        t, start, length = int(t), int(start), int(length)
        if not minus:
            return self.letters.row(t, start, length, do_mask, pad)
        out = np.full(length, pad, dtype=np.uint8)
        if 0 <= t < len(self.letters.seqs):
            whole = self.letters.of(t, do_mask)
            lo, hi = max(start, 0), min(start + length, len(whole))
            if lo < hi:  # positions [lo, hi) are elements start + length - hi .. start + length - 1 - lo, in descending order
                out[start + length - hi:start + length - lo] = COMPLEMENT[whole[lo:hi]][::-1]
        return out

    def row_loop(self, t, start, length, do_mask=True, pad=ord("N")):
        """a minus row by the contract as it is written: element j is position start + (length - 1 - j)"""
        out = np.full(length, pad, dtype=np.uint8)
        if 0 <= t < len(self.letters.seqs):
            whole = self.letters.of(t, do_mask)
            for j in range(length):
                p = start + (length - 1 - j)
                if 0 <= p < len(whole):
                    out[j] = COMPLEMENT[whole[p]]
        return out

    def bases(self, track_of, starts, lengths, strands, do_mask=True, pad=ord("N")):
        """(bytes uint8 [total], offsets int64 [n + 1])"""
        minus = as_minus(strands, len(starts))
        rows = [self.row(t, s, n, m, do_mask, pad) for t, s, n, m in zip(track_of, starts, lengths, minus)]
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        return (np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8)), offsets

    def matrix(self, track_of, starts, width, strands, do_mask=True, pad=ord("N")):
        return self.bases(track_of, starts, [width] * len(starts), strands, do_mask, pad)[0].reshape(len(starts), width)

    def composition(self, track_of, starts, ends, strands, do_mask=True):
        """int32 [n, 6] = A, C, G, T, N, masked by counting the characters of the strand's letters of the clipped row"""
        minus = as_minus(strands, len(starts))
        out = np.zeros((len(starts), 6), dtype=np.int32)
        for i, (t, s, e) in enumerate(zip(track_of, starts, ends)):
            if not 0 <= t < len(self.letters.seqs):
                continue
            s, e = max(int(s), 0), min(int(e), self.letters.seqs[t].size)
            if s >= e:
                continue
            text = self.row(t, s, e - s, minus[i], do_mask)
            upper = text & ~np.uint8(0x20)
            out[i] = [int((upper == ord(c)).sum()) for c in "ACGTN"] + [int((text >= ord("a")).sum())]
        return out

    def counts(self, track_of, starts, lengths, strands, k, radix, table, do_mask=True, drop_last=False):
        """int32 [n, radix ** k]: the window loop over the strand's string (pad 0: no digit); with drop_last the STRAND's string
        loses its last letter first"""
        minus = as_minus(strands, len(starts))
        out = np.zeros((len(starts), radix ** k), dtype=np.int32)
        for i, (t, s, n) in enumerate(zip(track_of, starts, lengths)):
            out[i] = K.count_text(self.row(t, s, n, minus[i], do_mask, 0), k, radix, table, drop_last)
        return out


# ---- the recordings ----
_manifest = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def recorded_letters(name):
    """[(twobit case, the reference's reverse-complemented string)] of a fixture: every recorded case the reference answers"""
    entry = manifest()["files"][name]
    data = np.load(os.path.join(GOLDEN, entry["letters"]))
    cases = M.recorded(name)
    return [(cases[c][0], data[a:b].tobytes().decode()) for c, a, b in entry["strings"]]


def recorded_counts(name):
    """[(twobit case, mapping name, k, the reference's int32 [radix ** k] counts of the reverse-complemented string)]"""
    entry = manifest()["files"][name]
    data = np.load(os.path.join(GOLDEN, entry["counts"]))
    cases = M.recorded(name)
    out = []
    for c, mapping, k, a, b in entry["entries"]:
        counts = np.zeros(K.MAPPINGS[mapping][1] ** k, dtype=np.int32)
        counts[data[0, a:b]] = data[1, a:b]
        out.append((cases[c][0], mapping, k, counts))
    return out


def recorded_rows(name, do_mask):
    """the recorded strings of one do_mask setting as a minus batch: (seqs list, track_of, starts, ends, want strings)"""
    seqs = M.read(name)
    names = list(seqs)
    t, s, e, want = [], [], [], []
    for case, text in recorded_letters(name):
        if case["mask"] != do_mask:
            continue
        a, b = M.case_row(seqs[case["seq"]].size, case)
        t.append(names.index(case["seq"]))
        s.append(a)
        e.append(b)
        want.append(text)
    return [seqs[n] for n in names], t, s, e, want


def recorded_batches(name, do_mask):
    """the recorded counts of one do_mask setting grouped by (mapping, k), one ragged minus batch each:
    [(mapping name, k, seqs list, track_of, starts, ends, want int32 [rows, bins])]"""
    seqs = M.read(name)
    names = list(seqs)
    groups = {}
    for case, mapping, k, want in recorded_counts(name):
        if case["mask"] != do_mask:
            continue
        s, e = M.case_row(seqs[case["seq"]].size, case)
        g = groups.setdefault((mapping, k), ([], [], [], []))
        for part, value in zip(g, (names.index(case["seq"]), s, e, want)):
            part.append(value)
    return [(mapping, k, [seqs[n] for n in names], t, s, e, np.array(w, dtype=np.int32)) for (mapping, k), (t, s, e, w) in groups.items()]
