"""A numpy statement of the contract of bxmi_twobit_kmer_counts (include/bxmi.h), of the reference's
count_ngrams(mapping.translate(text), k, radix) around it, and what the k-mer tests share: the mappings, the recorded counts of
tests/golden/kmers.  It builds on twobit_model.Letters: the string of a row is the model's own letters.  A mapping is a table
int16 [256] from a character to its digit (-1: none), made here from letters and digits, never through bxmi.kmers."""
import json
import os
import re

import numpy as np

import twobit_model as M

ROOT = M.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmers")
THREADS, RUN, TILE, BINS_MAX, LDS_BINS, CUT = 256, 8, 2048, 16384, 4096, 384  # of csrc/kmer.hpp (tests/test_kmer_abi.py checks them against its text)
KM_SLAB_CELLS = 1 << 24  # of csrc/sequence.hip: counters per slab of rows of bxmi_twobit_kmer_counts
LETTERS = "TCAGtcag"     # the order of the C ABI's digits[8]: 4 * lower_case + code
KS = (1, 2, 3, 6)        # the recorded k

# the recorded mappings: name -> (letter -> digit, radix); "dna" is bx.seqmapping.DNA on the letters a 2bit string can hold
MAPPINGS = {
    "dna": ({"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}, 4),
    "acgt": ({"A": 0, "C": 1, "G": 2, "T": 3}, 4),
    "ry": ({"A": 0, "G": 0, "C": 1, "T": 1}, 2),
}
# how bxmi.kmers is asked for the same: name -> (alphabet, case_sensitive)
ALPHABETS = {"dna": ("ACGT", False), "acgt": ("ACGT", True), "ry": ({"A": 0, "G": 0, "C": 1, "T": 1}, True)}


def kernel_constants():
    """KM_THREADS, KM_RUN, KM_TILE, KM_BINS_MAX, KM_LDS_BINS, KM_CUT as csrc/kmer.hpp states them"""
    text = open(os.path.join(ROOT, "bx-python_amd", "csrc", "kmer.hpp")).read()
    threads, run, bins_max, lds_bins, cut = (int(re.search(r"constexpr int KM_%s = (\d+);" % k, text).group(1))
                                             for k in ("THREADS", "RUN", "BINS_MAX", "LDS_BINS", "CUT"))
    assert re.search(r"constexpr int KM_TILE = KM_RUN \* KM_THREADS;", text)
    return threads, run, run * threads, bins_max, lds_bins, cut


def table_of(letter_digits):
    """int16 [256]: the digit of every character, -1 for none"""
    table = np.full(256, -1, dtype=np.int16)
    for ch, d in letter_digits.items():
        table[ord(ch)] = d
    return table


def digits8(table):
    """int8 [8]: the C ABI's digits of a table"""
    return np.array([table[ord(ch)] for ch in LETTERS], dtype=np.int8)


def use_lds(bins, windows, force=0):
    """km_use_lds of csrc/kmer.hpp"""
    if bins > LDS_BINS or force == 2:
        return False
    return True if force == 1 else windows >= CUT


def count_text(text, k, radix, table, drop_last=False):
    """int32 [radix ** k] of uint8 letters: every window whose k letters have a digit, at sum(digit[t] * radix ** t); with
    drop_last the text loses its last letter first (the reference's loop)"""
    d = table[np.asarray(text, dtype=np.uint8)].astype(np.int64)
    if drop_last:
        d = d[:-1]
    n = len(d) - k + 1
    bins = radix ** k
    if n <= 0:
        return np.zeros(bins, dtype=np.int32)
    ok, index = np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64)
    for t in range(k):
        c = d[t:t + n]
        ok &= c >= 0
        index += np.maximum(c, 0) * radix ** t
    return np.bincount(index[ok], minlength=bins).astype(np.int32)


def count_loop(text, k, radix, table):
    """the same by a plain loop over the windows, the last one included"""
    out = np.zeros(radix ** k, dtype=np.int32)
    d = [int(table[c]) for c in bytes(text)]
    for j in range(len(d) - k + 1):
        word = d[j:j + k]
        if min(word) >= 0:
            out[sum(x * radix ** t for t, x in enumerate(word))] += 1
    return out


class Counts:
    """the contract over a list of sequences"""

    def __init__(self, seqs):
        self.letters = seqs if isinstance(seqs, M.Letters) else M.Letters(seqs)

    def counts(self, track_of, starts, lengths, k, radix, table, do_mask=True, drop_last=False):
        """int32 [n, radix ** k]; pad 0: a position outside the sequence, or of a row without a track, has no digit"""
        out = np.zeros((len(starts), radix ** k), dtype=np.int32)
        for i, (t, s, n) in enumerate(zip(track_of, starts, lengths)):
            out[i] = count_text(self.letters.row(int(t), int(s), int(n), do_mask, 0), k, radix, table, drop_last)
        return out


# ---- the recorded counts ----
_manifest = None


def manifest():
    global _manifest
    if _manifest is None:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            _manifest = json.load(f)
    return _manifest


def recorded(name):
    """[(twobit case, its string, mapping name, k, the reference's int32 [radix ** k] counts)] of a fixture; the counts are stored
    as the non-zero (index, count) pairs"""
    entry = manifest()["files"][name]
    data = np.load(os.path.join(GOLDEN, entry["counts"]))
    cases = M.recorded(name)
    out = []
    for case, mapping, k, a, b in entry["entries"]:
        counts = np.zeros(MAPPINGS[mapping][1] ** k, dtype=np.int32)
        counts[data[0, a:b]] = data[1, a:b]
        out.append((cases[case][0], cases[case][1], mapping, k, counts))
    return out


def recorded_batches(name, do_mask):
    """the recorded entries of one do_mask setting grouped by (mapping, k), one ragged batch each:
    [(mapping name, k, seqs list, track_of, starts, ends, want int32 [rows, bins])]"""
    seqs = M.read(name)
    names = list(seqs)
    groups = {}
    for case, _, mapping, k, want in recorded(name):
        if case["mask"] != do_mask:
            continue
        s, e = M.case_row(seqs[case["seq"]].size, case)
        g = groups.setdefault((mapping, k), ([], [], [], []))
        for part, value in zip(g, (names.index(case["seq"]), s, e, want)):
            part.append(value)
    return [(mapping, k, [seqs[n] for n in names], t, s, e, np.array(w, dtype=np.int32)) for (mapping, k), (t, s, e, w) in groups.items()]
