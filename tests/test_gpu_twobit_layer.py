"""
The four kernels that walk a batch of 2bit rows segment by segment (csrc/twobit.hpp's row-segment layer under the letters and the
k-mer counts, the same walk as their own text in pwm.hpp and pwm_hits.hpp) at once: ONE ragged batch goes through bxmi_twobit_bases_dev,
bxmi_twobit_pwm_scores_dev, bxmi_twobit_pwm_hits_dev and bxmi_twobit_kmer_counts_dev, and the four answers are held to each other
and to the numpy models (tests/twobit_model.py, pwm_model.py, kmer_model.py).  The matrix has width 1 and scores a letter with its
class index, so a score NAMES the letter the scoring kernel decoded; at -inf every scored element is a hit; at k = 1 a row's counts
are the bincount of its letters.  Every comparison is exact.

The batch (under 40 000 elements): two sequences of about 20 000 bases and rows that name no track; 300 mask blocks of 1 to 3
bases inside the 1024 positions of the first row, which is one segment in every kernel (tiles of 1024, 2048 and 4096 elements), so
the chunk loop over the staged blocks takes two rounds in each; rows that start below 0 and rows that end past the size; empty
rows between others; rows that end exactly at elements 1024, 2048 and 4096; a row longer than 4096; both do_mask settings.
"""
import numpy as np
import pytest

import kmer_model as K
import pwm_hits_cases as H
import pwm_model as P
import twobit_cases as TC
import twobit_model as M

CLASSES = "TCAGNtcagn"  # pwm.hpp's letter classes
PAD = ord(".")
MATRIX = P.Matrix(CLASSES, [list(range(len(CLASSES)))])  # width 1: the score of a letter is its class
TABLE = K.table_of({ch: CLASSES.index(ch.upper()) for ch in "TCAGtcag"})  # k-mer digits: the code, whatever the case
STRETCH = 5000  # where the mask blocks of 1 to 3 bases begin


def batch():
    """(seqs, track_of, starts, lengths)"""
    rng = np.random.default_rng(20261020)
    sizes = (20011, 19997)
    packed = [rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8) for size in sizes]
    m_sizes = [1 + k % 3 for k in range(M.CHUNK + 44)]  # 300 blocks, a base between them: 899 positions
    m_starts = (STRETCH + np.concatenate([[0], np.cumsum(np.array(m_sizes[:-1]) + 1)])).tolist()
    assert len(m_starts) > M.CHUNK and m_starts[-1] + m_sizes[-1] <= STRETCH + 1024
    seqs = [TC.sequence_of(sizes[0], [0, 3100, 19000], [9, 40, 1011], m_starts + [9000], m_sizes + [700], packed[0]),
            TC.sequence_of(sizes[1], [50, 10000], [2000, 1], [0, 19990], [120, 7], packed[1])]
    rows = [(0, STRETCH, 1024),                        # the stretch in one segment; ends at element 1024
            (0, -7, 500), (1, 0, 0), (1, sizes[1] - 100, 524),  # below 0; empty; past the size, ends at element 2048
            (0, 0, 0), (2, 10, 48), (-1, 3, 52), (0, 9, 0),     # rows that name no track, empty rows
            (1, 100, 1948),                            # ends at element 4096
            (0, 3000, 4096 + 777),                     # longer than any tile, the stretch across tile boundaries
            (1, -20, sizes[1] + 50), (0, 19990, 30), (0, STRETCH + 1, 1), (0, STRETCH + 2, 1), (1, 49, 3)]
    t, s, n = (list(x) for x in zip(*rows))
    ends = np.cumsum(n)
    assert ends[0] == 1024 and ends[3] == 2048 and ends[8] == 4096 and max(n) > 4096 and ends[-1] < 40000
    return seqs, t, s, n


def letters_of_scores(plane):
    """the letters a plane of MATRIX's scores names, PAD where it holds a NaN"""
    named = np.frombuffer(CLASSES.encode(), dtype=np.uint8)[np.nan_to_num(plane, nan=0.0).astype(np.int64)]
    return np.where(np.isnan(plane), np.uint8(PAD), named)


def counts_of_letters(letters, offsets):
    """int32 [n, 4]: per row the bincount of the codes of its letters that are one of TCAG in either case"""
    code = np.full(256, -1, dtype=np.int64)
    for ch in "TCAGtcag":
        code[ord(ch)] = CLASSES.index(ch.upper())
    out = np.zeros((len(offsets) - 1, 4), dtype=np.int32)
    for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        c = code[letters[a:b]]
        out[i] = np.bincount(c[c >= 0], minlength=4)
    return out


@pytest.fixture(scope="module")
def models():
    """per do_mask: (letters, offsets, plane, hits, counts) of the three models on the batch"""
    seqs, t, s, n = batch()
    whole = M.Letters(seqs)
    out = {}
    for do_mask in (True, False):
        letters, offsets = whole.bases(t, s, n, do_mask, PAD)
        plane = P.Scores(whole).scores(t, s, n, [MATRIX], do_mask)
        counts = K.Counts(whole).counts(t, s, n, 1, 4, TABLE, do_mask)
        out[do_mask] = (letters, offsets, plane, H.expected(plane, offsets, -H.INF), counts)
    return out


@pytest.mark.parametrize("do_mask", (True, False))
def test_models_agree_on_the_batch(models, do_mask):
    """no GPU: what the device is held to is consistent in itself"""
    letters, offsets, plane, (mat_hits, rows, pos, score), counts = models[do_mask]
    assert np.array_equal(letters_of_scores(plane[0]), letters)
    assert (letters != PAD).sum() > 28000 and ((letters >= ord("a")).sum() > 1000) == do_mask and (letters == ord("N")).sum() > 3000
    assert mat_hits.tolist() == [0, int((letters != PAD).sum())]
    assert np.array_equal(offsets[rows] + pos, np.flatnonzero(letters != PAD)) and P.bits(score).tolist() == P.bits(plane[0][offsets[rows] + pos]).tolist()
    assert np.array_equal(counts_of_letters(letters, offsets), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("do_mask", (True, False))
def test_four_consumers_of_one_batch(models, do_mask):
    from bxmi import sequence

    from test_gpu_kmers import counts_dev
    from test_gpu_pwm import device_set, same_bits, scores_dev
    from test_gpu_pwm_hits import hits_dev
    from test_gpu_twobit import bases_dev

    seqs, t, s, n = batch()
    want_letters, offsets, want_plane, want_hits, want_counts = models[do_mask]
    tracks = [sequence.TwoBitTrack(q) for q in seqs]
    ms = device_set([MATRIX])
    try:
        letters = bases_dev(tracks, t, s, do_mask, PAD, lengths=n)
        plane = scores_dev(tracks, ms, t, s, lengths=n, do_mask=do_mask)
        rc, (mat_hits, rows, pos, score) = hits_dev(tracks, ms, t, s, -H.INF, lengths=n, do_mask=do_mask)
        counts = counts_dev(tracks, t, s, 1, 4, K.digits8(TABLE), lengths=n, do_mask=do_mask)
    finally:
        ms.close()
        for track in tracks:
            track.close()
    # each against its model
    assert np.array_equal(letters, want_letters)
    assert same_bits(plane, want_plane)
    assert rc == 0
    H.assert_hits((mat_hits, rows, pos, score), want_hits)
    assert np.array_equal(counts, want_counts)
    # and against each other
    assert np.array_equal(letters_of_scores(plane[0]), letters)
    assert np.array_equal(offsets[rows] + pos, np.flatnonzero(~np.isnan(plane[0]))) and np.array_equal(P.bits(score), P.bits(plane[0][offsets[rows] + pos]))
    assert np.array_equal(counts_of_letters(letters, offsets), counts)
