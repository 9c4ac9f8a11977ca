"""CPU-only: the two fast models of tests/twobit_cases.py -- the letters of a window from the packed bytes under it, the base counts
from running counts -- agree with the whole-sequence models of tests/twobit_model.py (which tests/test_twobit_model_golden.py pins to
the reference's recorded strings) on random sequences and random rows, and the seeded cases hold the conditions without which the
tests on them (test_twobit_kernel_host, test_gpu_twobit) would pass vacuously."""
import numpy as np
import pytest

import twobit_cases as K
import twobit_model as M


@pytest.mark.parametrize("seed", (401, 402))
def test_fast_models_agree_with_the_whole_sequence_models(seed):
    """three random sequences of at most 60 000 bases, 5 000 random rows: rows beyond both ends, empty and reversed ones, rows
    that name no sequence"""
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(K.EDGE_SIZE, 60001)), int(rng.choice(K.RANDOM_SIZES)), 60000]
    seqs = [K.random_sequence(rng, size, max(size // 200, 3), max(size // 60, 3)) for size in sizes]
    for seq in (seqs[0], seqs[2]):
        assert all(K.edges_of(seq).values())
    n = 5000
    track_of = rng.integers(-1, len(seqs), n)
    size_of = np.array(sizes + [0])[track_of]
    starts = rng.integers(-50, size_of + 51)
    lengths = K.log_uniform(rng, 1, 3 * M.TILE + 1, n) - 1
    ends = starts + lengths
    ends[:300] = rng.integers(-50, size_of[:300] + 51)  # arbitrary ends: reversed rows among them
    ends[300:350] = starts[300:350]
    whole = M.Letters(seqs)
    for do_mask in (True, False):
        for t, s, e in zip(track_of.tolist(), starts.tolist(), ends.tolist()):
            length = max(e - s, 0)
            assert np.array_equal(K.window_row(seqs, t, s, length, do_mask, ord(".")), whole.row(t, s, length, do_mask, ord("."))), (t, s, e, do_mask)
        want = whole.composition(track_of, starts, ends, do_mask)
        assert np.array_equal(K.composition_of(seqs, track_of, starts, ends, do_mask), want), do_mask
        assert (want > 0).any(axis=0).tolist() == [True] * 5 + [do_mask] and (want.sum(axis=1) == 0).any()
    got = K.window_bases(seqs, track_of[:50], starts[:50], lengths[:50])
    assert np.array_equal(got, whole.bases(track_of[:50], starts[:50], lengths[:50])[0])


def test_windows_of_whole_sequences_and_of_nothing():
    rng = np.random.default_rng(403)
    padding = []
    for size in K.RANDOM_SIZES:
        seq = K.random_sequence(rng, size, max(size // 200, 5), max(size // 60, 7))
        padding.append(int(seq.packed[-1]) & ((1 << 2 * (-size % 4)) - 1))  # the bits behind the last base
        for do_mask in (True, False):
            whole = M.letters(seq, do_mask)
            assert np.array_equal(K.window(seq, 0, size, do_mask), whole)
            for a in range(0, min(size, 9)):
                assert np.array_equal(K.window(seq, a, size, do_mask), whole[a:]) and len(K.window(seq, a, a)) == 0
            assert K.composition(whole, [0, -3, 1], [size, size + 3, 0]).tolist() == [K.counts_of_letters(whole)] * 2 + [[0] * 6]
    assert any(padding)  # they stay random


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_random_cases_have_their_edges(seed):
    case = K.random_case(seed)
    seqs = case["seqs"]
    assert len(seqs) == 4 and all(s.size in K.RANDOM_SIZES for s in seqs[:3]) and K.EDGE_SIZE <= seqs[3].size <= 40000
    assert all(K.edges_of(seqs[3]).values())
    assert sorted(case["matrix"]) == sorted(K.RANDOM_WIDTHS) and all(len(t) == len(s) > 0 for t, s in case["matrix"].values())
    t, s, e = case["comp"]
    assert len(t) == len(s) == len(e) == len(case["track_of"]) + 200
    assert K.random_case(seed) is case  # made once


def test_many_blocks_case_fills_chunks_and_threads():
    case = K.many_blocks_case()
    seq = case["seqs"][0]
    assert seq.size == 3 * M.TILE and case["most"] >= 5 * M.CHUNK
    (n0, n_count), (m0, m_count) = K.STRETCH_N, K.STRETCH_M
    n = np.flatnonzero(seq.n_starts == n0)[0]
    assert (seq.n_sizes[n:n + n_count] == 1).all() and (np.diff(seq.n_starts[n:n + n_count]) == 2).all() and n_count == 1500
    m = np.flatnonzero(seq.m_starts == m0)[0]
    assert (seq.m_sizes[m:m + m_count] == 1).all() and (np.diff(seq.m_starts[m:m + m_count]) == 1).all() and m_count == 1200
    # a thread's 16 bytes inside the mask stretch are 16 blocks: the first row that holds the stretch begins on a thread's byte 0
    offsets = np.concatenate([[0], np.cumsum(case["lengths"])])
    assert offsets[1] % 16 == 0 and case["lengths"][1] >= m_count + 32
    t, s, e = case["comp"]
    for first, past in ((n0, n0 + 2 * n_count - 1), (m0, m0 + m_count)):
        for d in range(40):
            assert ((s == first + d) & (e > past)).any() and ((e == first + d + 1) & (s < first)).any()
            assert ((s == past - 40 + d) & (e > past)).any() and ((e == past - 40 + d + 1) & (s < first)).any()


@pytest.mark.parametrize("which", (0, 1))
def test_big_sequences_cross_the_scan_tiles(which):
    """what tests/test_gpu_twobit.py::test_tables_beyond_one_scan_tile relies on"""
    seq, facts = K.big_conditions(which)
    assert seq.size == K.BIG_SIZES[which] and facts["stride"] % 4 == (2, 0)[which] and facts["stride"] > 2 * K.SCAN_TILE
    assert (len(seq.n_starts) + 1) % 2 == 1 and len(seq.n_starts) + 1 > 3 * K.SCAN_TILE
    assert facts["rows over N block 2048"] > 0 and facts["rows over checkpoint 2048"] > 0
