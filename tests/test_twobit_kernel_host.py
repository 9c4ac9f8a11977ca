"""CPU-only: the text of the kernels of bx-python_amd/csrc/twobit.hpp compiled for the host by tests/cpp/twobit_kernel_host.cpp -- a
workgroup of host threads, a barrier for __syncthreads and for the wave shuffle, address and undefined-behaviour sanitizers on, every
table in a buffer of exactly its size, the output between two guard bands -- runs the creation kernels and then gives every
recorded reference string and the model's answer on the structural cases of the GPU tests: rows of one base, rows across tiles,
empty rows, rows inside an N block, more one-base blocks in a segment than a chunk stages, pad on both sides, rows without a
track, the size-0 sequence, widths that are no multiple of 16, an output off a 16-byte boundary, the output cut into slabs; and
the base counts of rows inside one checkpoint block, on checkpoints, over everything, ending at a size that is no multiple of 4.
Then the seeded cases of tests/twobit_cases.py: random sequences that carry every block edge under random ragged rows, windows and
count rows, and a sequence where one segment meets six chunks of one-base blocks and a thread's 16 positions are 16 blocks.
This is the kernels' logic and indexing; tests/test_gpu_twobit.py checks the same cases on the device."""
import numpy as np
import pytest

import kernel_host
import twobit_cases as K
import twobit_model as M

GUARD = 64


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    program = kernel_host.build(tmp_path_factory, "twobit_kernel_host", "twobit kernel host ok")

    def run(seqs, track_of, starts, ends=None, width=0, offsets=None, misalign=0, slab_tiles=0, do_mask=True, pad=ord("N")):
        """bases (ends is None) -> uint8[total]; composition -> int32 [n, 6]; the guard bands are checked here"""
        n = len(track_of)
        mode = 0 if ends is None else 1
        total = 0 if mode else (int(offsets[-1]) if offsets is not None else n * width)

        def write_in(f):
            np.array([mode, len(seqs), n, width, offsets is not None, misalign, slab_tiles, do_mask, pad], dtype=np.int32).tofile(f)
            np.array([total], dtype=np.int64).tofile(f)
            for s in seqs:
                kernel_host.write_arrays(f, ([s.size, len(s.n_starts), len(s.m_starts)], np.int64), (s.packed, np.uint8), (s.n_starts, np.int32),
                                         (s.n_sizes, np.int32), (s.m_starts, np.int32), (s.m_sizes, np.int32))
            kernel_host.write_arrays(f, (track_of, np.int32), (starts, np.int32))
            if mode:
                kernel_host.write_arrays(f, (ends, np.int32))
            if offsets is not None:
                kernel_host.write_arrays(f, (offsets, np.int64))

        if mode:
            words = np.fromfile(program(write_in), dtype=np.int32)
            assert len(words) == 6 * n + 2 * GUARD
            assert (words[:GUARD] == 0x0EEEEEEE).all() and (words[GUARD + 6 * n:] == 0x0EEEEEEE).all(), "written outside the output"
            return words[GUARD:GUARD + 6 * n].reshape(n, 6)
        data = np.fromfile(program(write_in), dtype=np.uint8)
        assert len(data) == total + 2 * GUARD
        assert (data[:GUARD] == 0xEE).all() and (data[GUARD + total:] == 0xEE).all(), "written outside the output"
        return data[GUARD:GUARD + total]

    return run


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@pytest.mark.parametrize("name", M.FILES)
def test_recorded_cases(kernel, name):
    """all recorded regions of a file as ONE ragged batch per do_mask setting, a case the reference refuses as an empty row; their
    base counts against the characters of the recorded strings"""
    for do_mask in (True, False):
        seqs, _, track_of, starts, ends, want = M.recorded_rows(name, do_mask)
        offsets = offsets_of([len(w) for w in want])
        assert [e - s for s, e in zip(starts, ends)] == np.diff(offsets).tolist()
        got = kernel(seqs, track_of, starts, offsets=offsets, do_mask=do_mask)
        assert got.tobytes().decode() == "".join(want), (name, do_mask)
        counts = kernel(seqs, track_of, starts, ends=ends, do_mask=do_mask)
        expect = [[w.upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in w)] for w in want]
        assert counts.tolist() == expect, (name, do_mask)


def test_ragged_structural_cases(kernel):
    seqs = M.structural_sequences()
    model = M.Letters(seqs)
    track_of, starts, lengths = M.ragged_case()
    offsets = offsets_of(lengths)
    for do_mask, pad in ((True, ord("N")), (False, ord("."))):
        want, _ = model.bases(track_of, starts, lengths, do_mask, pad)
        assert np.array_equal(kernel(seqs, track_of, starts, offsets=offsets, do_mask=do_mask, pad=pad), want), do_mask
    want, _ = model.bases(track_of, starts, lengths, True, 0)
    assert np.array_equal(kernel(seqs, track_of, starts, offsets=offsets, misalign=1, pad=0), want), "out one byte past a 16-byte boundary"
    assert np.array_equal(kernel(seqs, track_of, starts, offsets=offsets, slab_tiles=2, pad=0), want), "in slabs of 2 tiles"


@pytest.mark.parametrize("width", M.MATRIX_WIDTHS)
def test_matrix_widths(kernel, width):
    seqs = M.structural_sequences()
    track_of, starts = M.matrix_case(width)
    want = M.Letters(seqs).matrix(track_of, starts, width, True, ord("-"))
    assert np.array_equal(kernel(seqs, track_of, starts, width=width, pad=ord("-")).reshape(-1, width), want), width
    if width in (37, M.TILE + 1):
        got = kernel(seqs, track_of, starts, width=width, pad=ord("-"), slab_tiles=1, misalign=5)
        assert np.array_equal(got.reshape(-1, width), want), (width, "slabs of 1 tile, misaligned")


def test_composition_structural_cases(kernel):
    seqs = M.structural_sequences()
    model = M.Letters(seqs)
    track_of, starts, ends = M.composition_case()
    for do_mask in (True, False):
        want = model.composition(track_of, starts, ends, do_mask)
        assert want[:, :5].any(axis=0).all() and want[:, 5].any() == do_mask
        assert np.array_equal(kernel(seqs, track_of, starts, ends=ends, do_mask=do_mask), want), do_mask


def test_nothing_to_do(kernel):
    seqs = M.structural_sequences()
    assert len(kernel(seqs, [], [], width=5)) == 0
    assert len(kernel(seqs, [0, 1], [3, 4], offsets=np.zeros(3, dtype=np.int64))) == 0
    assert kernel(seqs, [], [], ends=[]).shape == (0, 6)


def through(kernel):
    """the program as the `bases` and `counts` of twobit_cases.check_random_case"""

    def bases(seqs, track_of, starts, do_mask, pad, width=0, lengths=None):
        return kernel(seqs, track_of, starts, width=width, offsets=None if lengths is None else offsets_of(lengths), do_mask=do_mask, pad=pad)

    def counts(seqs, track_of, starts, ends, do_mask):
        return kernel(seqs, track_of, starts, ends=ends, do_mask=do_mask)

    return bases, counts


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_random_sequences(kernel, seed):
    """four random sequences with every block edge (twobit_cases.random_sequence), random ragged rows, windows of widths 1, 37
    and TILE + 1, random base-count rows: tests/test_gpu_twobit.py gives the device the same"""
    K.check_random_case(seed, *through(kernel))


def test_many_chunks_and_sixteen_blocks_in_a_thread(kernel):
    """1500 one-base N blocks in one segment, 1200 adjacent one-base mask blocks, their starts at every byte of a thread's 16"""
    K.check_many_blocks_case(*through(kernel))
