"""CPU-only: the text of the kernels of bx-python_amd/csrc/pwm.hpp compiled for the host by tests/cpp/pwm_kernel_host.cpp -- a
workgroup of host threads, a barrier for __syncthreads and for the wave maximum, a lock for the atomic maximum, address and
undefined-behaviour sanitizers on, -ffp-contract=off, every table in a buffer of exactly its size, the output planes between two
guard bands -- gives every recorded answer of the reference bit for bit and the model's answer on the structural cases of the GPU
tests.  This is the kernels' logic, indexing and order of additions; tests/test_gpu_pwm.py checks the same cases on the device.  The seeded cases of
tests/pwm_cases.py -- random matrices, sets at the LDS boundary, infinities and arithmetic NaNs, the best hit on sampled lanes, more
tiles than the grid, the phases of the top of int32 -- run here sized down."""
import numpy as np
import pytest

import kernel_host
import pwm_cases as PC
import pwm_model as P
import twobit_model as M

GUARD = 64
GUARD_BITS = 0xEEEEEEEE


def letter_col(mat):
    return np.array([mat.char_to_index[ord(ch)] for ch in P.LETTERS], dtype=np.int8)


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    program = kernel_host.build(tmp_path_factory, "pwm_kernel_host", "pwm kernel host ok")

    def run(seqs, mats, track_of, starts, width=0, offsets=None, best=False, misalign=0, slab_tiles=0, do_mask=True, grid=0, total=None):
        """scores -> float32 [n_mats, total]; best -> (float32 [n_mats, n], int32 [n_mats, n]); the guard bands are checked here"""
        n, n_mats = len(track_of), len(mats)
        if total is None:
            total = int(offsets[-1]) if offsets is not None else n * width

        def write_in(f):
            np.array([best, len(seqs), n, width, offsets is not None, misalign, slab_tiles, do_mask, n_mats, mats[0].values.shape[1], grid],
                     dtype=np.int32).tofile(f)
            np.array([total], dtype=np.int64).tofile(f)
            kernel_host.write_arrays(f, (letter_col(mats[0]), np.int8), (np.concatenate([[0], np.cumsum([m.width for m in mats])]), np.int32),
                                     (np.concatenate([m.values for m in mats]), np.float32))
            for s in seqs:
                kernel_host.write_arrays(f, ([s.size, len(s.n_starts), len(s.m_starts)], np.int64), (s.packed, np.uint8), (s.n_starts, np.int32),
                                         (s.n_sizes, np.int32), (s.m_starts, np.int32), (s.m_sizes, np.int32))
            kernel_host.write_arrays(f, (track_of, np.int32), (starts, np.int32))
            if offsets is not None:
                kernel_host.write_arrays(f, (offsets, np.int64))

        words = np.fromfile(program(write_in), dtype=np.uint32)

        def body(part, cells):
            assert len(part) == cells + 2 * GUARD
            assert (part[:GUARD] == GUARD_BITS).all() and (part[GUARD + cells:] == GUARD_BITS).all(), "written outside the output"
            return part[GUARD:GUARD + cells]

        if best:
            cells = n_mats * n
            half = cells + 2 * GUARD
            return body(words[:half], cells).view(np.float32).reshape(n_mats, n), body(words[half:], cells).view(np.int32).reshape(n_mats, n)
        return body(words, n_mats * total).view(np.float32).reshape(n_mats, total)

    return run


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def same_bits(got, want):
    return np.array_equal(P.bits(got), P.bits(want))


@pytest.mark.parametrize("name", M.FILES)
def test_recorded_cases(kernel, name):
    """the recorded regions of a file as one ragged batch per do_mask setting and alphabet: the reference's own float32 answers"""
    checked = 0
    for do_mask in (True, False):
        for names, seqs, track_of, starts, ends, want in P.recorded_batches(name, do_mask):
            mats = [P.matrix(k) for k in names]
            offsets = offsets_of([e - s for s, e in zip(starts, ends)])
            got = kernel(seqs, mats, track_of, starts, offsets=offsets, do_mask=do_mask)
            top, at = kernel(seqs, mats, track_of, starts, offsets=offsets, do_mask=do_mask, best=True)
            for m, k in enumerate(names):
                for row, answer in want[k]:
                    assert same_bits(got[m, offsets[row]:offsets[row + 1]], answer), (name, do_mask, k, row)
                    score, pos = P.best_of(answer)
                    assert same_bits(top[m, row], score) and at[m, row] == pos, (name, do_mask, k, row)
                    checked += 1
    assert checked == len(P.manifest()["files"][name]["entries"])


@pytest.mark.parametrize("misalign,slab_tiles", ((0, 0), (1, 0), (0, 2), (3, 1)))
def test_ragged_structural_cases(kernel, misalign, slab_tiles):
    """twobit_model.ragged_case() and the rows placed for the halo, the tile boundary, rows around the width, block edges; widths 1
    and WIDTH_MAX in one handle; planes that total % 4 misaligns; `out` off a 16-byte boundary; the output cut into slabs"""
    seqs = M.structural_sequences()
    model = P.Scores(seqs)
    mats = P.structural_mats()
    track_of, starts, lengths = P.ragged_case()
    if misalign == 1:  # total % 4 == 1: the planes after the first are misaligned too
        lengths = lengths + [1]
        track_of, starts = track_of + [0], starts + [50]
    offsets = offsets_of(lengths)
    for do_mask in (True, False):
        want = model.scores(track_of, starts, lengths, mats, do_mask)
        assert (~np.isnan(want)).any(axis=1).all() and np.isnan(want).any()
        got = kernel(seqs, mats, track_of, starts, offsets=offsets, do_mask=do_mask, misalign=misalign, slab_tiles=slab_tiles)
        assert same_bits(got, want), (do_mask, np.flatnonzero((P.bits(got) != P.bits(want)).any(axis=0))[:10])


@pytest.mark.parametrize("width", (1, 37, P.TILE + 1))
def test_score_matrix_widths(kernel, width):
    seqs = M.structural_sequences()
    track_of, starts = M.matrix_case(width)
    for names in (("w20n", "w4n"), ("w20lc",), ("ninf", "denorm", "zeros")):
        mats = [P.matrix(k) for k in names]
        want = P.Scores(seqs).scores(track_of, starts, [width] * len(starts), mats, True)
        got = kernel(seqs, mats, track_of, starts, width=width, slab_tiles=1 if width == 37 else 0)
        assert same_bits(got, want), (width, names)


def test_best_structural_cases(kernel):
    """the model's NaN-aware maximum and first position: the zeros matrix (every score ties), a row over three tiles with its
    maximum in the last tile and an equal score in the first, rows with no scoreable window, a grid smaller than the tiles and a
    total that is only a bound"""
    seqs = M.structural_sequences()
    model = P.Scores(seqs)
    track_of, starts, lengths = P.ragged_case()
    offsets = offsets_of(lengths)
    mats = [P.matrix("zeros"), P.matrix("w4"), P.matrix("ninf")]
    for do_mask in (True, False):
        want = model.best(track_of, starts, lengths, mats, do_mask)
        assert (want[1] == -1).any() and (want[1][0] > 0).any()  # (the zeros matrix: the first scoreable offset, not always 0)
        for grid, total in ((0, None), (3, int(offsets[-1]) + 5 * P.TILE + 7)):
            got = kernel(seqs, mats, track_of, starts, offsets=offsets, do_mask=do_mask, best=True, grid=grid, total=total)
            assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), (do_mask, grid)
    seq, row_t, row_s, row_n, mat = P.tie_case()
    want = P.Scores([seq]).best(row_t, row_s, row_n, [mat], True)
    got = kernel([seq], [mat], row_t, row_s, offsets=offsets_of(row_n), best=True)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1][0, 1] < P.TILE - 100 and not np.isnan(want[0][0, 1])
    # as windows of one width
    t, s = M.matrix_case(37)
    want = model.best(t, s, [37] * len(s), mats, True)
    got = kernel(seqs, mats, t, s, width=37, best=True)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_nothing_to_do(kernel):
    seqs = M.structural_sequences()
    mats = [P.matrix("w4")]
    assert kernel(seqs, mats, [], [], width=5).shape == (1, 0)
    assert kernel(seqs, mats, [0, 1], [3, 4], offsets=np.zeros(3, dtype=np.int64)).shape == (1, 0)
    top, at = kernel(seqs, mats, [0, 1], [3, 4], offsets=np.zeros(3, dtype=np.int64), best=True)
    assert (P.bits(top) == P.NAN_BITS).all() and (at == -1).all()


# ------------------------------------------------------------ the seeded cases of tests/pwm_cases.py, sized down --
class OnHost:
    """the program as a device of pwm_cases.check_batch"""

    def __init__(self, kernel):
        self.kernel = kernel

    def scores(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True):
        return self.kernel(seqs, mats, track_of, starts, width=width, offsets=None if lengths is None else offsets_of(lengths), do_mask=do_mask)

    def best(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True, grid=0, slack=0):
        offsets = offsets_of(lengths)
        return self.kernel(seqs, mats, track_of, starts, offsets=offsets, do_mask=do_mask, best=True, grid=grid, total=int(offsets[-1]) + slack)


@pytest.mark.parametrize("name", sorted(PC.MATRIX_SETS))
def test_seeded_matrix_sets(kernel, name):
    """random matrices of mixed magnitudes, so that the order of the additions shows: exactly PW_LDS_VALUES values and the smallest
    set beyond them, 16 columns with column 15 in use, PW_MATS_MAX matrices of 1 .. 256 rows; a few dozen ragged rows, and windows"""
    rows, longest = (10, 400) if name == "mats_max" else (30, 1500)  # (the program's time goes with tiles x matrices)
    PC.check_batch([OnHost(kernel)], PC.matrix_set_case(name, rows, 20_000, longest), where=name)


def test_extremes_and_arithmetic_nans(kernel):
    """negative, denormal, +inf and -inf best scores; windows that sum to inf - inf or meet a NaN entry are NaN in the planes and
    never the best hit"""
    PC.check_batch([OnHost(kernel)], PC.extremes_case(60, 20_000, 2000), where="extremes")


def test_best_hit_on_sampled_lanes(kernel):
    """rows of one tile whose greatest score lies at offset i, for the i of pwm_cases.LANE_SAMPLE: every element of a thread, the
    first and last lane of every wave; under the second matrix offsets i and i + k tie, the first wins"""
    case = PC.lane_case(PC.LANE_SAMPLE)
    PC.check_batch([OnHost(kernel)], case, do_masks=(True,), planes=False, where="lanes")
    got = OnHost(kernel).best(case["seqs"], case["mats"], case["track_of"], case["starts"], case["lengths"])
    assert np.array_equal(got[1][0], case["which"]) and np.array_equal(got[1][1], case["which"]) and (got[0] == 1).all()


@pytest.mark.parametrize("rows", ("long", "many"))
def test_best_walks_more_tiles_than_the_grid(kernel, rows):
    """five tiles and a bit in a grid of two workgroups, so each takes two or three: one long row in which every offset ties or
    the greatest score lies in the far end and its equal in the near end, and the same total in many rows; a total that is only
    a bound several grid fills beyond the rows"""
    case = PC.long_row_case(5) if rows == "long" else PC.many_rows_case(5)
    PC.check_batch([OnHost(kernel)], case, planes=False, where=rows, best_args=(dict(grid=2), dict(grid=2, slack=7 * P.TILE + 5)))


def test_rows_at_the_phases_of_the_top_of_int32(kernel):
    """pwm_cases.top_rows on a sequence of 2^15 - 1 bases: the size, the blocks' edges and so every staged word and column have
    the phases they have at 2^31 - 1; matrices of 20 and 256 rows in 16 columns, the halo reaching past the size"""
    PC.check_batch([OnHost(kernel)], PC.small_top_case(), where="small top")
