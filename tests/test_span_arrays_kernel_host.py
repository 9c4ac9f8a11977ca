"""CPU-only: the text of sa_arrays_kernel (bx-python_amd/csrc/span_arrays.hpp) compiled for the host by
tests/cpp/span_arrays_kernel_host.cpp -- a workgroup of host threads, a barrier for __syncthreads, address and undefined-behaviour
sanitizers on, the output between two guard bands -- gives every recorded reference array and the model's answer on the edge shapes
of the GPU tests: ragged batches whose rows start anywhere in a thread's 4 elements, empty rows, widths around a tile, runs around
the chunk size, ordered tracks with overlapping items, tracks that are not ordered, rows without a track, windows from below 0 and
at the end of int32, items that end at 2^31 - 1 under rows that end there or run past it, an output off a 16-byte boundary, and the output cut into slabs as the host form cuts it.  This is the
kernel's logic and indexing; tests/test_gpu_arrays.py checks the same cases on the device."""
import numpy as np
import pytest

import kernel_host
import arrays_model as M
from test_arrays_model_golden import ALL_FILES, all_recorded, spans

GUARD = 64


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    program = kernel_host.build(tmp_path_factory, "span_arrays_kernel_host", "span arrays kernel host ok")

    def run(tracks, track_of, starts, width=0, offsets=None, misalign=0, slab_tiles=0):
        """-> float32[total]; the guard bands are checked here"""
        n = len(track_of)
        total = int(offsets[-1]) if offsets is not None else n * width

        def write_in(f):
            np.array([len(tracks), n, width, offsets is not None, misalign, slab_tiles], dtype=np.int32).tofile(f)
            np.array([total], dtype=np.int64).tofile(f)
            for s, e, v in tracks:
                kernel_host.write_arrays(f, ([len(s), M.is_ordered((s, e, v))], np.int32), (s, np.int32), (e, np.int32), (v, np.float32))
            kernel_host.write_arrays(f, (track_of, np.int32), (starts, np.int32))
            if offsets is not None:
                kernel_host.write_arrays(f, (offsets, np.int64))

        words = np.fromfile(program(write_in), dtype=np.uint32)
        assert len(words) == total + 2 * GUARD
        assert (words[:GUARD] == 0xDEADBEEF).all() and (words[GUARD + total:] == 0xDEADBEEF).all(), "written outside the output"
        return words[GUARD:GUARD + total].view(np.float32)

    return run


@pytest.mark.parametrize("name", ALL_FILES)
def test_recorded_cases(kernel, name):
    """all regions of a file as ONE ragged batch, the reference's None as an empty row"""
    tracks = spans(name)
    order = list(tracks)
    cases = all_recorded(name)
    track_of = [order.index(c) if c in order else -1 for (c, _, _), _ in cases]
    starts = [s for (_, s, _), _ in cases]
    lengths = [0 if a is None else len(a) for _, a in cases]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    want = np.concatenate([a for _, a in cases if a is not None])
    M.assert_same(kernel([tracks[c] for c in order], track_of, starts, offsets=offsets), want, name)


def test_ragged_edges(kernel):
    tracks, track_of, starts, ends, (want, offsets) = M.ragged_case()
    M.assert_same(kernel(tracks, track_of, starts, offsets=offsets), want, "ragged")
    M.assert_same(kernel(tracks, track_of, starts, offsets=offsets, misalign=1), want, "ragged, out 4 bytes past a 16-byte boundary")
    M.assert_same(kernel(tracks, track_of, starts, offsets=offsets, slab_tiles=3), want, "ragged, in slabs of 3 tiles")


@pytest.mark.parametrize("width", M.MATRIX_WIDTHS)
def test_matrix_widths(kernel, width):
    tracks, track_of, starts, want = M.matrix_case(width)
    M.assert_same(kernel(tracks, track_of, starts, width=width).reshape(-1, width), want, width)
    if width in (3, M.TILE + 1):
        M.assert_same(kernel(tracks, track_of, starts, width=width, slab_tiles=2, misalign=3).reshape(-1, width), want, (width, "slabs of 2 tiles"))


def test_items_that_end_at_the_top_of_int32(kernel):
    tracks, track_of, starts, _, (want, offsets), _ = M.top_ragged_case()
    M.assert_same(kernel(tracks, track_of, starts, offsets=offsets), want, "ragged")
    M.assert_same(kernel(tracks, track_of, starts, offsets=offsets, misalign=1, slab_tiles=2), want, "ragged, in slabs of 2 tiles, out off a 16-byte boundary")
    for width in M.TOP_WIDTHS:
        tracks, track_of, starts, want = M.top_matrix_case(width)
        M.assert_same(kernel(tracks, track_of, starts, width=width).reshape(-1, width), want, width)


def test_nothing_to_do(kernel):
    tracks = M.tracks()
    assert len(kernel(tracks, [], [], width=5)) == 0
    assert len(kernel(tracks, [0, 1], [3, 4], offsets=np.zeros(3, dtype=np.int64))) == 0
