"""CPU-only: the text of sm_summary_kernel (bx-python_amd/csrc/summary.hpp) compiled for the host by tests/cpp/summary_kernel_host.cpp
-- 64 threads per workgroup, a barrier for __syncthreads, address and undefined-behaviour sanitizers on -- gives every recorded
reference result, the model's answer on the seeded batches of the GPU tests (ordered, not ordered and empty tracks, rows without a
track, regions at the end of int32), under items that end at 2^31 - 1 and on runs around the chunk size.  This is the kernel's logic and indexing, not the GPU's
arithmetic: tests/test_gpu_summary.py checks the same cases on the device."""
import numpy as np
import pytest

import kernel_host
import summary_model as M
from summary_cases import CHUNK, TOP_SIZES, assert_planes, chunk_track, differential_case, empty_planes, top_case
from test_summary_model_golden import FILES, recorded, spans


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    program = kernel_host.build(tmp_path_factory, "summary_kernel_host", "summary kernel host ok")

    def run(tracks, track_of, starts, ends, size):
        def write_in(f):
            np.array([len(tracks), len(starts), size], dtype=np.int32).tofile(f)
            for s, e, v in tracks:
                ordered = bool(np.all(np.diff(s) >= 0) and np.all(np.diff(e) >= 0))
                kernel_host.write_arrays(f, ([len(s), ordered], np.int32), (s, np.int32), (e, np.int32), (v, np.float32))
            kernel_host.write_arrays(f, (track_of, np.int32), (starts, np.int32), (ends, np.int32))

        return np.fromfile(program(write_in), dtype=np.float64).reshape(5, len(starts), size)

    return run


@pytest.mark.parametrize("name", sorted(FILES))
def test_recorded_cases(kernel, name):
    tracks = spans(name)
    order = list(tracks)
    cases = FILES[name]["cases"]
    for size in sorted({c["size"] for c in cases}):
        ks = [k for k, c in enumerate(cases) if c["size"] == size]
        rows = [cases[k] for k in ks]
        track_of = [order.index(c["chrom"]) if c["chrom"] in order else -1 for c in rows]
        got = kernel([tracks[c] for c in order], track_of, [c["start"] for c in rows], [c["end"] for c in rows], size)
        want = np.stack([recorded(name, k)[1] if not cases[k]["none"] else empty_planes(size) for k in ks], axis=1)
        assert_planes(got, want, (name, size))


@pytest.mark.parametrize("size", (1, 2, 64, 65, 200))
def test_seeded_batches(kernel, size):
    tracks, track_of, starts, ends, want = differential_case(size)
    assert_planes(kernel(tracks, track_of, starts, ends, size), want, size)


@pytest.mark.parametrize("size", TOP_SIZES)
def test_items_that_end_at_the_top_of_int32(kernel, size):
    tracks, track_of, starts, ends, want = top_case(size)
    assert_planes(kernel(tracks, track_of, starts, ends, size), want, size)


def test_runs_around_the_chunk_size(kernel):
    track = chunk_track()
    runs = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7, 4 * CHUNK + 63]
    starts = np.array([3 * 7 + 1] * len(runs), dtype=np.int32)
    ends = (3 * 7 + 3 * np.array(runs)).astype(np.int32)
    zeros = np.zeros(len(runs), dtype=np.int32)
    for size in (1, 2, 3):
        assert_planes(kernel([track], zeros, starts, ends, size), M.summarize([track], zeros, starts, ends, size), size)
    back = tuple(a[::-1].copy() for a in track)  # not ordered: the general path
    assert_planes(kernel([back], zeros, starts, ends, 3), M.summarize([back], zeros, starts, ends, 3), "reversed track")
