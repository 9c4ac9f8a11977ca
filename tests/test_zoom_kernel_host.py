"""CPU-only: the text of zm_summary_kernel (bx-python_amd/csrc/zoom_summary.hpp) compiled for the host by
tests/cpp/zoom_kernel_host.cpp -- 64 threads per workgroup, a barrier for __syncthreads, address and undefined-behaviour sanitizers
on -- gives every recorded reference result, the model's answer on the seeded batches of the GPU tests (several tracks and levels,
an empty one, rows without a track, a region ending at 2^31 - 1), under records and leaves that end at 2^31 - 1 and on runs around
the chunk size.  This is the kernel's logic and
indexing, not the GPU's arithmetic: tests/test_gpu_zoom.py checks the same cases on the device."""
import numpy as np
import pytest

import kernel_host
import zoom_model as M
from zoom_cases import CHUNK, FILES, SIZES, TOP_SIZES, assert_planes, chunk_level, differential_case, levels, recorded, top_case, zoom_cases


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    program = kernel_host.build(tmp_path_factory, "zoom_kernel_host", "zoom kernel host ok")

    def run(tracks, track_of, starts, ends, size):
        def write_in(f):
            np.array([len(tracks), len(starts), size], dtype=np.int32).tofile(f)
            for z in tracks:
                np.array([len(z.start), len(z.leaf_lo)], dtype=np.int32).tofile(f)
                kernel_host.write_arrays(f, *zip(z, (np.int32, np.int32, np.uint32) + (np.float32,) * 4 + (np.int32, np.int32, np.int64)))
            kernel_host.write_arrays(f, (track_of, np.int32), (starts, np.int32), (ends, np.int32))

        return np.fromfile(program(write_in), dtype=np.float64).reshape(5, len(starts), size)

    return run


@pytest.mark.parametrize("name", sorted(FILES))
def test_recorded_cases(kernel, name):
    """all zoom regions of one file that share a size in ONE call: the table lists every (chromosome, level) part"""
    per_level = levels(name)
    order = list(per_level[0][1])
    tracks = [per[chrom] for chrom in order for _, per in per_level]
    cases = FILES[name]["cases"]
    for size in sorted({cases[k]["size"] for k in zoom_cases(name)}):
        ks = [k for k in zoom_cases(name) if cases[k]["size"] == size]
        rows = [cases[k] for k in ks]
        track_of = [order.index(c["chrom"]) * len(per_level) + c["level"] for c in rows]
        got = kernel(tracks, track_of, [c["start"] for c in rows], [c["end"] for c in rows], size)
        assert_planes(got, np.stack([recorded(name, k)[1] for k in ks], axis=1), (name, size))


@pytest.mark.parametrize("size", SIZES)
def test_seeded_batches(kernel, size):
    tracks, track_of, starts, ends, want = differential_case(size)
    assert_planes(kernel(tracks, track_of, starts, ends, size), want, size)


@pytest.mark.parametrize("size", TOP_SIZES)
def test_records_that_end_at_the_top_of_int32(kernel, size):
    tracks, track_of, starts, ends, want = top_case(size)
    assert_planes(kernel(tracks, track_of, starts, ends, size), want, size)


def test_runs_around_the_chunk_size(kernel):
    track = chunk_level()
    runs = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7, 4 * CHUNK + 63]
    starts = np.array([3 * 7 + 1] * len(runs), dtype=np.int32)
    ends = (3 * 7 + 3 * np.array(runs)).astype(np.int32)
    zeros = np.zeros(len(runs), dtype=np.int32)
    for size in (1, 2, 3):
        assert_planes(kernel([track], zeros, starts, ends, size), M.summarize([track], zeros, starts, ends, size), size)
