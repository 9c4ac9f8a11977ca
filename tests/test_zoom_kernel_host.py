"""CPU-only: the text of zm_summary_kernel (bx-python_amd/csrc/zoom_summary.hpp) compiled for the host by
tests/cpp/zoom_kernel_host.cpp -- 64 threads per workgroup, a barrier for __syncthreads, address and undefined-behaviour sanitizers
on -- gives every recorded reference result, the model's answer on the seeded batches of the GPU tests (several tracks and levels,
an empty one, rows without a track, a region ending at 2^31 - 1) and on runs around the chunk size.  This is the kernel's logic and
indexing, not the GPU's arithmetic: tests/test_gpu_zoom.py checks the same cases on the device."""
import os
import subprocess

import numpy as np
import pytest

import zoom_model as M
from zoom_cases import CHUNK, FILES, SIZES, assert_planes, chunk_level, differential_case, levels, recorded, zoom_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    work = tmp_path_factory.mktemp("zoom_kernel_host")
    exe = str(work / "zoom_kernel_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "bx-python_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "zoom_kernel_host.cpp"), "-o", exe])

    def run(tracks, track_of, starts, ends, size):
        src, dst = str(work / "in.bin"), str(work / "out.bin")
        with open(src, "wb") as f:
            np.array([len(tracks), len(starts), size], dtype=np.int32).tofile(f)
            for z in tracks:
                np.array([len(z.start), len(z.leaf_lo)], dtype=np.int32).tofile(f)
                for a, dtype in zip(z, (np.int32, np.int32, np.uint32) + (np.float32,) * 4 + (np.int32, np.int32, np.int64)):
                    np.ascontiguousarray(a, dtype=dtype).tofile(f)
            for a in (track_of, starts, ends):
                np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().endswith("zoom kernel host ok"), (out.stdout[-500:], out.stderr[-3000:])
        return np.fromfile(dst, dtype=np.float64).reshape(5, len(starts), size)

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


def test_runs_around_the_chunk_size(kernel):
    track = chunk_level()
    runs = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 7, 4 * CHUNK + 63]
    starts = np.array([3 * 7 + 1] * len(runs), dtype=np.int32)
    ends = (3 * 7 + 3 * np.array(runs)).astype(np.int32)
    zeros = np.zeros(len(runs), dtype=np.int32)
    for size in (1, 2, 3):
        assert_planes(kernel([track], zeros, starts, ends, size), M.summarize([track], zeros, starts, ends, size), size)
