"""CPU-only: the text of bd_summary_kernel (bx-python_amd/csrc/bed_summary.hpp) compiled for the host by
tests/cpp/bed_summary_kernel_host.cpp -- 64 threads per workgroup, a barrier for __syncthreads, address and undefined-behaviour
sanitizers on -- gives every recorded reference result, the model's answer on the seeded batches of the GPU tests and on the chunk
cases; the program first checks the builder of reach[] and creach[] against a direct computation (n = 0, 1, BD_CHUNK,
BD_CHUNK + 1, ...).  This is the kernel's logic and indexing, not the GPU's arithmetic: tests/test_gpu_bed_summary.py checks
the same cases on the device."""
import os
import subprocess

import numpy as np
import pytest

from bed_cases import FILES, SIZES, assert_planes, by_size, chunk_cases, differential_case, items, recorded_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    work = tmp_path_factory.mktemp("bed_summary_kernel_host")
    exe = str(work / "bed_summary_kernel_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "bx-python_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "bed_summary_kernel_host.cpp"), "-o", exe])

    def run(tracks, track_of, starts, ends, size):
        src, dst = str(work / "in.bin"), str(work / "out.bin")
        with open(src, "wb") as f:
            np.array([len(tracks), len(starts), size], dtype=np.int32).tofile(f)
            for t in tracks:
                np.array([len(t[0])], dtype=np.int32).tofile(f)
                for a in t[:2]:
                    np.ascontiguousarray(a, dtype=np.int32).tofile(f)
            for a in (track_of, starts, ends):
                np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().endswith("bed summary kernel host ok"), (out.returncode, out.stdout[-500:], out.stderr[-3000:])
        cells = 5 * len(starts) * size
        is_sorted = np.fromfile(dst, dtype=np.int32, offset=8 * cells)
        assert [bool(x) for x in is_sorted] == [bool(np.all(np.diff(t[0]) >= 0)) for t in tracks]
        return np.fromfile(dst, dtype=np.float64, count=cells).reshape(5, len(starts), size)

    return run


@pytest.mark.parametrize("name", sorted(FILES))
def test_recorded_cases(kernel, name):
    tracks = [items(name)[c] for c in FILES[name]["chroms"]]
    for size, ks, track_of, starts, ends in by_size(name):
        assert_planes(kernel(tracks, track_of, starts, ends, size), recorded_batch(name, ks, size), (name, size))


@pytest.mark.parametrize("size", SIZES)
def test_seeded_batches(kernel, size):
    tracks, track_of, starts, ends, want = differential_case(size)
    assert_planes(kernel(tracks, track_of, starts, ends, size), want, size)


def test_chunk_cases(kernel):
    for label, tracks, track_of, starts, ends, size, want in chunk_cases():
        assert_planes(kernel(tracks, track_of, starts, ends, size), want, label)
