#!/usr/bin/env python
"""
Building a 2bit track from letters, timed on the device, every route in the same run: the synthetic sequence of tools/bench_twobit.py
(SIZE bases, default 250 M; 42 N blocks, about 416 k mask blocks over half of it) is put on the device from its arrays, its letters
are read into HBM (sequences_dev) and from there:

  from_letters_dev      TwoBitTrack.from_letters_dev on the tensor: HIP events around the call (which holds two stream
                        synchronisations of its own), REPS (default 15) repetitions after 2 warm-ups, median and range.
                        `input_GBps` is SIZE bytes over the median, `fraction_of_hbm_peak` that over 8 TB/s: the first pass reads a
                        byte per base and writes a quarter, the second reads the letters of the tiles that hold a block boundary
                        again -- a whole-call figure, allocations and the creation tail (checkpoints, counts under N) included.
  before                the route there was before: the tensor to the host, tests/build_model.py's numpy model, bxmi_twobit_create.
                        Wall clock, BEFORE_REPS (default 3) repetitions: it is host work of seconds.
  from_letters          the letters from host memory (the upload of the whole input included), wall clock, REPS repetitions.
  from_nib              the same sequence as nibbles from host memory, wall clock, REPS repetitions.
  matrix_rows           from_letters_dev on the N x WIDTH (default 100 k x 1000) tensor straight from matrix_dev, HIP events.

Anything slower than `before` is marked "SLOWER".  The arrays of the built track are compared with the synthetic arrays (blocks)
and the model's packed bytes; if they differ the tool exits with an error after printing its line.

The kernels' own times come from a trace, in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_twobit_build.py --once
runs from_letters_dev once on each of the two inputs: bl_build_kernel<0, false> (pack and count), bl_build_kernel<0, true> (place),
bl_sizes_kernel, the scans and the creation tail appear twice each in time order.

    python tools/bench_twobit_build.py
    SIZE=20000000 N=20000 python tools/bench_twobit_build.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_twobit as BT  # noqa: E402  (puts bx-python_amd and tests on the path)

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else int(os.environ.get("REPS", 15))
WARM = 0 if ONCE else 2
BEFORE_REPS = int(os.environ.get("BEFORE_REPS", 3))
HBM_PEAK = 8.0e12


def spread(values, unit):
    v = np.array(values)
    return {"median_" + unit: round(float(np.median(v)), 4), "min_" + unit: round(float(v.min()), 4), "max_" + unit: round(float(v.max()), 4), "reps": len(values)}


def main():
    import torch

    import build_model as B
    from bxmi import sequence

    def events(fn):
        for _ in range(WARM):
            fn().close()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            track = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            track.close()
        return spread(ms, "ms")

    def wall(fn, reps):
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            track = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
            track.close()
        return spread(ms, "ms")

    seq = BT.synthetic()
    size = BT.SIZE
    source = sequence.TwoBitTrack.from_arrays(seq[0], size, *seq[1:])
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    letters, _ = sequence.sequences_dev([source], zero, zero, torch.full((1,), size, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert letters.numel() == size

    def rate(entry, bases):
        entry.update(bases=bases, input_GBps=round(bases / (entry["median_ms"] * 1e-3) / 1e9, 1),
                     fraction_of_hbm_peak=round(bases / (entry["median_ms"] * 1e-3) / HBM_PEAK, 4))
        return entry

    result = {"size": size, "n_blocks": len(seq[1]), "mask_blocks": len(seq[3])}
    result["from_letters_dev"] = rate(events(lambda: sequence.TwoBitTrack.from_letters_dev(letters)), size)

    # the N x WIDTH matrix straight from matrix_dev
    short_h, _ = BT.sites()
    rows = sequence.matrix_dev([source], torch.zeros(BT.N, dtype=torch.int32, device="cuda"), torch.from_numpy(short_h).cuda(), BT.WIDTH)
    torch.cuda.synchronize()
    result["matrix_rows"] = rate(events(lambda: sequence.TwoBitTrack.from_letters_dev(rows)), rows.numel())
    result["matrix_rows"].update(rows=BT.N, width=BT.WIDTH)
    if ONCE:
        print(json.dumps(result))
        return

    built = {}

    def before():
        host = letters.cpu().numpy()
        built["model"] = B.from_letters(host)
        return sequence.TwoBitTrack(built["model"].seq)

    result["before"] = wall(before, BEFORE_REPS)
    host_letters = letters.cpu().numpy()
    result["from_letters"] = wall(lambda: sequence.TwoBitTrack.from_letters(host_letters), REPS)
    nibbles = B.to_nib(host_letters)
    result["from_nib"] = wall(lambda: sequence.TwoBitTrack.from_nib(nibbles, size), REPS)
    base = result["before"]["median_ms"]
    for key in ("from_letters_dev", "from_letters", "from_nib"):
        result[key]["over_before"] = round(result[key]["median_ms"] / base, 4)
        if result[key]["median_ms"] > base:
            result[key]["verdict"] = "SLOWER"

    track = sequence.TwoBitTrack.from_letters_dev(letters)
    got, model = track.arrays(), built["model"].seq
    same = (B.same_arrays(got, model) and np.array_equal(got.n_starts, seq[1]) and np.array_equal(got.n_sizes, seq[2])
            and np.array_equal(got.m_starts, seq[3]) and np.array_equal(got.m_sizes, seq[4]))
    track.close()
    result["equals_model"] = bool(same)
    print(json.dumps(result))
    source.close()
    if not same:
        sys.exit("the built track's arrays differ from the model's: the times above measure a wrong result")


if __name__ == "__main__":
    main()
