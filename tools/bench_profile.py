#!/usr/bin/env python
"""
Site profiles at scale, timed on the device: one track of SIZE bases (default 250 M) of phastCons-like three-decimal scores (a
fifth of the bases without one) and N windows (default 1 M) of WIDTH bases (default 5000) from device arrays through
bxmi_scores_profile_dev, HIP-event timed: warm-up, then REPS (default 15) repetitions, median and spread.  Two cases:

    auto          scores.profile_chain = 0: such scores are summed in parallel (the case reports how many columns took the chain)
    forced_chain  scores.profile_chain = 1: every column runs the ordered chain -- what exactness costs when it is needed
                  (CHAIN_REPS repetitions, default 3)

and the same rows through the NumPy model (tests/profile_model.py: the reference's loop, a window per Python iteration) on the
same box, MODEL_ROWS of them (default all; its totals are then compared with the device's, byte for byte).  Prints one JSON line.

    python tools/bench_profile.py
    SIZE=50000000 N=200000 WIDTH=2000 python tools/bench_profile.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_profile.py --once     # one call per case: the per-kernel split

`GBps_of_scores` is 4 bytes per window position over the measured time; the windows overlap and mostly hit in cache, so HBM is
not the floor here.
"""
import json
import os
import sys
import time

import torch  # noqa: F401  (first, like the other device-side tools: its allocator owns the arrays)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bx-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import profile_model  # noqa: E402
from bxmi import _ffi, scores  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else int(os.environ.get("REPS", 15))
CHAIN_REPS = 1 if ONCE else int(os.environ.get("CHAIN_REPS", 3))
WARM = 0 if ONCE else 2
SIZE = int(os.environ.get("SIZE", 250_000_000))
N = int(os.environ.get("N", 1_000_000))
WIDTH = int(os.environ.get("WIDTH", 5000))
MODEL_ROWS = 0 if ONCE else int(os.environ.get("MODEL_ROWS", N))


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4), "reps": int(reps)}


def main():
    rng = np.random.default_rng(9)
    track = scores.ScoreTrack(SIZE)
    host = np.empty(SIZE, dtype=np.float32)
    chunk = 1 << 24
    for at in range(0, SIZE, chunk):
        m = min(chunk, SIZE - at)
        v = (rng.integers(0, 1001, size=m) / 1000.0).astype(np.float32)
        v[rng.random(m, dtype=np.float32) < 0.2] = np.nan
        host[at:at + m] = v
        track.write(at, v)
    starts_h = rng.integers(-WIDTH // 2, SIZE - WIDTH // 2, N).astype(np.int32)
    track_of_h = np.zeros(N, dtype=np.int32)
    starts, track_of = torch.from_numpy(starts_h).cuda(), torch.from_numpy(track_of_h).cuda()
    positions = N * WIDTH
    out = {"track_bases": SIZE, "windows": N, "width": WIDTH, "window_positions": positions, "cases": {}}
    results = {}
    try:
        for name, chain, reps in (("auto", 0, REPS), ("forced_chain", 1, CHAIN_REPS)):
            _ffi.call("bxmi_set_option", b"scores.profile_chain", chain)
            res = {}

            def call():
                res["r"] = scores.profile_dev([track], track_of, starts, WIDTH)

            r = timed(call, reps, WARM)
            sec = r["median_ms"] * 1e-3
            r["chain_columns"] = int(res["r"].chain_columns.item())
            r["windows_per_s"] = round(N / sec)
            r["GBps_of_scores"] = round(4.0 * positions / sec / 1e9, 2)
            results[name] = (res["r"].totals.cpu().numpy(), res["r"].valid.cpu().numpy())
            out["cases"][name] = r
    finally:
        _ffi.call("bxmi_set_option", b"scores.profile_chain", 0)
    out["forced_chain_equals_auto"] = bool(results["auto"][0].tobytes() == results["forced_chain"][0].tobytes())
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        t0 = time.perf_counter()
        totals, valid = profile_model.profile([host], track_of_h[:rows], starts_h[:rows], WIDTH)
        sec = time.perf_counter() - t0
        model = {"rows": rows, "seconds": round(sec, 3), "windows_per_s": round(rows / sec)}
        if rows == N:
            model["equals_device"] = bool(totals.tobytes() == results["auto"][0].tobytes() and np.array_equal(valid, results["auto"][1]))
        model["device_auto_speedup"] = round((sec / rows) / (out["cases"]["auto"]["median_ms"] * 1e-3 / N), 1)
        model["device_forced_chain_speedup"] = round((sec / rows) / (out["cases"]["forced_chain"]["median_ms"] * 1e-3 / N), 1)
        out["numpy_model"] = model
    print(json.dumps(out))
    track.close()


if __name__ == "__main__":
    main()
