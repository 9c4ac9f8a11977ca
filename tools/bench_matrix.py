#!/usr/bin/env python
"""
Per-base signal matrices at scale, timed on the device: N sites (default 100 k) of WIDTH bases (default 1000) -- the site x base
matrix of a whole BED file, 400 MB of float32 -- from device arrays through bxmi_spans_arrays_dev into a matrix allocated once,
HIP-event timed: warm-up, then REPS (default 15) repetitions, median and spread.  Two tracks, one JSON line each:

    A  `unit`      ITEMS (default 20 M) items of one base each, touching: a fixedStep span=1 signal; a site meets WIDTH items
    B  `bedgraph`  ITEMS items of 1-50 bases (about 25), touching or a little apart: a bedGraph; a site meets about WIDTH / 25

    python tools/bench_matrix.py
    ITEMS=2000000 N=20000 python tools/bench_matrix.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_matrix.py --once     # one call per track: the kernel's own time

`output_bytes` is 4 bytes per base written, the floor of the pass; `fraction_of_hbm_peak` is those bytes over the median time
over 8 TB/s (a float4 copy reaches about 0.79 of that peak on this part, so about 0.4 is half of the achievable write rate).
The items a site reads (12 bytes each, `items_per_site`) come on top and are not counted.  MODEL_ROWS (default 200) of the rows
are also computed by tests/arrays_model.py and compared byte for byte; if they differ the tool exits with an error after
printing its line.

The figure to hold against it is the reference's own loop -- BigWigFile.get_as_array once per site, as
scripts/bed_bigwig_profile.py makes it -- timed on a CPU by `tools/record_arrays_golden.py --time-reference` (DESIGN.md 3.12
quotes both with where they were measured).
"""
import json
import os
import sys

import torch  # noqa: F401  (first, like the other device-side tools: its allocator owns the arrays)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bx-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import arrays_model  # noqa: E402
from bxmi import summary  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else int(os.environ.get("REPS", 15))
WARM = 0 if ONCE else 2
ITEMS = int(os.environ.get("ITEMS", 20_000_000))
N = int(os.environ.get("N", 100_000))
WIDTH = int(os.environ.get("WIDTH", 1000))
MODEL_ROWS = 0 if ONCE else int(os.environ.get("MODEL_ROWS", 200))
HBM_PEAK = 8.0e12  # bytes per second


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


def make_track(kind, rng):
    if kind == "unit":
        item_starts = np.arange(ITEMS, dtype=np.int64) + 1000
        lengths = np.ones(ITEMS, dtype=np.int64)
    else:
        lengths = rng.integers(1, 51, size=ITEMS)
        gaps = np.where(rng.random(ITEMS) < 0.2, rng.integers(0, 100, size=ITEMS), 0)
        item_starts = np.cumsum(lengths + gaps) - lengths
    if int(item_starts[-1] + lengths[-1]) > 2 ** 31 - 1:
        sys.exit("ITEMS = %d reaches beyond 2^31 - 1 bases" % ITEMS)
    values = (rng.integers(0, 100001, size=ITEMS) / 1000.0).astype(np.float32)
    return item_starts.astype(np.int32), (item_starts + lengths).astype(np.int32), values


def bench(kind, rng):
    host_track = make_track(kind, rng)
    item_starts, item_ends, _ = host_track
    track = summary.SpanTrack(*host_track)
    assert track.ordered
    reach = int(item_ends[-1])
    starts_h = rng.integers(0, max(reach - WIDTH, 1), N).astype(np.int32)
    track_of_h = np.zeros(N, dtype=np.int32)
    starts, track_of = (torch.from_numpy(a).cuda() for a in (starts_h, track_of_h))
    run_items = int((np.searchsorted(item_starts, starts_h.astype(np.int64) + WIDTH, side="left") - np.searchsorted(item_ends, starts_h, side="right")).sum())
    out_matrix = torch.empty((N, WIDTH), dtype=torch.float32, device="cuda")

    def call():
        summary.matrix_dev([track], track_of, starts, WIDTH, out=out_matrix)

    r = timed(call, REPS, WARM)
    sec = r["median_ms"] * 1e-3
    output_bytes = 4 * N * WIDTH
    out = {"track": kind, "items": ITEMS, "track_bases": reach, "sites": N, "width": WIDTH, "items_per_site": round(run_items / N, 1),
           "output_bytes": output_bytes, "sites_per_s": round(N / sec), "GBps_output": round(output_bytes / sec / 1e9, 2),
           "fraction_of_hbm_peak": round(output_bytes / sec / HBM_PEAK, 5)}
    out.update(r)
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        got = out_matrix[:rows].cpu().numpy()
        same = True
        for i in range(rows):  # (the model walks every item it is given: only the row's own run)
            s = int(starts_h[i])
            lo, hi = np.searchsorted(item_ends, s, side="right"), np.searchsorted(item_starts, s + WIDTH, side="left")
            same = same and arrays_model.same_bytes(got[i], arrays_model.region(tuple(a[lo:hi] for a in host_track), s, s + WIDTH))
        out["model_rows"] = rows
        out["equals_model"] = bool(same)
    print(json.dumps(out))
    track.close()
    del out_matrix
    return out.get("equals_model", True)


def main():
    rng = np.random.default_rng(9)
    ok = [bench(kind, rng) for kind in ("unit", "bedgraph")]
    if not all(ok):
        sys.exit("the device's rows differ from the model's: the time above measures a wrong result")


if __name__ == "__main__":
    main()
