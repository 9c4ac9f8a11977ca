#!/usr/bin/env python
"""
Browser-scale summaries answered from a zoom level, timed on the device against the same request answered from full data: a
synthetic PER-BASE track of BASES one-base items (default 64 Mi) with zoom levels 4 times apart (4, 16, 64, ... while a level has
at least 64 records; leaves of LEAF records, default 512), and N regions (default 10 000) of WIDTH bases (default 1 Mb) in BINS
bins (default 100).  The reference's rule picks the level with the largest reduction <= WIDTH / BINS / 2 for every one of them.

Timed, alternating, after WARM warm-up calls of each (default 1), REPS times each (default 5), median and spread:
    host forms    bxmi.summary.TrackSet.summarize(zoom=True) and (zoom=False): host arrays in, host arrays out, a host clock around
                  calls that block until the planes are back (they include the copies of N * BINS * 40 bytes to the host);
    device forms  summarize_zoom_dev and summarize_dev on device tensors, HIP events around the call: the kernels and the table.
Prints one JSON line.

`bytes` is what each call has to touch in HBM, computed from the shapes on the host: per region the records (28 bytes each) or
items (12 bytes each) from the first that ends after the region's start to the last that starts before its end, plus 40 bytes
per bin written.  MODEL_ROWS (default 20) of the zoom rows are also computed by tests/zoom_model.py and compared byte for byte;
if they differ the tool exits with an error after printing its line.

    python tools/bench_zoom_summary.py
    BASES=8388608 N=1000 python tools/bench_zoom_summary.py
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

import zoom_model  # noqa: E402
from bxmi import summary  # noqa: E402
from bxmi.bigwig import ZoomArrays  # noqa: E402

REPS = int(os.environ.get("REPS", 5))
WARM = int(os.environ.get("WARM", 1))
BASES = int(os.environ.get("BASES", 64 << 20))
N = int(os.environ.get("N", 10_000))
WIDTH = int(os.environ.get("WIDTH", 1_000_000))
BINS = int(os.environ.get("BINS", 100))
LEAF = int(os.environ.get("LEAF", 512))
MODEL_ROWS = int(os.environ.get("MODEL_ROWS", 20))


def zoom_level(values, reduction):
    """the level of `reduction` bases per record over a per-base track (BASES is a multiple of it)"""
    v = values.astype(np.float64).reshape(-1, reduction)
    n = len(v)
    start = (np.arange(n, dtype=np.int64) * reduction).astype(np.int32)
    first = np.append(np.arange(0, n, LEAF, dtype=np.int64), n)
    return ZoomArrays(start, start + reduction, np.full(n, reduction, dtype=np.uint32), v.min(axis=1).astype(np.float32), v.max(axis=1).astype(np.float32),
                      v.sum(axis=1).astype(np.float32), (v * v).sum(axis=1).astype(np.float32), start[first[:-1]],
                      (start + reduction)[first[1:] - 1], first)


def spread(samples):
    a = np.array(samples)
    return {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a.min()), 3), "max_ms": round(float(a.max()), 3), "reps": len(a)}


def main():
    if BASES % (1 << 20) or BASES > 2 ** 31 - 1:
        sys.exit("BASES must be a multiple of 2^20 below 2^31")
    rng = np.random.default_rng(5)
    values = (rng.integers(0, 100001, size=BASES) / 1000.0).astype(np.float32)
    base = np.arange(BASES, dtype=np.int32)
    spans = {"chrS": (base, base + 1, values)}
    levels, reduction = [], 4
    while BASES // reduction >= 64:
        levels.append((reduction, {"chrS": zoom_level(values, reduction)}))
        reduction *= 4
    ts = summary.TrackSet(spans, levels)
    starts_h = rng.integers(0, BASES - WIDTH, N).astype(np.int32)
    ends_h = (starts_h + WIDTH).astype(np.int32)
    chrom_h = np.zeros(N, dtype=np.int32)
    picked = summary.pick_levels(ts.reductions, starts_h, ends_h, BINS)
    assert picked.min() == picked.max() >= 0, "the shape picks no level, or not one level for all regions"
    level = int(picked[0])
    z = levels[level][1]["chrS"]
    zoom_track = ts.zoom[level]
    records = int((np.searchsorted(z.start, ends_h, side="left") - np.searchsorted(z.end, starts_h, side="right")).sum())
    out = {"bases": BASES, "regions": N, "width": WIDTH, "bins": BINS, "reductions": ts.reductions, "level_picked": level,
           "reduction_picked": ts.reductions[level], "records_per_region": round(records / N, 1), "items_per_region": WIDTH,
           "bytes_zoom": 28 * records + 40 * N * BINS, "bytes_full": 12 * WIDTH * N + 40 * N * BINS}
    dev = [torch.from_numpy(a).cuda() for a in (chrom_h, starts_h, ends_h)]
    keep = {}
    calls = {
        "host_zoom": lambda: keep.__setitem__("zoom", ts.summarize(chrom_h, starts_h, ends_h, BINS, zoom=True)),
        "host_full": lambda: ts.summarize(chrom_h, starts_h, ends_h, BINS, zoom=False),
        "dev_zoom": lambda: summary.summarize_zoom_dev([zoom_track], *dev, BINS),
        "dev_full": lambda: summary.summarize_dev([ts.spans["chrS"]], *dev, BINS),
    }
    samples = {k: [] for k in calls}
    for rep in range(WARM + REPS):
        for name, fn in calls.items():  # alternating: every round takes one sample of each
            torch.cuda.synchronize()
            if name.startswith("host"):
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0) * 1e3
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
            if rep >= WARM:
                samples[name].append(ms)
    for name in calls:
        out[name] = spread(samples[name])
    out["GBps_zoom_dev"] = round(out["bytes_zoom"] / (out["dev_zoom"]["median_ms"] * 1e-3) / 1e9, 2)
    out["GBps_full_dev"] = round(out["bytes_full"] / (out["dev_full"]["median_ms"] * 1e-3) / 1e9, 2)
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        want = zoom_model.summarize([z], chrom_h[:rows], starts_h[:rows], ends_h[:rows], BINS)
        out["model_rows"] = rows
        out["equals_model"] = bool(all(zoom_model.same_bits(g[:rows], w) for g, w in zip(keep["zoom"], want)))
    print(json.dumps(out))
    ts.close()
    if not out.get("equals_model", True):
        sys.exit("the device's rows differ from the model's: the times above measure a wrong result")


if __name__ == "__main__":
    main()
