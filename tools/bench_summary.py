#!/usr/bin/env python
"""
Binned summaries at scale, timed on the device: one span track of ITEMS bedGraph items (default 20 M: items of 1-50 bases, touching
or a little apart, about half a billion bases -- a whole-genome signal track) and N sites (default 100 k) of WIDTH bases (default
5000) cut into BINS bins (default 100), from device arrays through bxmi_spans_summarize_dev, HIP-event timed: warm-up, then REPS
(default 15) repetitions, median and spread.  Prints one JSON line.

    python tools/bench_summary.py
    ITEMS=2000000 N=20000 python tools/bench_summary.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_summary.py --once     # one call: the kernel's own time

`algorithmic_bytes` is what the pass has to move: 12 bytes per item of every site's run (start, end, value; counted per site, from
the track on the host) plus 40 bytes per bin written (five float64 planes); `fraction_of_hbm_peak` is those bytes over the median
time over 8 TB/s.  Neighbouring sites share items only by chance, but the items of one site are read once per group of 64 bins,
mostly from cache, so the figure says how far the pass is from its memory floor, not what the memory system did.
MODEL_ROWS (default 200) of the sites are also computed by tests/summary_model.py and compared byte for byte; if they differ the
tool exits with an error after printing its line.

`bxmi.summary.stats` on device tensors relies on torch's float64 division and square root being the IEEE ones there.  Probed on an
MI355X: torch.sqrt and `/` of 4 M random float64 values on the device against numpy's on the host, no difference in either (the
same probe of torch on the CPU: 52 323 of the 4 M roots are one ulp off).

The figure to hold against it is the reference's own loop -- BigWigFile.summarize_from_full once per site -- timed on a CPU by
`tools/record_summary_golden.py --time-reference` (DESIGN.md 3.9 quotes both with where they were measured).
"""
import json
import os
import sys

import torch  # noqa: F401  (first, like the other device-side tools: its allocator owns the arrays)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bx-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import summary_model  # noqa: E402
from bxmi import summary  # noqa: E402

ONCE = "--once" in sys.argv
REPS = 1 if ONCE else int(os.environ.get("REPS", 15))
WARM = 0 if ONCE else 2
ITEMS = int(os.environ.get("ITEMS", 20_000_000))
N = int(os.environ.get("N", 100_000))
WIDTH = int(os.environ.get("WIDTH", 5000))
BINS = int(os.environ.get("BINS", 100))
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


def main():
    rng = np.random.default_rng(9)
    lengths = rng.integers(1, 51, size=ITEMS)
    gaps = np.where(rng.random(ITEMS) < 0.2, rng.integers(0, 100, size=ITEMS), 0)
    item_starts = np.cumsum(lengths + gaps) - lengths
    if int(item_starts[-1] + lengths[-1]) > 2 ** 31 - 1:
        sys.exit("ITEMS = %d reaches beyond 2^31 - 1 bases" % ITEMS)
    item_starts, item_ends = item_starts.astype(np.int32), (item_starts + lengths).astype(np.int32)
    values = (rng.integers(0, 100001, size=ITEMS) / 1000.0).astype(np.float32)
    host_track = (item_starts, item_ends, values)
    track = summary.SpanTrack(*host_track)
    assert track.ordered
    reach = int(item_ends[-1])
    starts_h = rng.integers(0, max(reach - WIDTH, 1), N).astype(np.int32)
    ends_h = (starts_h + WIDTH).astype(np.int32)
    track_of_h = np.zeros(N, dtype=np.int32)
    starts, ends, track_of = (torch.from_numpy(a).cuda() for a in (starts_h, ends_h, track_of_h))
    run_items = int((np.searchsorted(item_starts, ends_h, side="left") - np.searchsorted(item_ends, starts_h, side="right")).sum())
    algorithmic = 12 * run_items + 40 * N * BINS
    res = {}

    def call():
        res["r"] = summary.summarize_dev([track], track_of, starts, ends, BINS)

    r = timed(call, REPS, WARM)
    sec = r["median_ms"] * 1e-3
    out = {"items": ITEMS, "track_bases": reach, "sites": N, "width": WIDTH, "bins": BINS, "items_per_site": round(run_items / N, 1),
           "algorithmic_bytes": algorithmic, "sites_per_s": round(N / sec), "GBps_algorithmic": round(algorithmic / sec / 1e9, 2),
           "fraction_of_hbm_peak": round(algorithmic / sec / HBM_PEAK, 5)}
    out.update(r)
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        want = summary_model.summarize([host_track], track_of_h[:rows], starts_h[:rows], ends_h[:rows], BINS)
        out["model_rows"] = rows
        out["equals_model"] = bool(all(summary_model.same_bits(g[:rows].cpu().numpy(), w) for g, w in zip(res["r"], want)))
    print(json.dumps(out))
    track.close()
    if not out.get("equals_model", True):
        sys.exit("the device's rows differ from the model's: the time above measures a wrong result")


if __name__ == "__main__":
    main()
