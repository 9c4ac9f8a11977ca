#!/usr/bin/env python
"""
bigBed coverage summaries at scale, timed on the device: one sorted bed track of ITEMS records (default 4 M: starts every 25 bases
on average; four lengths in five 20-200 bases, one in five 200-3000, so that the ends descend all the time; record 0 spans the
whole chromosome) and N sites (default 100 k) of WIDTH bases (default 5000) cut into BINS bins (default 100), from device arrays
through bxmi_beds_summarize_dev, HIP-event timed: 2 warm-up runs, then REPS (default 15) repetitions, median and range.  Prints one
JSON line with three figures:

  beds      the new path (csrc/bed_summary.hpp);
  spans     the only way before it, in the same run on the same records: a SpanTrack with every value 1 through
            bxmi_spans_summarize_dev.  Its ends descend, so it is not `ordered` and every site walks the whole track: SPAN_N sites
            (default 2048, enough to fill the device) are timed, 1 warm-up run and SPAN_REPS (default 3) repetitions, and the time is
            scaled linearly to N sites (`scaled_ms`);
  ordered   a reference point: a track of touching, non-overlapping items with the same number of items per site, on the ordered
            bigWig path of bxmi_spans_summarize_dev, all N sites.

    python tools/bench_bigbed_summary.py
    ITEMS=1000000 N=20000 python tools/bench_bigbed_summary.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_bigbed_summary.py --once     # one call: the kernel's own time

`algorithmic_bytes` is what the new path has to move: 12 bytes (start, end, chunk reach) per record that meets a group of 64 bins,
counted per site and group from the track on the host, plus 40 bytes per bin written (five float64 planes); `fraction_of_hbm_peak`
is those bytes over the median time over 8 TB/s -- a whole-call figure: how far the pass is from its memory floor, not what the
memory system did.  `chunk_tests_per_site` is what the chromosome-long record costs: it is every site's first record, so a site
tests every chunk of records from the head of the track to its own (one load each) and stages only those that reach it.
MODEL_ROWS (default 200) of the sites are also computed by tests/summary_model.py over the records as items of value 1 and compared
byte for byte; if they differ the tool exits with an error after printing its line.
"""
import json
import os
import re
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
ITEMS = int(os.environ.get("ITEMS", 4_000_000))
N = int(os.environ.get("N", 100_000))
WIDTH = int(os.environ.get("WIDTH", 5000))
BINS = int(os.environ.get("BINS", 100))
SPAN_N = 0 if ONCE else int(os.environ.get("SPAN_N", 2048))
SPAN_REPS = int(os.environ.get("SPAN_REPS", 3))
MODEL_ROWS = 0 if ONCE else int(os.environ.get("MODEL_ROWS", 200))
HBM_PEAK = 8.0e12  # bytes per second
with open(os.path.join(ROOT, "bx-python_amd", "csrc", "bed_summary.hpp")) as _f:
    CHUNK = int(re.search(r"constexpr int BD_CHUNK = (\d+);", _f.read()).group(1))


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
    extent = 25 * ITEMS
    if extent + 3000 > 2 ** 31 - 1:
        sys.exit("ITEMS = %d reaches beyond 2^31 - 1 bases" % ITEMS)
    rec_starts = np.sort(rng.integers(0, extent, size=ITEMS))
    lengths = np.where(rng.random(ITEMS) < 0.2, rng.integers(200, 3001, size=ITEMS), rng.integers(20, 201, size=ITEMS))
    rec_ends = rec_starts + lengths
    rec_starts[0], rec_ends[0] = 0, extent + 3000  # the chromosome-long record at the head of the file
    rec_starts, rec_ends = rec_starts.astype(np.int32), rec_ends.astype(np.int32)
    descents = int(np.count_nonzero(np.diff(rec_ends.astype(np.int64)) < 0))
    beds = summary.BedTrack(rec_starts, rec_ends)
    assert beds.sorted
    starts_h = rng.integers(0, extent - WIDTH, N).astype(np.int32)
    ends_h = (starts_h + WIDTH).astype(np.int32)
    track_of_h = np.zeros(N, dtype=np.int32)
    starts, ends, track_of = (torch.from_numpy(a).cuda() for a in (starts_h, ends_h, track_of_h))
    # records that meet each group of 64 bins: start < the group's end and end > its first base
    step = WIDTH // BINS
    sorted_ends = np.sort(rec_ends)
    met = 0
    for g0 in range(0, BINS, 64):
        g1 = min(g0 + 64, BINS)
        met += int((np.searchsorted(rec_starts, starts_h.astype(np.int64) + step * g1, side="left")
                    - np.searchsorted(sorted_ends, starts_h.astype(np.int64) + step * g0, side="right")).sum())
    per_site = int((np.searchsorted(rec_starts, ends_h, side="left") - np.searchsorted(sorted_ends, starts_h, side="right")).sum()) / N
    algorithmic = 12 * met + 40 * N * BINS
    res = {}

    def call():
        res["r"] = summary.summarize_beds_dev([beds], track_of, starts, ends, BINS)

    r = timed(call, REPS, WARM)
    sec = r["median_ms"] * 1e-3
    out = {"records": ITEMS, "track_bases": extent, "end_descents": descents, "sites": N, "width": WIDTH, "bins": BINS, "records_per_site": round(per_site, 1),
           "chunk_tests_per_site": round(float(np.searchsorted(rec_starts, ends_h, side="left").mean()) / CHUNK * ((BINS + 63) // 64), 1),
           "algorithmic_bytes": algorithmic, "sites_per_s": round(N / sec), "GBps_algorithmic": round(algorithmic / sec / 1e9, 2),
           "fraction_of_hbm_peak": round(algorithmic / sec / HBM_PEAK, 5), "beds": r}
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        host_track = (rec_starts, rec_ends, np.ones(ITEMS, dtype=np.float32))
        want = summary_model.summarize([host_track], track_of_h[:rows], starts_h[:rows], ends_h[:rows], BINS)
        out["model_rows"] = rows
        out["equals_model"] = bool(all(summary_model.same_bits(g[:rows].cpu().numpy(), w) for g, w in zip(res["r"], want)))
    if SPAN_N > 0:
        m = min(SPAN_N, N)
        spans = summary.SpanTrack(rec_starts, rec_ends, np.ones(ITEMS, dtype=np.float32))
        assert not spans.ordered

        def general():
            res["g"] = summary.summarize_dev([spans], track_of[:m], starts[:m], ends[:m], BINS)

        g = timed(general, SPAN_REPS, 1)
        g.update(sites=m, scaled_ms=round(g["median_ms"] * N / m, 1))
        out["spans"] = g
        out["spans_equal_beds"] = bool(all(torch.equal(a[:m], b) for a, b in zip(res["r"], res["g"])))
        out["speedup_over_spans"] = round(g["scaled_ms"] / r["median_ms"], 1)
        spans.close()
        # the reference point: touching items, as many per site, on the ordered path
        length = max(int(round(WIDTH / max(per_site, 1.0))), 1)
        count = extent // length
        o_starts = (np.arange(count, dtype=np.int64) * length).astype(np.int32)
        ordered = summary.SpanTrack(o_starts, o_starts + np.int32(length), np.ones(count, dtype=np.float32))
        assert ordered.ordered

        def fast():
            res["o"] = summary.summarize_dev([ordered], track_of, starts, ends, BINS)

        o = timed(fast, REPS, WARM)
        o.update(items_per_site=round(WIDTH / length, 1))
        out["ordered"] = o
        ordered.close()
    print(json.dumps(out))
    beds.close()
    if not out.get("equals_model", True):
        sys.exit("the device's rows differ from the model's: the time above measures a wrong result")


if __name__ == "__main__":
    main()
