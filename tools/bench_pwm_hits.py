#!/usr/bin/env python
"""
Thresholded position weight matrix hits over 2bit sites at scale, timed on the device against the route through the score planes:
the workload of tools/bench_pwm.py (SIZE = 250 M bases, N = 100 k sites of WIDTH = 1000 bases, one seeded matrix of MOTIF = 20
positions over ACGT plus its reverse complement).  The thresholds are taken from the scores of SAMPLE (default 2000) sites so
that about 1 element in 1000 (`sparse`) and about 1 in 10 (`dense`) is a hit, and 1 in 100 000 (`rare`: what a scan for a
motif's sites asks for -- most tiles then hold no hit, and the placing pass passes them by).  HIP-event timed, 2 warm-up runs,
then REPS repetitions, median and range, both routes in the same run on the same tensors.  Prints one JSON line; per threshold:

  hits_dev       bxmi.motif.hits_dev with max_hits given: two scoring passes, no plane written; the window holds torch's clipping
                 of the rows and the call's wait for the counts;
  planes_route   what there was before: bxmi.motif.score_matrix_dev into a preallocated 2 x N x WIDTH tensor (800 MB), then
                 torch's `>=`, `nonzero` and the gather of the scores;
  same_hits      whether the two routes list the same (matrix, row, offset, score bits) in the same order.

`whole_sequence` times hits_dev on ONE row of all SIZE bases at the rare and the sparse threshold; the planes route would need
2 * SIZE * 4 bytes for it and is not run.

    python tools/bench_pwm_hits.py
    SIZE=20000000 N=20000 python tools/bench_pwm_hits.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pwm_hits.py --once     # one call each: the kernels' own times
"""
import json
import os
import sys

import numpy as np

import bench_twobit as B
from bench_pwm import MOTIF, motif_rows
from bench_twobit import N, REPS, SIZE, WARM, WIDTH

SAMPLE = min(int(os.environ.get("SAMPLE", 2000)), N)
LONG_REPS = max(1, min(REPS, 5))


def main():
    import torch

    from bxmi import motif, sequence

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

    seq = B.synthetic()
    track = sequence.TwoBitTrack.from_arrays(seq[0], SIZE, *seq[1:])
    forward = motif.ScoringMatrix("ACGT", motif_rows())
    ms = motif.MatrixSet([forward, forward.reverse_complement()])
    short_h, _ = B.sites()
    track_of = torch.zeros(N, dtype=torch.int32, device="cuda")
    short = torch.from_numpy(short_h).cuda()
    short_end = short + WIDTH
    out = torch.empty((2, N, WIDTH), dtype=torch.float32, device="cuda")

    # the thresholds: the scores of the first SAMPLE sites, NaN counted as no hit
    sample = motif.score_matrix_dev([track], track_of[:SAMPLE], short[:SAMPLE], WIDTH, ms).flatten()
    numbers = torch.sort(sample[~torch.isnan(sample)], descending=True).values
    thresholds = {name: float(numbers[min(int(sample.numel() * share), numbers.numel() - 1)]) for name, share in (("rare", 1e-5), ("sparse", 1e-3), ("dense", 1e-1))}
    result = {"size": SIZE, "sites": N, "width": WIDTH, "motif": MOTIF, "matrices": 2, "elements": 2 * N * WIDTH, "plane_bytes": out.numel() * 4}
    res = {}
    for name, t in thresholds.items():
        counts = motif.hits_dev([track], track_of, short, short_end, ms, t)[0]  # (untimed: how many there are)
        cap = int(counts[-1]) + 1024

        def hits():
            res["h"] = motif.hits_dev([track], track_of, short, short_end, ms, t, max_hits=cap)

        def planes_route():
            motif.score_matrix_dev([track], track_of, short, WIDTH, ms, out=out)
            mask = out >= t
            res["p"] = (mask.nonzero(), out[mask])

        h, p = timed(hits, REPS, WARM), timed(planes_route, REPS, WARM)
        mat_hits, rows, pos, score = res["h"]
        where, values = res["p"]
        same = (int(mat_hits[-1]) == where.shape[0] and bool((where[:, 1] == rows).all()) and bool((where[:, 2] == pos).all())
                and bool((values.view(torch.int32) == score.view(torch.int32)).all())
                and np.array_equal(np.diff(mat_hits), torch.bincount(where[:, 0], minlength=2).cpu().numpy()))
        result[name] = {"threshold": t, "hits": int(mat_hits[-1]), "hits_per_matrix": np.diff(mat_hits).tolist(),
                        "share_of_elements": round(int(mat_hits[-1]) / (2 * N * WIDTH), 6), "hits_dev": h, "planes_route": p,
                        "planes_over_hits": round(p["median_ms"] / h["median_ms"], 3), "same_hits": same}
        res.clear()
    del out
    torch.cuda.empty_cache()

    # one row of the whole sequence
    one, first, last = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, 0, SIZE))
    result["whole_sequence"] = {"planes_route_bytes": 2 * SIZE * 4}
    for name in ("rare", "sparse"):
        t = thresholds[name]
        counts = motif.hits_dev([track], one, first, last, ms, t)[0]
        cap = int(counts[-1]) + 1024

        def whole():
            res["w"] = motif.hits_dev([track], one, first, last, ms, t, max_hits=cap)

        w = timed(whole, LONG_REPS, min(WARM, 1))
        w.update(threshold=t, hits=int(res["w"][0][-1]), bases_per_s=round(SIZE / (w["median_ms"] * 1e-3)))
        result["whole_sequence"][name] = w
    print(json.dumps(result))
    ms.close()
    track.close()
    if not all(result[name]["same_hits"] for name in thresholds):
        sys.exit("the two routes list different hits: the times above measure a wrong result")


if __name__ == "__main__":
    main()
