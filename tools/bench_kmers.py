#!/usr/bin/env python
"""
K-mer counts over 2bit sites at scale, timed on the device against the route a user had before: the sequence workload of
tools/bench_twobit.py (SIZE = 250 M bases, N = 100 k sites of WIDTH = 1000 bases), the case-folded ACGT alphabet.  HIP-event
timed, 2 warm-up runs, then REPS repetitions, median and range, every route in the same run on the same tensors.  Prints one JSON
line; per k in 2, 4, 6:

  plan           bxmi.kmers.count_matrix_dev into a preallocated N x 4^k tensor, the way csrc/kmer.hpp's km_use_lds chooses;
  lds, direct    the same with the LDS histogram forced and with the atomics sent straight to HBM (bxmi_twobit_kmer_force);
  torch_route    bxmi.sequence.matrix_dev (N x WIDTH bytes), a lookup of the digits, the words as a sum over k shifted views and a
                 scatter-add into N x 4^k (int32), with torch;
  same_counts    whether the four agree.

`whole_sequence` times ONE row of all SIZE bases per k (and k = 7, which has more words than a workgroup keeps in LDS) each way
the plan allows.  `cutoff` measures where the two ways cross: 4^k words for k = 2 .. 6 against rows of 32 .. 2048 bases, CUT_BASES
bases in all (at most 2 M rows), each way forced; the KM_CUT of csrc/kmer.hpp is read off it.

    python tools/bench_kmers.py
    SIZE=20000000 N=20000 python tools/bench_kmers.py
"""
import json
import os
import sys

import numpy as np

import bench_twobit as B
from bench_twobit import N, REPS, SIZE, WARM, WIDTH

LONG_REPS = max(1, min(REPS, 5))
CUT_BASES = int(os.environ.get("CUT_BASES", 50_000_000))
KS = (2, 4, 6)


def main():
    import torch

    from bxmi import _ffi, kmers, sequence

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

    def forced(way, fn):
        def run():
            _ffi.call("bxmi_twobit_kmer_force", way)
            try:
                fn()
            finally:
                _ffi.call("bxmi_twobit_kmer_force", 0)
        return run

    seq = B.synthetic()
    track = sequence.TwoBitTrack.from_arrays(seq[0], SIZE, *seq[1:])
    short_h, _ = B.sites()
    track_of = torch.zeros(N, dtype=torch.int32, device="cuda")
    short = torch.from_numpy(short_h).cuda()
    lookup = torch.full((256,), -1, dtype=torch.int64, device="cuda")
    for d, ch in enumerate("ACGT"):
        lookup[ord(ch)] = lookup[ord(ch.lower())] = d
    letters = torch.empty((N, WIDTH), dtype=torch.uint8, device="cuda")
    result = {"size": SIZE, "sites": N, "width": WIDTH, "alphabet": "ACGT, case folded", "lds_bins": 4096}
    ways = (("plan", 0), ("lds", 1), ("direct", 2))

    for k in KS:
        bins = 4 ** k
        out = {name: torch.empty((N, bins), dtype=torch.int32, device="cuda") for name, _ in ways}
        res = {}

        def ours(name):
            return lambda: kmers.count_matrix_dev([track], track_of, short, WIDTH, k, case_sensitive=False, out=out[name])

        def torch_route():
            sequence.matrix_dev([track], track_of, short, WIDTH, out=letters)
            digit = lookup[letters.to(torch.int64)]
            windows = WIDTH - k + 1
            word = torch.zeros((N, windows), dtype=torch.int64, device="cuda")
            ok = torch.ones((N, windows), dtype=torch.bool, device="cuda")
            for t in range(k):
                part = digit[:, t:t + windows]
                ok &= part >= 0
                word += part.clamp(min=0) * 4 ** t
            word += torch.arange(N, device="cuda").unsqueeze(1) * bins
            table = torch.zeros(N * bins, dtype=torch.int32, device="cuda")
            index = word[ok]
            table.scatter_add_(0, index, torch.ones(1, dtype=torch.int32, device="cuda").expand(index.numel()))
            res["t"] = table.view(N, bins)

        entry = {"bins": bins, "out_bytes": N * bins * 4}
        for name, way in ways:
            entry[name] = timed(forced(way, ours(name)), REPS, WARM)
        entry["torch_route"] = timed(torch_route, max(REPS // 3, 3), 1)
        entry["same_counts"] = all(bool((out[name] == res["t"]).all()) for name, _ in ways)
        entry["words_counted"] = int(res["t"].sum(dtype=torch.int64))
        entry["torch_over_plan"] = round(entry["torch_route"]["median_ms"] / entry["plan"]["median_ms"], 3)
        result["k%d" % k] = entry
        del out, res
        torch.cuda.empty_cache()
    del letters
    torch.cuda.empty_cache()

    # one row of the whole sequence
    one, first = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, 0))
    result["whole_sequence"] = {}
    for k in KS + (7,):
        bins = 4 ** k
        out = torch.empty((1, bins), dtype=torch.int32, device="cuda")
        entry, seen = {"bins": bins}, []
        for name, way in ways:
            if name == "lds" and bins > result["lds_bins"]:
                continue
            w = timed(forced(way, lambda: kmers.count_matrix_dev([track], one, first, SIZE, k, case_sensitive=False, out=out)), LONG_REPS, min(WARM, 1))
            w["bases_per_s"] = round(SIZE / (w["median_ms"] * 1e-3))
            entry[name] = w
            seen.append(out.clone())
        entry["same_counts"] = all(bool((s == seen[0]).all()) for s in seen)
        entry["words_counted"] = int(seen[0].sum(dtype=torch.int64))
        result["whole_sequence"]["k%d" % k] = entry

    # where the two ways cross: rows of `width` bases, CUT_BASES in all
    result["cutoff"] = {}
    rng = np.random.default_rng(13)
    for k in (2, 3, 4, 5, 6):
        bins = 4 ** k
        for width in (32, 64, 128, 192, 256, 320, 384, 448, 512, 1024, 2048):
            rows = max(min(CUT_BASES // width, 2_000_000, (1 << 30) // bins), 1)  # (at most 4 GiB of counts)
            starts = torch.from_numpy(rng.integers(0, SIZE - width, size=rows).astype(np.int32)).cuda()
            which = torch.zeros(rows, dtype=torch.int32, device="cuda")
            out = torch.empty((rows, bins), dtype=torch.int32, device="cuda")
            entry = {"rows": rows}
            for name, way in ways[1:]:
                entry[name] = timed(forced(way, lambda: kmers.count_matrix_dev([track], which, starts, width, k, case_sensitive=False, out=out)),
                                    LONG_REPS, 1)["median_ms"]
            entry["direct_over_lds"] = round(entry["direct"] / entry["lds"], 3)
            result["cutoff"]["bins%d_width%d" % (bins, width)] = entry
            del out
        torch.cuda.empty_cache()
    print(json.dumps(result))
    track.close()
    if not all(result["k%d" % k]["same_counts"] for k in KS) or not all(v["same_counts"] for v in result["whole_sequence"].values()):
        sys.exit("the routes count differently: the times above measure a wrong result")


if __name__ == "__main__":
    main()
