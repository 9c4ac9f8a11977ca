#!/usr/bin/env python
"""
Strand-aware position weight matrix scores over 2bit sites at scale, timed on the device: the workload of tools/bench_pwm.py (SIZE =
250 M bases, N = 100 k sites of WIDTH = 1000 bases, one seeded matrix of MOTIF = 20 positions over ACGT plus its reverse complement)
through `score_matrix_dev`, `best_dev` and `hits_dev` -- the last at the three thresholds of tools/bench_pwm_hits.py -- by five routes
in the same run on the same tensors.  HIP-event timed, 2 warm-up runs, then REPS (default 15) repetitions, median and range.  Prints
one JSON line; per call:

  unstranded     strands=None: the kernels of before;
  all_minus      every site on the minus strand;
  half_minus     a seeded random half of the sites on the minus strand;
  zeros          a strand tensor of zeros: the plus path of the STRANDED kernels;
  before         what a user had before (score_matrix alone): the planes of the all-plus call -- whose second matrix is the reverse
                 complement -- then, for the minus sites, torch's flip along the offsets, a shift by the motif's width and the swap
                 of the two planes.  NOT bit-identical to the minus strand: the same terms added in the opposite order
                 (`before_equal_share`: the share of the scored minus elements whose bits agree all the same).

`whole_sequence` times best_dev and hits_dev (the rare threshold) on ONE minus row of all SIZE bases against the same row on the
plus strand; `short_rows` times score_matrix_dev on N * WIDTH / 32 rows of 32 bases, all minus against unstranded.  MODEL_ROWS
(default 100) minus sites are compared bit for bit with tests/pwm_strand_model.py on the host's own letters; if they differ the
tool exits with an error after printing its line.

    python tools/bench_pwm_strand.py
    SIZE=20000000 N=20000 python tools/bench_pwm_strand.py
"""
import json
import os
import sys

import numpy as np

import bench_twobit as B
from bench_pwm import MODEL_ROWS, MOTIF, motif_rows
from bench_pwm_hits import LONG_REPS, SAMPLE
from bench_twobit import N, REPS, SIZE, WARM, WIDTH

sys.path.insert(0, os.path.join(B.ROOT, "tests"))


def main():
    import torch

    import pwm_model as P
    import pwm_strand_model as PS
    from bxmi import motif, sequence

    def timed(fn, reps=REPS, warm=WARM):
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
    half_h = np.random.default_rng(17).integers(0, 2, N).astype(np.int8)
    strands = {"unstranded": None, "all_minus": torch.ones(N, dtype=torch.int8, device="cuda"), "half_minus": torch.from_numpy(half_h).cuda(),
               "zeros": torch.zeros(N, dtype=torch.int8, device="cuda")}
    result = {"size": SIZE, "sites": N, "width": WIDTH, "motif": MOTIF, "matrices": 2, "score_matrix": {}, "best": {}, "hits": {}}
    res = {}

    for name, st in strands.items():
        result["score_matrix"][name] = timed(lambda: motif.score_matrix_dev([track], track_of, short, WIDTH, ms, out=out, strands=st))
        result["best"][name] = timed(lambda: res.__setitem__("b", motif.best_dev([track], track_of, short, short_end, ms, strands=st)))

    # the route of before, for the random half: plus planes, then flip, shift and swap of the minus rows
    minus_rows = torch.from_numpy(np.flatnonzero(half_h)).cuda()
    nan = torch.full((), float("nan"), dtype=torch.float32, device="cuda")

    def before():
        motif.score_matrix_dev([track], track_of, short, WIDTH, ms, out=out)
        part = out[:, minus_rows].flip(0).flip(2)  # (plane m of a minus row: the other matrix's plane, read backwards)
        shifted = torch.cat([part[:, :, MOTIF - 1:], nan.expand(2, part.shape[1], MOTIF - 1)], dim=2)
        out[:, minus_rows] = shifted

    result["score_matrix"]["before"] = timed(before)
    route = out[:, minus_rows].clone()
    motif.score_matrix_dev([track], track_of, short, WIDTH, ms, out=out, strands=strands["half_minus"])
    exact = out[:, minus_rows]
    scored = ~torch.isnan(exact)
    result["score_matrix"]["before_same_nans"] = bool((torch.isnan(route) == torch.isnan(exact)).all())
    result["score_matrix"]["before_equal_share"] = round(float((route.view(torch.int32) == exact.view(torch.int32))[scored].float().mean()), 4)
    del route, exact, scored

    # the model, on the first minus sites of the random half
    if MODEL_ROWS > 0:
        mats = [P.Matrix("ACGT", motif_rows())]
        mats.append(mats[0].reverse_complement())
        rows = [int(i) for i in np.flatnonzero(half_h)[:MODEL_ROWS]]
        got = out[:, rows].cpu().numpy()
        same = True
        for k, i in enumerate(rows):
            text = B.window(seq, int(short_h[i]), int(short_h[i]) + WIDTH)
            for m, mat in enumerate(mats):
                same &= np.array_equal(P.bits(got[m, k]), P.bits(PS.score(mat, text, True)))
        result.update(model_rows=len(rows), equals_model=bool(same))

    # hits at the thresholds of bench_pwm_hits.py
    sample = motif.score_matrix_dev([track], track_of[:SAMPLE], short[:SAMPLE], WIDTH, ms).flatten()
    numbers = torch.sort(sample[~torch.isnan(sample)], descending=True).values
    thresholds = {name: float(numbers[min(int(sample.numel() * share), numbers.numel() - 1)]) for name, share in (("rare", 1e-5), ("sparse", 1e-3), ("dense", 1e-1))}
    for level, t in thresholds.items():
        result["hits"][level] = {"threshold": t}
        for name, st in strands.items():
            counts = motif.hits_dev([track], track_of, short, short_end, ms, t, strands=st)[0]
            cap = int(counts[-1]) + 1024
            h = timed(lambda: res.__setitem__("h", motif.hits_dev([track], track_of, short, short_end, ms, t, max_hits=cap, strands=st)))
            h.update(hits=int(counts[-1]))
            result["hits"][level][name] = h
    del out
    res.clear()
    torch.cuda.empty_cache()

    # one row of the whole sequence
    one, first, last = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, 0, SIZE))
    result["whole_sequence"] = {}
    for name, st in (("plus", None), ("minus", torch.ones(1, dtype=torch.int8, device="cuda"))):
        w = {"best": timed(lambda: motif.best_dev([track], one, first, last, ms, strands=st), LONG_REPS, min(WARM, 1))}
        cap = int(motif.hits_dev([track], one, first, last, ms, thresholds["rare"], strands=st)[0][-1]) + 1024
        w["hits_rare"] = timed(lambda: motif.hits_dev([track], one, first, last, ms, thresholds["rare"], max_hits=cap, strands=st), LONG_REPS, min(WARM, 1))
        result["whole_sequence"][name] = w

    # rows of 32 bases: many segments per tile
    n32 = N * WIDTH // 32
    starts32 = torch.from_numpy(np.random.default_rng(19).integers(0, SIZE - 32, n32).astype(np.int32)).cuda()
    track32 = torch.zeros(n32, dtype=torch.int32, device="cuda")
    out32 = torch.empty((2, n32, 32), dtype=torch.float32, device="cuda")
    result["short_rows"] = {"rows": n32, "width": 32}
    for name, st in (("unstranded", None), ("all_minus", torch.ones(n32, dtype=torch.int8, device="cuda"))):
        result["short_rows"][name] = timed(lambda: motif.score_matrix_dev([track], track32, starts32, 32, ms, out=out32, strands=st))
    print(json.dumps(result))
    ms.close()
    track.close()
    if not result.get("equals_model", True):
        sys.exit("the device's minus scores differ from the host's: the times above measure a wrong result")


if __name__ == "__main__":
    main()
