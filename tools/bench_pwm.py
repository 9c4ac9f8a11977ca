#!/usr/bin/env python
"""
Position weight matrix scores over 2bit sites at scale, timed on the device: the synthetic sequence and the sites of
tools/bench_twobit.py (SIZE = 250 M bases, N = 100 k sites of WIDTH = 1000 bases) and one seeded matrix of MOTIF (default 20)
positions over ACGT plus its reverse complement, as one MatrixSet.  From device arrays through the `_dev` entry points, HIP-event
timed: 2 warm-up runs, then REPS (default 15) repetitions, median and range.  Prints one JSON line with two figures:

  score_matrix   the 2 x N x WIDTH float32 scores, bxmi_twobit_pwm_scores_dev; `fraction_of_hbm_peak` is the OUTPUT bytes
                 (2 * N * WIDTH * 4; the packed input is a sixteenth of one plane) over the median time over 8 TB/s -- a
                 whole-call figure: how far the pass is from its store floor, not what the memory system did;
  best           the best hit of every site and matrix, bxmi.motif.best_dev: no per-base output at all.  The window holds torch's
                 clipping of the rows as well as the call.

MODEL_ROWS (default 100) sites are also scored on the host by tests/pwm_model.py from the host's own letters and compared bit
for bit; if they differ the tool exits with an error after printing its line.

    python tools/bench_pwm.py
    SIZE=20000000 N=20000 python tools/bench_pwm.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pwm.py --once     # one call each: the kernels' own times

    python tools/bench_pwm.py --reference REFERENCE_LIB_DIR      # no device: the reference's loop on one CPU core
times, for the same sites, `ScoringMatrix.score_string` of both matrices on the site's string (made on the host from the packed
bytes; making it is not timed) for REF_N sites (default 2000) and scales the time linearly to N.  REFERENCE_LIB_DIR holds the
reference's bx package; bx.motif._pwm is built out of its tree as tools/record_pwm_golden.py does.
"""
import json
import os
import sys
import time

import numpy as np

import bench_twobit as B
from bench_twobit import HBM_PEAK, N, ONCE, REFERENCE, REPS, SIZE, WARM, WIDTH

sys.path.insert(0, os.path.join(B.ROOT, "tests"))

MOTIF = int(os.environ.get("MOTIF", 20))
MODEL_ROWS = 0 if ONCE else int(os.environ.get("MODEL_ROWS", 100))


def motif_rows():
    return np.random.default_rng(13).normal(0.0, 2.0, (MOTIF, 4)).astype(np.float32)


def reference_main():
    import types

    import record_pwm_golden as R

    lib = os.path.abspath(REFERENCE)
    built = R.build_extension(lib)
    for pkg, where in (("bx", [os.path.join(lib, "bx")]), ("bx.motif", [os.path.join(lib, "bx", "motif"), built])):
        module = types.ModuleType(pkg)
        module.__path__ = where
        sys.modules[pkg] = module
    from bx.motif.pwm import ScoringMatrix

    forward = ScoringMatrix.from_rows(list("ACGT"), motif_rows().tolist())
    mats = [forward, forward.reverse_complement()]
    seq = B.synthetic()
    short, _ = B.sites()
    ref_n = min(int(os.environ.get("REF_N", 2000)), N)
    texts = [B.window(seq, int(s), int(s) + WIDTH).tobytes().decode() for s in short[:ref_n]]
    t0 = time.perf_counter()
    for text in texts:
        for m in mats:
            m.score_string(text)
    t_score = time.perf_counter() - t0
    print(json.dumps({"reference": True, "size": SIZE, "sites": N, "width": WIDTH, "motif": MOTIF, "matrices": 2,
                      "score_string": {"timed_sites": ref_n, "seconds": round(t_score, 3), "scaled_s": round(t_score * N / ref_n, 2)}}))


def main():
    import torch

    import pwm_model as P
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
    res = {}

    def score_matrix():
        motif.score_matrix_dev([track], track_of, short, WIDTH, ms, out=out)

    def best():
        res["b"] = motif.best_dev([track], track_of, short, short_end, ms)

    m, b = timed(score_matrix, REPS, WARM), timed(best, REPS, WARM)
    out_bytes = out.numel() * 4
    m.update(output_bytes=out_bytes, GBps_output=round(out_bytes / (m["median_ms"] * 1e-3) / 1e9, 1),
             fraction_of_hbm_peak=round(out_bytes / (m["median_ms"] * 1e-3) / HBM_PEAK, 4))
    b.update(bases_per_s=round(N * WIDTH / (b["median_ms"] * 1e-3)))
    result = {"size": SIZE, "sites": N, "width": WIDTH, "motif": MOTIF, "matrices": 2, "score_matrix": m, "best": b}
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        mats = [P.Matrix("ACGT", motif_rows())]
        mats.append(mats[0].reverse_complement())
        got = out[:, :rows].cpu().numpy()
        top, at = (x[:, :rows].cpu().numpy() for x in res["b"])
        same = True
        for i, s in enumerate(short_h[:rows]):
            text = B.window(seq, int(s), int(s) + WIDTH)
            for k, mat in enumerate(mats):
                want = mat.score(text)
                score, pos = P.best_of(want)
                same &= np.array_equal(P.bits(got[k, i]), P.bits(want)) and P.bits(top[k, i])[0] == P.bits(np.float32(score))[0] and at[k, i] == pos
        result.update(model_rows=rows, equals_model=bool(same))
    print(json.dumps(result))
    ms.close()
    track.close()
    if not result.get("equals_model", True):
        sys.exit("the device's scores differ from the host's: the times above measure a wrong result")


if __name__ == "__main__":
    reference_main() if REFERENCE else main()
