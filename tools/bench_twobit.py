#!/usr/bin/env python
"""
2bit sequence extraction and base counts at scale, timed on the device: one synthetic sequence of SIZE bases (default 250 M) with
random codes, N blocks like an assembly's gaps (two telomeres of 10 kb and GAPS = 40 gaps of 1 kb to 1 Mb) and mask blocks like
RepeatMasker's (one every 600 bases on average, 1 to 600 bases long: about 400 k blocks over half of the sequence), and N sites
(default 100 k).  From device arrays through the `_dev` entry points, HIP-event timed: 2 warm-up runs, then REPS (default 15)
repetitions, median and range.  Prints one JSON line with three figures:

  matrix             the N x WIDTH (default 1000) letter matrix, bxmi_twobit_bases_dev; `fraction_of_hbm_peak` is the OUTPUT bytes
                     (N * WIDTH; the packed input is a quarter of that again) over the median time over 8 TB/s -- a whole-call
                     figure: how far the pass is from its store floor, not what the memory system did;
  composition        the same rows through bxmi_twobit_composition_dev;
  composition_long   N rows of LONG (default 1 M) bases through the same entry point.  The work per row is the same, so the two
                     times should be close: `long_over_short` is their ratio.

Each timed window is ONE call: it holds the call through ctypes, the launch that fills the track table and the kernel, so the two
composition figures share a fixed overhead and their ratio understates a difference between the kernels.  The kernels' own times
come from a trace, in a run of its own: `REPS=5 rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_twobit.py` lists 7
dispatches of tb_bases_kernel and 14 of tb_composition_kernel in time order -- 2 warm-up and 5 timed calls of the short rows, then
the same of the long ones.

MODEL_ROWS (default 200) rows of each are also computed on the host from the packed bytes and the blocks and compared byte for
byte; if they differ the tool exits with an error after printing its line.

    python tools/bench_twobit.py
    SIZE=20000000 N=20000 python tools/bench_twobit.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_twobit.py --once     # one call each: the kernels' own times

    python tools/bench_twobit.py --reference REFERENCE_LIB_DIR      # no device: the reference's loop on one CPU core
writes the same sequence as a .2bit file (TMPDIR) and times, for the same sites, `TwoBitSequence.get` once per site and the counts
taken from its strings (`str.count` per letter, as a user of the reference would), REF_N sites each (default: all N for the short
rows, 200 for the long ones, scaled linearly to N).  REFERENCE_LIB_DIR holds the reference's bx package with bx.seq._twobit built
(tools/record_twobit_golden.py says how).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bx-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

ONCE = "--once" in sys.argv
REFERENCE = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else None
REPS = 1 if ONCE else int(os.environ.get("REPS", 15))
WARM = 0 if ONCE else 2
SIZE = int(os.environ.get("SIZE", 250_000_000))
N = int(os.environ.get("N", 100_000))
WIDTH = int(os.environ.get("WIDTH", 1000))
LONG = int(os.environ.get("LONG", 1_000_000))
GAPS = int(os.environ.get("GAPS", 40))
MODEL_ROWS = 0 if ONCE else int(os.environ.get("MODEL_ROWS", 200))
HBM_PEAK = 8.0e12  # bytes per second


def synthetic():
    """(packed uint8, n_starts, n_sizes, m_starts, m_sizes) of the sequence; the same for every caller"""
    rng = np.random.default_rng(11)
    packed = rng.integers(0, 256, size=(SIZE + 3) // 4, dtype=np.uint8)
    # gaps: the two telomeres, and GAPS more spread over the sequence, each inside its own stretch
    stretch = (SIZE - 20_000) // GAPS
    limit = max(min(1_000_000, stretch // 2), 1001)
    g_sizes = rng.integers(1000, limit, size=GAPS)
    g_starts = 10_000 + np.arange(GAPS) * stretch + rng.integers(0, stretch - g_sizes)
    n_starts = np.concatenate([[0], g_starts, [SIZE - 10_000]])
    n_sizes = np.concatenate([[10_000], g_sizes, [10_000]])
    # repeats: a gap of 1 .. 600 bases, a block of 1 .. 600, and so on to the end
    count = SIZE // 500
    steps = rng.integers(1, 601, size=(count, 2))
    ends = np.cumsum(steps.reshape(-1)).reshape(count, 2)
    keep = ends[:, 1] <= SIZE
    m_starts, m_sizes = ends[keep, 0], steps[keep, 1]
    return packed, n_starts, n_sizes, m_starts, m_sizes


def sites():
    rng = np.random.default_rng(12)
    short = rng.integers(0, SIZE - WIDTH, size=N).astype(np.int32)
    long_ = rng.integers(0, SIZE - LONG, size=N).astype(np.int32)
    return short, long_


def window(seq, s, e):
    """the letters of [s, e) on the host, from the packed bytes and the blocks"""
    packed, n_starts, n_sizes, m_starts, m_sizes = seq
    p = packed[s // 4:(e + 3) // 4]
    codes = np.stack([(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3], axis=1).reshape(-1)[s % 4:s % 4 + e - s]
    out = np.frombuffer(b"TCAG", dtype=np.uint8)[codes].copy()
    for starts, sizes, lower in ((n_starts, n_sizes, False), (m_starts, m_sizes, True)):
        k = max(int(np.searchsorted(starts, s, side="right")) - 1, 0)
        while k < len(starts) and starts[k] < e:
            a, b = max(int(starts[k]), s) - s, min(int(starts[k] + sizes[k]), e) - s
            if a < b:
                if lower:
                    out[a:b] |= 0x20
                else:
                    out[a:b] = ord("N")
            k += 1
    return out


def counts_of(text):
    upper = text & ~np.uint8(0x20)
    return [int((upper == ord(c)).sum()) for c in "ACGTN"] + [int((text >= ord("a")).sum())]


def reference_main():
    import tempfile
    import types

    import write_twobit_fixture as W

    lib = os.path.abspath(REFERENCE)
    for pkg, where in (("bx", os.path.join(lib, "bx")), ("bx.seq", os.path.join(lib, "bx", "seq"))):
        module = types.ModuleType(pkg)
        module.__path__ = [where]
        sys.modules[pkg] = module
    from bx.seq.twobit import TwoBitFile

    packed, n_starts, n_sizes, m_starts, m_sizes = synthetic()
    short, long_ = sites()
    ref_n = int(os.environ.get("REF_N", N))
    ref_long = int(os.environ.get("REF_LONG_N", 200))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synthetic.2bit")
        W.write_2bit_packed(path, "chrS", SIZE, packed, list(zip(n_starts.tolist(), n_sizes.tolist())), list(zip(m_starts.tolist(), m_sizes.tolist())))
        with open(path, "rb") as f:
            seq = TwoBitFile(f)["chrS"]
            t0 = time.perf_counter()
            for s in short[:ref_n].tolist():
                seq.get(s, s + WIDTH)
            t_get = time.perf_counter() - t0
            t0 = time.perf_counter()
            for s in short[:ref_n].tolist():
                text = seq.get(s, s + WIDTH)
                upper = text.upper()
                [upper.count(c) for c in "ACGTN"] + [sum(map(str.islower, text))]
            t_comp = time.perf_counter() - t0
            t0 = time.perf_counter()
            for s in long_[:ref_long].tolist():
                text = seq.get(s, s + LONG)
                upper = text.upper()
                [upper.count(c) for c in "ACGTN"] + [sum(map(str.islower, text))]
            t_long = time.perf_counter() - t0
    print(json.dumps({"reference": True, "size": SIZE, "sites": N, "width": WIDTH, "long": LONG,
                      "get": {"timed_sites": ref_n, "seconds": round(t_get, 3), "scaled_s": round(t_get * N / ref_n, 2)},
                      "composition": {"timed_sites": ref_n, "seconds": round(t_comp, 3), "scaled_s": round(t_comp * N / ref_n, 2)},
                      "composition_long": {"timed_sites": ref_long, "seconds": round(t_long, 3), "scaled_s": round(t_long * N / ref_long, 1)}}))


def main():
    import torch

    from bxmi import sequence

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

    seq = synthetic()
    t0 = time.perf_counter()
    track = sequence.TwoBitTrack.from_arrays(seq[0], SIZE, *seq[1:])
    create_s = time.perf_counter() - t0
    short_h, long_h = sites()
    track_of = torch.zeros(N, dtype=torch.int32, device="cuda")
    short, long_ = torch.from_numpy(short_h).cuda(), torch.from_numpy(long_h).cuda()
    short_end, long_end = short + WIDTH, long_ + LONG
    out = torch.empty((N, WIDTH), dtype=torch.uint8, device="cuda")
    res = {}

    def matrix():
        sequence.matrix_dev([track], track_of, short, WIDTH, out=out)

    def comp():
        res["c"] = sequence.composition_dev([track], track_of, short, short_end)

    def comp_long():
        res["l"] = sequence.composition_dev([track], track_of, long_, long_end)

    m, c, lg = timed(matrix, REPS, WARM), timed(comp, REPS, WARM), timed(comp_long, REPS, WARM)
    m.update(output_bytes=N * WIDTH, GBps_output=round(N * WIDTH / (m["median_ms"] * 1e-3) / 1e9, 1),
             fraction_of_hbm_peak=round(N * WIDTH / (m["median_ms"] * 1e-3) / HBM_PEAK, 4))
    c.update(rows_per_s=round(N / (c["median_ms"] * 1e-3)))
    lg.update(rows_per_s=round(N / (lg["median_ms"] * 1e-3)), bases_per_row=LONG)
    result = {"size": SIZE, "n_blocks": len(seq[1]), "mask_blocks": len(seq[3]), "masked_fraction": round(float(seq[4].sum()) / SIZE, 3), "sites": N,
              "width": WIDTH, "create_s": round(create_s, 3), "matrix": m, "composition": c, "composition_long": lg,
              "long_over_short": round(lg["median_ms"] / c["median_ms"], 3)}
    if MODEL_ROWS > 0:
        rows = min(MODEL_ROWS, N)
        got, got_c, got_l = out[:rows].cpu().numpy(), res["c"][:rows].cpu().numpy(), res["l"][:max(rows // 20, 1)].cpu().numpy()
        same = all(np.array_equal(got[i], window(seq, int(s), int(s) + WIDTH)) for i, s in enumerate(short_h[:rows]))
        same_c = all(got_c[i].tolist() == counts_of(window(seq, int(s), int(s) + WIDTH)) for i, s in enumerate(short_h[:rows]))
        same_l = all(got_l[i].tolist() == counts_of(window(seq, int(s), int(s) + LONG)) for i, s in enumerate(long_h[:len(got_l)]))
        result.update(model_rows=rows, equals_model=bool(same and same_c and same_l))
    print(json.dumps(result))
    track.close()
    if not result.get("equals_model", True):
        sys.exit("the device's rows differ from the host's: the times above measure a wrong result")


if __name__ == "__main__":
    reference_main() if REFERENCE else main()
