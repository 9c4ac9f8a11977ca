#!/usr/bin/env python
"""
Strand-aware letters, base counts and k-mer counts at scale, timed on the device against the unstranded calls and against the route
a user had before: the sequence workload of tools/bench_twobit.py (SIZE = 250 M bases, N = 100 k sites of WIDTH = 1000 bases).
HIP-event timed, 2 warm-up runs, then REPS (default 15) repetitions, median and range, every route in the same run on the same
tensors.  Prints one JSON line.  Three strand settings: `minus` (every row), `half` (a random half), `plus` (a strand tensor of
zeros through the stranded entry points).

  letters      sequence.matrix_dev into a preallocated N x WIDTH tensor: `unstranded` (no strands: the call of before), the three
               settings, and `torch_route`, what a user did for `half`: matrix_dev, then a flip along the row and a 256-entry
               complement lookup on the minus rows (the pad is N here, which is its own complement; a pad that is a letter would
               need a mask as well);
  composition  sequence.composition_dev: unstranded, the three settings, and the torch route (a column gather on the minus rows);
  k2, k4, k6   kmers.count_matrix_dev, case-folded ACGT, into a preallocated N x 4^k tensor: unstranded, the three settings, and
               the torch route: count_matrix_dev without strands, then the gather of kmers.strand_columns on the minus rows;
  whole_sequence   ONE minus row of all SIZE bases: letters (SIZE bytes out), k = 4 and k = 7, beside the plus row;
  rows_of_32   SHORT_BASES (default 50 M) bases in rows of 32: letters and k = 2, plus and minus.

`same_*` says whether the stranded result of `half` equals the torch route's, whether `plus` equals `unstranded`, and whether the
first MODEL_ROWS minus rows equal the host's reverse complement of the rows cut from the packed bytes; if any is false the tool
exits with an error after printing its line.  `x_over_unstranded` is a median over the unstranded median (above 1: SLOWER).

    python tools/bench_strand.py
    SIZE=20000000 N=20000 python tools/bench_strand.py
"""
import json
import os
import sys

import numpy as np

import bench_twobit as B
from bench_twobit import MODEL_ROWS, N, REPS, SIZE, WARM, WIDTH

LONG_REPS = max(1, min(REPS, 5))
SHORT_BASES = int(os.environ.get("SHORT_BASES", 50_000_000))
KS = (2, 4, 6)

COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in zip("ACGTNacgtn", "TGCANtgcan"):
    COMPLEMENT[ord(_a)] = ord(_b)


def main():
    import torch

    from bxmi import kmers, sequence

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

    def ratios(entry, base="unstranded"):
        for name in list(entry):
            if isinstance(entry[name], dict) and name != base:
                entry[name + "_over_" + base] = round(entry[name]["median_ms"] / entry[base]["median_ms"], 3)

    seq = B.synthetic()
    track = sequence.TwoBitTrack.from_arrays(seq[0], SIZE, *seq[1:])
    short_h, _ = B.sites()
    half_h = np.random.default_rng(14).integers(0, 2, N).astype(np.int8)
    track_of = torch.zeros(N, dtype=torch.int32, device="cuda")
    short = torch.from_numpy(short_h).cuda()
    short_end = short + WIDTH
    strands = {"minus": torch.ones(N, dtype=torch.int8, device="cuda"), "half": torch.from_numpy(half_h).cuda(), "plus": torch.zeros(N, dtype=torch.int8, device="cuda")}
    is_minus = strands["half"].bool()
    lookup = torch.from_numpy(COMPLEMENT).cuda()
    result = {"size": SIZE, "sites": N, "width": WIDTH, "minus_rows_of_half": int(half_h.sum()), "alphabet": "ACGT, case folded"}
    ok = True

    # ---- letters
    out = {name: torch.empty((N, WIDTH), dtype=torch.uint8, device="cuda") for name in ("unstranded", "minus", "half", "plus", "torch_route")}
    entry = {"out_bytes": N * WIDTH}
    entry["unstranded"] = timed(lambda: sequence.matrix_dev([track], track_of, short, WIDTH, out=out["unstranded"]))
    for name, st in strands.items():
        entry[name] = timed(lambda: sequence.matrix_dev([track], track_of, short, WIDTH, out=out[name], strands=st))

    def letters_route():
        o = out["torch_route"]
        sequence.matrix_dev([track], track_of, short, WIDTH, out=o)
        o[is_minus] = lookup[o[is_minus].flip(1).long()]

    entry["torch_route"] = timed(letters_route, max(REPS // 3, 3), 1)
    rows = min(MODEL_ROWS, N)
    got = out["minus"][:rows].cpu().numpy()
    entry["same_as_torch_route"] = bool((out["half"] == out["torch_route"]).all())
    entry["plus_same_as_unstranded"] = bool((out["plus"] == out["unstranded"]).all())
    entry["same_as_model"] = all(np.array_equal(got[i], COMPLEMENT[B.window(seq, int(s), int(s) + WIDTH)][::-1]) for i, s in enumerate(short_h[:rows]))
    entry["torch_over_half"] = round(entry["torch_route"]["median_ms"] / entry["half"]["median_ms"], 3)
    ratios(entry)
    ok &= entry["same_as_torch_route"] and entry["plus_same_as_unstranded"] and entry["same_as_model"]
    result["letters"] = entry
    del out
    torch.cuda.empty_cache()

    # ---- base counts
    res = {}
    entry = {}

    def comp(name, st):
        def run():
            res[name] = sequence.composition_dev([track], track_of, short, short_end, strands=st)
        return run

    entry["unstranded"] = timed(comp("unstranded", None))
    for name, st in strands.items():
        entry[name] = timed(comp(name, st))
    swap = torch.tensor([3, 2, 1, 0, 4, 5], device="cuda")

    def comp_route():
        c = sequence.composition_dev([track], track_of, short, short_end)
        res["torch_route"] = torch.where(is_minus[:, None], c[:, swap], c)

    entry["torch_route"] = timed(comp_route, max(REPS // 3, 3), 1)
    entry["same_as_torch_route"] = bool((res["half"] == res["torch_route"]).all())
    entry["plus_same_as_unstranded"] = bool((res["plus"] == res["unstranded"]).all())
    got = res["minus"][:rows].cpu().numpy()
    entry["same_as_model"] = all(got[i].tolist() == B.counts_of(COMPLEMENT[B.window(seq, int(s), int(s) + WIDTH)]) for i, s in enumerate(short_h[:rows]))
    ratios(entry)
    ok &= entry["same_as_torch_route"] and entry["plus_same_as_unstranded"] and entry["same_as_model"]
    result["composition"] = entry
    res.clear()

    # ---- k-mers
    for k in KS:
        bins = 4 ** k
        out = {name: torch.empty((N, bins), dtype=torch.int32, device="cuda") for name in ("unstranded", "minus", "half", "plus")}
        rc = torch.from_numpy(kmers.strand_columns(k, "ACGT", False)).cuda()
        entry = {"bins": bins, "out_bytes": N * bins * 4}
        entry["unstranded"] = timed(lambda: kmers.count_matrix_dev([track], track_of, short, WIDTH, k, case_sensitive=False, out=out["unstranded"]))
        for name, st in strands.items():
            entry[name] = timed(lambda: kmers.count_matrix_dev([track], track_of, short, WIDTH, k, case_sensitive=False, out=out[name], strands=st))
        scratch = torch.empty((N, bins), dtype=torch.int32, device="cuda")

        def kmer_route():
            kmers.count_matrix_dev([track], track_of, short, WIDTH, k, case_sensitive=False, out=scratch)
            scratch[is_minus] = scratch[is_minus][:, rc]

        entry["torch_route"] = timed(kmer_route, max(REPS // 3, 3), 1)
        entry["same_as_torch_route"] = bool((out["half"] == scratch).all())
        entry["plus_same_as_unstranded"] = bool((out["plus"] == out["unstranded"]).all())
        entry["minus_is_the_gather_of_plus"] = bool((out["minus"] == out["unstranded"][:, rc]).all())
        entry["words_counted"] = int(out["minus"].sum(dtype=torch.int64))
        entry["torch_over_half"] = round(entry["torch_route"]["median_ms"] / entry["half"]["median_ms"], 3)
        ratios(entry)
        ok &= entry["same_as_torch_route"] and entry["plus_same_as_unstranded"] and entry["minus_is_the_gather_of_plus"]
        result["k%d" % k] = entry
        del out, scratch
        torch.cuda.empty_cache()

    # ---- one row of the whole sequence
    one, first = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (0, 0))
    m1, p1 = torch.ones(1, dtype=torch.int8, device="cuda"), torch.zeros(1, dtype=torch.int8, device="cuda")
    whole = {}
    out = torch.empty((1, SIZE), dtype=torch.uint8, device="cuda")
    entry = {"out_bytes": SIZE}
    entry["unstranded"] = timed(lambda: sequence.matrix_dev([track], one, first, SIZE, out=out), LONG_REPS, 1)
    entry["minus"] = timed(lambda: sequence.matrix_dev([track], one, first, SIZE, out=out, strands=m1), LONG_REPS, 1)
    tail = out[0, :4096].cpu().numpy()
    entry["same_as_model"] = bool(np.array_equal(tail, COMPLEMENT[B.window(seq, SIZE - 4096, SIZE)][::-1]))
    ok &= entry["same_as_model"]
    ratios(entry)
    whole["letters"] = entry
    del out
    torch.cuda.empty_cache()
    for k in (4, 7):
        bins = 4 ** k
        rc = torch.from_numpy(kmers.strand_columns(k, "ACGT", False)).cuda()
        outs = {name: torch.empty((1, bins), dtype=torch.int32, device="cuda") for name in ("unstranded", "minus")}
        entry = {"bins": bins}
        entry["unstranded"] = timed(lambda: kmers.count_matrix_dev([track], one, first, SIZE, k, case_sensitive=False, out=outs["unstranded"]), LONG_REPS, 1)
        entry["minus"] = timed(lambda: kmers.count_matrix_dev([track], one, first, SIZE, k, case_sensitive=False, out=outs["minus"], strands=m1), LONG_REPS, 1)
        entry["minus_is_the_gather_of_plus"] = bool((outs["minus"] == outs["unstranded"][:, rc]).all())
        ok &= entry["minus_is_the_gather_of_plus"]
        ratios(entry)
        whole["k%d" % k] = entry
    result["whole_sequence"] = whole
    del p1

    # ---- rows of 32 bases
    width = 32
    n_short = max(min(SHORT_BASES // width, 2_000_000), 1)
    rng = np.random.default_rng(15)
    starts = torch.from_numpy(rng.integers(0, SIZE - width, size=n_short).astype(np.int32)).cuda()
    which = torch.zeros(n_short, dtype=torch.int32, device="cuda")
    all_minus = torch.ones(n_short, dtype=torch.int8, device="cuda")
    mixed = torch.from_numpy(rng.integers(0, 2, n_short).astype(np.int8)).cuda()
    entry = {"rows": n_short, "width": width}
    out = torch.empty((n_short, width), dtype=torch.uint8, device="cuda")
    letters = {"unstranded": timed(lambda: sequence.matrix_dev([track], which, starts, width, out=out))}
    keep = out.clone()
    letters["minus"] = timed(lambda: sequence.matrix_dev([track], which, starts, width, out=out, strands=all_minus))
    letters["same_as_flip_and_lookup"] = bool((out == lookup[keep.flip(1).long()]).all())
    letters["half"] = timed(lambda: sequence.matrix_dev([track], which, starts, width, out=out, strands=mixed))
    ok &= letters["same_as_flip_and_lookup"]
    ratios(letters)
    entry["letters"] = letters
    del out, keep
    counts = torch.empty((n_short, 16), dtype=torch.int32, device="cuda")
    k2 = {"unstranded": timed(lambda: kmers.count_matrix_dev([track], which, starts, width, 2, case_sensitive=False, out=counts))}
    keep = counts.clone()
    k2["minus"] = timed(lambda: kmers.count_matrix_dev([track], which, starts, width, 2, case_sensitive=False, out=counts, strands=all_minus))
    k2["minus_is_the_gather_of_plus"] = bool((counts == keep[:, torch.from_numpy(kmers.strand_columns(2, "ACGT", False)).cuda()]).all())
    k2["half"] = timed(lambda: kmers.count_matrix_dev([track], which, starts, width, 2, case_sensitive=False, out=counts, strands=mixed))
    ok &= k2["minus_is_the_gather_of_plus"]
    ratios(k2)
    entry["k2"] = k2
    result["rows_of_32"] = entry

    print(json.dumps(result))
    track.close()
    if not ok:
        sys.exit("the routes differ: the times above measure a wrong result")


if __name__ == "__main__":
    main()
