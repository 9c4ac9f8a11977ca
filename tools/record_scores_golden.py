#!/usr/bin/env python
"""
Record what the reference's scripts/aggregate_scores_in_intervals.py prints for the cases of tests/golden/scores (run where
a built reference is at hand; the engine is not involved).  The inputs are committed data: a hand-written case and a seeded
synthetic one; where an input file is missing it is written first (the generators below are their definition).  Large inputs
are stored gzipped and unpacked into a scratch directory for the reference, which reads plain text only.
manifest.json lists, per case, its inputs and the file that holds the recorded standard output.

The synthetic case must be able to tell an ordered float32 chain from any other summation: at least half of its non-empty
intervals have an ordered sum that differs from both the rounded float64 sum and numpy's pairwise float32 sum (asserted here
and again by tests/test_scores_model_golden.py).

usage: record_scores_golden.py AGGREGATE_SCORES_PY REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

# (expectation, scores, intervals, mask or None)
CASES = [
    ("hand.out", "hand.wig", "hand.bed", None),
    ("hand.masked.out", "hand.wig", "hand.bed", "hand.mask.bed"),
    ("syn.out", "syn.wig.gz", "syn.bed", None),
    ("syn.masked.out", "syn.wig.gz", "syn.bed", "syn.mask.bed"),
]

HAND_WIG = """\
track type=wiggle_0 name=hand
# bed-style lines: zeros of both signs and a nan are stored but never counted
chr1\t0\t5\t1.5
chr1\t5\t8\t0.0
chr1\t8\t10\t-0.0
chr1\t10\t12\tnan
chr1\t12\t14\t-2.25\tname\t-
chr1\t1\t2

browser position chr1:1-100
variableStep chrom=chr1 span=3
21\t2.0
22\t3.0
24\t4.0
31\t1.0000000596046447754
fixedStep chrom=chr1 start=41 step=2 span=1
0.5
0.25
0.25
fixedStep chrom=chr1 start=61 step=3 span=2
0.1
0.2
0.3
variableStep chrom=chr2
1\t200000000
2\t300000000
5\t-200000000
6\t-300000000
7\t5
8\t100000000
9\t-100000000
fixedStep chrom=chr3 start=1 step=1
1e-45
3e-39
-1e-40
inf
1
-inf
"""

HAND_BED = """\
chr1\t0\t14
chr1\t0\t5
chr1\t5\t12
chr1\t20\t26
chr1\t20\t22
chr1\t30\t31
chr1\t40\t46
chr1\t60\t70
chr1\t100\t200
chr1\t7\t7
chr1\t12\t10
chrUn\t0\t10
chr2\t0\t2
chr2\t4\t6
chr2\t0\t7
chr2\t7\t8
chr2\t8\t9
chr2\t0\t9
chr3\t0\t3
chr3\t0\t4
chr3\t0\t5
chr3\t0\t6
chr3\t5\t6
chr1\t0\t1000\textra\tcolumns
"""

HAND_MASK = """\
# mask
chr1\t0\t3
chr1\t21\t22
chr1\t42\t43
chr2\t1\t2
chr3\t3\t4
chrOther\t0\t100
"""

SYN_SIZES = (("chrA", 50000), ("chrB", 20011))
SYN_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1000, 4095, 4096, 4097)


def synthetic(seed=20240611):
    """(wiggle text, interval text, mask text) of the synthetic case"""
    rng = np.random.default_rng(seed)
    wig, bed, mask = [], [], []
    for chrom, size in SYN_SIZES:
        scale = rng.choice(np.array([1e-3, 1.0, 1e4]), size=size)
        v = (rng.standard_normal(size) * scale).astype(np.float32)
        kind = rng.random(size)
        v[kind < 0.01] = (rng.integers(-5000, 5000, size=int((kind < 0.01).sum())) * 1e-42).astype(np.float32)  # denormals
        v[(kind >= 0.01) & (kind < 0.06)] = 0.0
        nan = (kind >= 0.06) & (kind < 0.26)
        written_nan = nan & (rng.random(size) < 0.5)  # half of the missing scores are `nan` lines, half are left out
        # runs of written positions as fixedStep blocks
        present = ~nan | written_nan
        p = 0
        while p < size:
            if not present[p]:
                p += 1
                continue
            q = p
            while q < size and present[q]:
                q += 1
            wig.append("fixedStep chrom=%s start=%d step=1\n" % (chrom, p + 1))
            wig.extend("nan\n" if nan[i] else repr(float(v[i])) + "\n" for i in range(p, q))
            p = q
        # intervals: every listed length at every residue of the start mod 64, unsorted, with duplicates, one over everything
        rows = []
        for k in range(300 if chrom == "chrA" else 290):
            ln = SYN_LENGTHS[k % len(SYN_LENGTHS)]
            s = int(rng.integers(0, (size - ln) // 64)) * 64 + k % 64
            rows.append((s, min(s + ln, size)))
        rows += [rows[3], rows[17], rows[100], (0, size), (size - 70, size + 500)]
        for j in rng.permutation(len(rows)):
            bed.append("%s\t%d\t%d\n" % (chrom, rows[j][0], rows[j][1]))
        # mask runs that begin and end on 64-bit word edges and one bit either side of them
        word = 0
        for k in range(size // 700):
            gap, run = int(rng.integers(1, 6)), int(rng.integers(1, 5))
            a = 64 * (word + gap) + (-1, 0, 1)[k % 3]
            b = 64 * (word + gap + run) + (-1, 0, 1)[(k // 3) % 3]
            if b >= size:
                break
            mask.append("%s\t%d\t%d\n" % (chrom, a, b))
            word += gap + run + 1
    order = np.random.default_rng(seed + 1).permutation(len(bed))
    return "".join(wig), "".join(bed[j] for j in order), "".join(mask)


def write_inputs(golden):
    os.makedirs(golden, exist_ok=True)
    texts = {"hand.wig": HAND_WIG, "hand.bed": HAND_BED, "hand.mask.bed": HAND_MASK}
    if not all(os.path.exists(os.path.join(golden, n)) for n in ("syn.wig.gz", "syn.bed", "syn.mask.bed")):
        texts["syn.wig.gz"], texts["syn.bed"], texts["syn.mask.bed"] = synthetic()
    for name, text in texts.items():
        path = os.path.join(golden, name)
        if os.path.exists(path):
            continue
        if name.endswith(".gz"):
            with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
                f.write(text.encode())
        else:
            with open(path, "w") as f:
                f.write(text)


def check_order_sensitive(golden):
    import scores_model as M

    with M.open_text(os.path.join(golden, "syn.wig.gz")) as f:
        tracks = M.load_wiggle(f)
    rows = [line.split() for line in open(os.path.join(golden, "syn.bed"))]
    worst = 1.0
    for chrom, track in tracks.items():
        mine = [(int(r[1]), int(r[2])) for r in rows if r[0] == chrom]
        frac = M.fraction_order_sensitive(track, [s for s, _ in mine], [e for _, e in mine])
        print("%s: %.0f %% of the non-empty intervals are order-sensitive" % (chrom, 100 * frac))
        worst = min(worst, frac)
    assert worst >= 0.5, "the synthetic case cannot tell an ordered chain from a reduction tree"


def main(script, libdir, golden=os.path.join(HERE, "..", "tests", "golden", "scores")):
    write_inputs(golden)
    check_order_sensitive(golden)
    env = dict(os.environ, PYTHONPATH=libdir)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        def plain(name):
            if name is None:
                return None
            if name.endswith(".gz"):
                dst = os.path.join(tmp, name[:-3])
                if not os.path.exists(dst):
                    with gzip.open(os.path.join(golden, name), "rb") as src, open(dst, "wb") as out:
                        out.write(src.read())
                return dst
            if not os.path.exists(os.path.join(tmp, name)):
                shutil.copy(os.path.join(golden, name), tmp)
            return os.path.join(tmp, name)

        for expect, wig, bed, mask in CASES:
            cmd = [sys.executable, script, plain(wig), plain(bed)] + (["-m", plain(mask)] if mask else [])
            out = subprocess.run(cmd, check=True, env=env, stdout=subprocess.PIPE).stdout
            with open(os.path.join(golden, expect), "wb") as f:
                f.write(out)
            manifest.append({"expected": expect, "scores": wig, "intervals": bed, "mask": mask, "lines": out.count(b"\n")})
            print(expect, out.count(b"\n"))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in manifest) + "\n]\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
