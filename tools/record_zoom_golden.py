#!/usr/bin/env python
"""
Record what the reference computes for the cases of tests/golden/zoom (run where a built reference is at hand; the engine is not
involved).  Per bigWig file and region: the five arrays of ``BigWigFile.summarize`` -- the reference's own choice between a zoom
level and the full data -- and the dicts of ``query`` (mean, max, min, coverage, std_dev), concatenated per file into two float64
.npy files of shape [5, bins]; manifest.json lists the files, their reduction levels in file order, the regions, where each
region's bins lie in the arrays and the level the reference's rule picks for it (an index into the file's levels, or null for
full data).  The reference's ``_best_zoom_level`` cannot be called from Python; the recorded index is tests/zoom_model.py's
restatement of it, and every recorded array is asserted to equal the model's answer FROM THAT LEVEL bit for bit -- the fixture
files' levels disagree with each other and with their full data, so this is a statement about the reference's choice as well.

The reference's own test file is read in place (tests/golden/profile/test.bw) and its test.expectation is copied beside the
results as data; the small files come from tools/write_bigwig_zoom_fixture.py (written first where missing).  How the reference's
modules are built: tools/record_profile_golden.py.

WHICH ROUNDINGS the reference's  acc += field * overlap_factor  performs is decided here, by the built reference: the model is
run under both readings of tests/zoom_model.py over every recorded zoom bin, the one that reproduces every bit is written into
the manifest ("reading"), and the other one must differ in at least 64 bins.  Also asserted, on the model: at least 64 recorded
bins change when a bin's records are accumulated in reverse order, at least 16 have valid_count == 0 with a min that is not NaN
(a front record that does not overlap its bin), at least 16 are NaN in min and max (no record left).

usage: record_zoom_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR [REFERENCE_ROOT]]
(REFERENCE_ROOT holds test_data/; default: the parent of REFERENCE_LIB_DIR)
"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, "..", "bx-python_amd"))
sys.path.insert(0, HERE)

PROFILE = "../profile/"
# file (relative to the golden directory) -> regions (chrom, start, end, size)
REGIONS = {
    # the reference's own queries (bigwig_tests.py:29-71); levels 20, 80, 320 and 20480; before, across the end of and after the data
    PROFILE + "test.bw": [("chr1", 10000, 20000, 10), ("chr1", 10000, 20000, 1), ("chr1", 11000, 11005, 5), ("chr1", 11000, 11005, 1),
                          ("chr1", 10000, 21000, 100), ("chr1", 0, 64000, 64), ("chr1", 9000, 22000, 65), ("chr1", 10000, 20000, 200),
                          ("chr1", 30000, 40000, 10), ("chr1", 0, 5000, 5), ("chr1", 20000, 30000, 20), ("chr1", 0, 247000000, 2),
                          ("chr1", 10917, 21157, 2), ("chr2", 0, 10000, 10)],
    # before the first leaf (both levels), after the last, across the end, over the gaps; full-data rows; rows the reference
    # answers with None
    "leaves.bw": [("chrL", 0, 900, 2), ("chrL", 0, 640, 10), ("chrL", 15000, 19992, 64), ("chrL", 12000, 15000, 60), ("chrL", 1000, 14000, 200),
                  ("chrL", 900, 7556, 65), ("chrL", 1000, 5096, 64), ("chrL", 1100, 1140, 1), ("chrL", 2000, 2100, 2), ("chrL", 0, 20000, 1),
                  ("chrL", 1300, 2900, 40), ("chrL", 2500, 7000, 100), ("chrL", 960, 20000, 64), ("chrL", 1000, 1400, 100), ("chrL", 2990, 3070, 8),
                  ("chrNone", 0, 100, 4), ("chrL", 500, 500, 3), ("chrL", 700, 600, 3), ("chrL", 8000, 2147483647, 2)],
    "chroms.bw": [("chrA", 0, 256, 8), ("chrB", 0, 400, 2), ("chrB", 90, 300, 10), ("chrC", 0, 600, 30), ("chrC", 0, 600, 1), ("chrA", 300, 400, 4),
                  ("chrB", 0, 64, 2), ("chrC", 0, 2080, 65), ("chrC", 0, 130, 65), ("chrA", 0, 128, 64), ("chrA", 60, 160, 5), ("chrC", 150, 470, 16),
                  ("chrB", 100, 1380, 64), ("chrA", 250, 250, 2)],
    "odd.bw": [("chrO", 0, 160, 8), ("chrO", 0, 62, 2), ("chrO", 0, 480, 16), ("chrO", 3, 157, 7), ("chrO", 0, 500, 1), ("chrO", 0, 500, 5),
               ("chrO", 90, 170, 3), ("chrO", 30, 160, 1), ("chrO", 25, 165, 2), ("chrO", 0, 13000, 200), ("chrO", 200, 1480, 64), ("chrO", 5, 1045, 50),
               ("chrO", 0, 100, 10)],
}


def model_row(M, levels, spans, case):
    """the model's five lists for a recorded case, under M.READING unless `how` says otherwise"""
    def run(**how):
        chrom, start, end, size, level = (case[k] for k in ("chrom", "start", "end", "size", "level"))
        if level is None:
            import summary_model as S

            return S.summarize_region(spans[chrom], start, end, size)
        return M.summarize_region(levels[level][1][chrom], start, end, size, **how)
    return run


def main(libdir, golden=os.path.join(HERE, "..", "tests", "golden", "zoom"), root=None):
    import write_bigwig_zoom_fixture as W
    import zoom_model as M
    from bxmi import bigwig

    root = root or os.path.dirname(os.path.abspath(libdir))
    W.main(golden)
    shutil.copyfile(os.path.join(root, "test_data", "bbi_tests", "test.expectation"), os.path.join(golden, "test.expectation"))
    sys.path.insert(0, libdir)
    from bx.bbi.bigwig_file import BigWigFile

    manifest = {"files": []}
    seen = {"bins": 0, "other_reading": 0, "reversed": 0, "front_only": 0, "all_nan": 0}
    matches = {"a": True, "b": True}
    for rel, regions in REGIONS.items():
        stem = os.path.basename(rel)
        path = os.path.join(golden, rel)
        levels, spans = bigwig.read_zoom_file(path), bigwig.read_spans_file(path)
        reductions = [r for r, _ in levels]
        planes, queries, cases, at = [], [], [], 0
        with open(path, "rb") as f, np.errstate(all="ignore"):
            bw = BigWigFile(f)
            assert [int(level.reduction_level) for level in bw.level_list] == reductions
            for chrom, start, end, size in regions:
                sd = bw.summarize(chrom, start, end, size)
                case = {"chrom": chrom, "start": start, "end": end, "size": size, "none": sd is None, "level": None}
                if sd is None:
                    assert bw.query(chrom, start, end, size) is None
                    cases.append(case)
                    continue
                case["level"] = M.pick_level(reductions, start, end, size)
                case["at"] = at
                want = [np.asarray(getattr(sd, p)) for p in M.PLANES]
                run = model_row(M, levels, spans, case)
                if case["level"] is None:
                    assert all(M.same_bits(a, b) for a, b in zip(run(), want)), (rel, case)
                else:
                    a, b = run(reading="a"), run(reading="b")
                    for name, got in (("a", a), ("b", b)):
                        matches[name] = matches[name] and all(M.same_bits(x, y) for x, y in zip(got, want))
                    back = run(reverse=True)
                    mine = run()
                    for j in range(size):
                        seen["bins"] += 1
                        seen["other_reading"] += any(not M.same_bits(a[p][j], b[p][j]) for p in range(5))
                        seen["reversed"] += any(not M.same_bits(mine[p][j], back[p][j]) for p in range(5))
                        seen["front_only"] += mine[0][j] == 0 and not np.isnan(mine[1][j])
                        seen["all_nan"] += bool(np.isnan(mine[1][j]) and np.isnan(mine[2][j]) and mine[0][j] == 0)
                own = bw.query(chrom, start, end, size)
                q = [[float(row[k]) for row in own] for k in M.QUERY_KEYS]
                assert all(M.same_bits(x, y) for x, y in zip(q, M.query_region(want, start, end, size))), (rel, case)
                planes.append(np.array(want, dtype=np.float64))
                queries.append(np.array(q, dtype=np.float64))
                cases.append(case)
                at += size
        np.save(os.path.join(golden, stem + ".planes.npy"), np.concatenate(planes, axis=1))
        np.save(os.path.join(golden, stem + ".query.npy"), np.concatenate(queries, axis=1))
        manifest["files"].append({"file": rel, "reductions": reductions, "planes": stem + ".planes.npy", "query": stem + ".query.npy", "cases": cases})
        print(rel, len(cases), "regions,", at, "bins,", sum(c["level"] is not None for c in cases), "of them zoom-level regions")
    print("readings that reproduce every recorded bit:", matches, "--", seen)
    assert matches["a"] != matches["b"], "the recorded results do not decide between the two readings"
    reading = "a" if matches["a"] else "b"
    assert reading == M.READING, "tests/zoom_model.py assumes reading %r; the built reference performs %r" % (M.READING, reading)
    assert seen["other_reading"] >= 64 and seen["reversed"] >= 64 and seen["front_only"] >= 16 and seen["all_nan"] >= 16, seen
    manifest["reading"] = reading
    manifest["seen"] = {k: int(v) for k, v in seen.items()}
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
