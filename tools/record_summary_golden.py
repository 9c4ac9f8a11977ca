#!/usr/bin/env python
"""
Record what the reference computes for the cases of tests/golden/summary (run where a built reference is at hand; the engine is
not involved).  Per bigWig file and region: the five arrays of ``BigWigFile.summarize_from_full`` and the dicts of ``query``
(mean, max, min, coverage, std_dev), concatenated per file into two float64 .npy files of shape [5, bins]; manifest.json lists the
files, their zoom headers' reduction levels, the regions, where each region's bins lie in the arrays, and for every region whether
the reference's ``summarize`` -- and with it ``query`` -- takes a zoom level there (its own rule, bbi_file.pyx:205-215, 281-294,
applied to the ``level_list`` of the reference's object).  ``query`` is always the reference's own; for a region it would take from
a zoom level its object's ``level_list`` is emptied for that call, so that the answer comes from full data.

The bigWig files of tests/golden/profile are read in place; the small files defined below (`FIXTURES`) are written first, where
missing, with tools/write_bigwig_fixture.py's writer.  How the reference's modules are built: tools/record_profile_golden.py.

Also asserted here, on tests/summary_model.py: the straddling case can see the two mistakes that matter.  At least 64 of its bins
change when every  acc += value * weight  is one fused, exactly rounded multiply-add, and at least 64 change when the items are
walked in reverse order.

usage: record_summary_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
       record_summary_golden.py REFERENCE_LIB_DIR --time-reference [CALLS [WIDTH [BINS]]]

The second form records nothing: it times the reference's own loop, ``summarize_from_full`` once per site, over CALLS (default
5000) sites of WIDTH bases (default 200: test.bw's items are one base each, so a site meets about as many items as a site of
tools/bench_summary.py's default shape) and BINS bins (default 100) inside the data of tests/golden/profile/test.bw, and prints
one JSON line with the time per site and what 100 000 sites would take.  That is the figure DESIGN.md 3.9 holds against the device.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)

BEDGRAPH = 1
STRADDLE_SEED = 7
STRADDLE_CASE = ("chrS", 3, 40021, 1000)  # step 40, a remainder of 18 bases


def f32(x):
    return float(np.float32(x))


def straddle_items(seed=STRADDLE_SEED):
    """bedGraph items of length 2-40 laid out against the bins of STRADDLE_CASE (40 bases each, the first at 3).  Over every bin
    edge lies an item of n bases, a of them on one side, chosen among the ten (n, a) with n <= 40 whose weight n * (a / n) is NOT
    the integer a (22 * (15 / 22), ...); no n has such an a on both sides, so the side alternates from edge to edge and every
    second bin gets two such weights, one from each neighbour.  Shorter items fill the bins in between.  Values have 24 significant
    bits and one binary order of magnitude, so the sums carry and round."""
    rng = np.random.default_rng(seed)
    odd = sorted((n, a) for n in range(2, 41) for a in range(1, n) if n * (a / n) != a and a <= 15)
    assert len(odd) >= 6, odd
    _, first, _, _ = STRADDLE_CASE

    def value():
        return f32(rng.uniform(0.5, 2.0) * (1 if rng.random() < 0.7 else -1))

    items, at = [], None
    for k, edge in enumerate(range(first, first + 40 * 1001, 40)):
        n, a = odd[int(rng.integers(len(odd)))]
        begin = edge - (n - a) if k % 2 == 0 else edge - a  # the `a` bases lie right of an even edge, left of an odd one
        if begin < 0:
            continue
        if at is not None:  # fill [at, begin) with items of 2 bases or more
            gap = begin - at
            assert gap >= 2, gap
            while gap > 0:
                m = gap if gap < 4 else int(rng.integers(2, min(gap - 2, 14) + 1))
                items.append((at, at + m, value()))
                at, gap = at + m, gap - m
        items.append((begin, begin + n, value()))
        at = begin + n
    return items


def blocks_of(items, per_block=500):
    return [dict(chrom_id=0, kind=BEDGRAPH, items=items[k:k + per_block]) for k in range(0, len(items), per_block)]


# name -> (chromosomes, blocks): all little-endian, uncompressed, no zoom levels
FIXTURES = {
    "straddle.bw": ([("chrS", 50000)], blocks_of(straddle_items())),
    # values whose float32 square is not their float64 square
    "sq.bw": ([("chrQ", 200)], blocks_of([(2, 9, f32(0.1)), (9, 30, f32(1.1)), (30, 31, f32(3.3)), (35, 60, f32(-2.7)), (60, 100, f32(1e-3)),
                                         (100, 101, f32(16777215.0)), (101, 150, f32(1.0 / 3.0))])),
    # absorption, and a float32 square that overflows
    "big.bw": ([("chrG", 100)], blocks_of([(0, 10, f32(1e30)), (10, 20, 1.0), (20, 30, f32(-1e30)), (40, 45, 2.0), (45, 50, f32(1e20))])),
    "nan.bw": ([("chrN", 100)], blocks_of([(0, 5, 1.0), (5, 9, float("nan")), (9, 20, 2.5), (30, 40, -1.0), (40, 44, float("nan"))])),
    # NOT ordered: overlapping and out-of-order items (each block's first item has its smallest start, which is what the writer
    # takes for the block's extent)
    "unordered.bw": ([("chrU", 300)], [
        dict(chrom_id=0, kind=BEDGRAPH, items=[(0, 50, 1.5), (30, 45, f32(0.3)), (10, 20, -2.0), (40, 100, f32(0.7)), (5, 60, 4.0), (90, 95, f32(1e-3)),
                                               (70, 80, f32(-0.1))]),
        dict(chrom_id=0, kind=BEDGRAPH, items=[(60, 130, f32(2.2)), (200, 260, 8.0), (120, 210, f32(0.9)), (100, 101, -5.0), (250, 300, f32(0.6))]),
    ]),
}

PROFILE = "../profile/"
# file (relative to the golden directory) -> regions (chrom, start, end, size)
REGIONS = {
    PROFILE + "bg.bw": [("chr1", 0, 400, 1), ("chr1", 0, 400, 10), ("chr1", 0, 400, 7), ("chr1", 5, 33, 4), ("chr1", 120, 131, 20),
                        ("chr1", 395, 450, 5), ("chr1", 140, 200, 3), ("chr1", 3, 10, 1), ("chr1", 72, 128, 8), ("chr1", 300, 390, 4),
                        ("chr1", 25, 38, 13), ("chr1", 0, 3, 2), ("chr1", 400, 500, 4), ("chr1", 10, 10, 3), ("chr1", 20, 10, 3),
                        ("chrNone", 0, 100, 5)],
    PROFILE + "bg.z.bw": [("chr1", 0, 400, 16), ("chr1", 28, 37, 3)],
    PROFILE + "fs.bw": [("chrF", 0, 250, 25), ("chrF", 98, 112, 5), ("chrF", 150, 166, 3), ("chrF", 7, 71, 64), ("chrF", 6, 73, 65)],
    PROFILE + "fs.z.bw": [("chrF", 0, 250, 9)],
    PROFILE + "two.z.bw": [("chrA", 0, 100, 10), ("chrBB", 0, 50, 7), ("chrA", 18, 62, 5), ("chrBB", 40, 60, 4), ("chrC", 0, 10, 2)],
    PROFILE + "two.be.bw": [("chrA", 0, 100, 3), ("chrBB", 0, 50, 50)],
    # the reference's own file: test_get_leaf's two queries; a region served from full data (step 22: 11 < the first reduction
    # level, 20); regions the reference takes from a zoom level; before, across the end of and after the data
    PROFILE + "test.bw": [("chr1", 11000, 11005, 5), ("chr1", 11000, 11005, 1), ("chr1", 10000, 21000, 500), ("chr1", 10000, 21000, 100),
                          ("chr1", 10900, 11700, 10), ("chr1", 0, 64, 4), ("chr1", 20800, 21200, 8), ("chr1", 30000, 31000, 10),
                          ("chr1", 10917, 10919, 1), ("chr2", 0, 10000, 10)],
    "straddle.bw": [STRADDLE_CASE, ("chrS", 0, 50000, 200), ("chrS", 100, 7300, 199), ("chrS", 17, 1017, 65), ("chrS", 39000, 41000, 64),
                    ("chrS", 5, 6, 1), ("chrS", 2000, 2100, 100), ("chrS", 2000, 2100, 101)],
    "sq.bw": [("chrQ", 0, 200, 1), ("chrQ", 0, 160, 16), ("chrQ", 5, 149, 12), ("chrQ", 99, 102, 3)],
    "big.bw": [("chrG", 0, 30, 1), ("chrG", 0, 100, 2), ("chrG", 0, 50, 5), ("chrG", 5, 25, 1), ("chrG", 38, 50, 2)],
    "nan.bw": [("chrN", 0, 100, 1), ("chrN", 0, 48, 6), ("chrN", 4, 10, 3), ("chrN", 9, 40, 2), ("chrN", 40, 44, 2)],
    "unordered.bw": [("chrU", 0, 300, 1), ("chrU", 0, 300, 10), ("chrU", 0, 300, 64), ("chrU", 25, 215, 7), ("chrU", 95, 125, 30),
                     ("chrU", 130, 200, 2), ("chrU", 44, 45, 1)],
}


def check_straddle():
    import summary_model as M

    starts, ends, values = (np.array(c) for c in zip(*straddle_items()))
    track = (starts.astype(np.int32), ends.astype(np.int32), values.astype(np.float32))
    _, s, e, size = STRADDLE_CASE
    plain = M.summarize_region(track, s, e, size)
    changed = {}
    for name, how in (("fused", dict(fused=True)), ("reversed", dict(reverse=True))):
        other = M.summarize_region(track, s, e, size, **how)
        changed[name] = sum(1 for j in range(size) if any(plain[p][j] != other[p][j] for p in (3, 4)))
    print("straddling case: %d of %d bins change when fused, %d when reversed" % (changed["fused"], size, changed["reversed"]))
    assert changed["fused"] >= 64 and changed["reversed"] >= 64, "the straddling case cannot see a fused or a reversed chain"
    return changed


def main(libdir, golden=os.path.join(HERE, "..", "tests", "golden", "summary")):
    import summary_model as M
    import write_bigwig_fixture as W

    os.makedirs(golden, exist_ok=True)
    for name, (chroms, blocks) in FIXTURES.items():
        path = os.path.join(golden, name)
        if not os.path.exists(path):
            W.write_bigwig(path, chroms, blocks)
            print("wrote", path)
    changed = check_straddle()
    sys.path.insert(0, libdir)
    from bx.bbi.bigwig_file import BigWigFile

    manifest = {"straddle": {"file": "straddle.bw", "region": list(STRADDLE_CASE), "bins_changed_when_fused": changed["fused"],
                             "bins_changed_when_reversed": changed["reversed"]}, "files": []}
    for rel, regions in REGIONS.items():
        stem = os.path.basename(rel)
        planes, queries, cases, at = [], [], [], 0
        with open(os.path.join(golden, rel), "rb") as f, np.errstate(all="ignore"):
            bw = BigWigFile(f)
            levels = bw.level_list
            reductions = [int(level.reduction_level) for level in levels]
            for chrom, start, end, size in regions:
                sd = bw.summarize_from_full(chrom.encode(), start, end, size)
                zoom = sd is not None and M.picks_zoom(reductions, start, end, size)
                if sd is None:
                    assert bw.query(chrom, start, end, size) is None
                    cases.append({"chrom": chrom, "start": start, "end": end, "size": size, "none": True, "zoom": False})
                    continue
                sd_planes = [getattr(sd, p) for p in M.PLANES]
                if zoom:  # the reference's own query, made to go to full data: its object's list of zoom levels emptied for the call
                    bw.level_list = []
                own = bw.query(chrom, start, end, size)
                bw.level_list = levels
                q = [[float(row[k]) for row in own] for k in M.QUERY_KEYS]
                # (the model's derivation, which the tests use, equals it bit for bit)
                assert all(M.same_bits(a, b) for a, b in zip(q, M.query_region(sd_planes, start, end, size))), (rel, chrom, start, end)
                planes.append(np.array(sd_planes, dtype=np.float64))
                queries.append(np.array(q, dtype=np.float64))
                cases.append({"chrom": chrom, "start": start, "end": end, "size": size, "none": False, "zoom": bool(zoom), "at": at})
                at += size
        np.save(os.path.join(golden, stem + ".planes.npy"), np.concatenate(planes, axis=1))
        np.save(os.path.join(golden, stem + ".query.npy"), np.concatenate(queries, axis=1))
        manifest["files"].append({"file": rel, "reductions": reductions, "planes": stem + ".planes.npy", "query": stem + ".query.npy", "cases": cases})
        print(rel, len(cases), "regions,", at, "bins,", sum(c["zoom"] for c in cases), "of them zoom-level regions")
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


def time_reference(libdir, calls=5000, width=200, bins=100):
    import time

    calls, width, bins = int(calls), int(width), int(bins)
    sys.path.insert(0, libdir)
    from bx.bbi.bigwig_file import BigWigFile

    rng = np.random.default_rng(3)
    path = os.path.join(HERE, "..", "tests", "golden", "profile", "test.bw")
    starts = rng.integers(10920, 20900 - width, size=calls)
    with open(path, "rb") as f:
        bw = BigWigFile(f)
        items = sum(len(bw.get(b"chr1", int(s), int(s) + width)) for s in starts[:50]) / 50.0
        t0 = time.perf_counter()
        for s in starts:
            bw.summarize_from_full(b"chr1", int(s), int(s) + width, bins)
        sec = time.perf_counter() - t0
    print(json.dumps({"calls": calls, "width": width, "bins": bins, "items_per_site": round(items, 1), "seconds": round(sec, 3),
                      "us_per_site": round(sec / calls * 1e6, 1), "seconds_per_100k_sites": round(sec / calls * 1e5, 1)}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--time-reference":
        time_reference(sys.argv[1], *sys.argv[3:])
    else:
        main(*sys.argv[1:])
