#!/usr/bin/env python
"""
Record what the reference computes for the cases of tests/golden/bigbed (run where a built reference is at hand; the engine is
not involved).  Per bigBed file and region, from the reference's own ``BigBedFile``: the five arrays of ``summarize_from_full``
(``X.planes.npy``, float64 [5, bins]), those of ``summarize`` (``X.summarize.npy``: from the zoom level its rule picks, else the
same as from full data) and the dicts of ``query`` (``X.query.npy``: mean, max, min, coverage, std_dev), concatenated per file;
per file and region of `GETS`, what ``get`` returns (chrom, start, end, strand, fields of every GenomicInterval).  manifest.json
lists the files, their chromosomes and reduction levels, the regions, where each region's bins lie in the arrays, the zoom level
the reference takes for it (its own rule, applied to the ``level_list`` of its object; null for full data), the regions where it
answers None, and the types ``query`` returns.  ``summarize_from_full`` and ``get`` take ``char *chrom`` (bytes; str raises
TypeError, recorded as such), ``summarize`` and ``query`` take str.

The files are written first, where missing, by tools/write_bigbed_fixture.py.  The reference's modules are built by the recipe
in tools/record_profile_golden.py's docstring, with "bx.bbi.bigbed_file" added to `names`.

Also asserted here, on tests/summary_model.py with values of 1: the model gives every recorded from-full array bit for bit, and
the straddle case can see a wrong order: at least 32 of its bins change when the chain is walked in reverse.

usage: record_bigbed_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, "..", "bx-python_amd"))
sys.path.insert(0, HERE)

import write_bigbed_fixture as W  # noqa: E402

GENES = [("chrA", 0, 2000, 1), ("chrA", 0, 2000, 10), ("chrA", 100, 1000, 7), ("chrA", 120, 131, 11), ("chrA", 119, 401, 64), ("chrA", 124, 126, 2),
         ("chrA", 125, 126, 1), ("chrA", 630, 660, 3), ("chrA", 1490, 1810, 5), ("chrA", 0, 100, 4), ("chrA", 1900, 2000, 2), ("chrA", 130, 140, 20),
         ("chrBB", 0, 400, 8), ("chrBB", 0, 65, 65), ("chrBB", 26, 63, 3), ("chrBB", 300, 400, 2), ("chrA", 10, 10, 3), ("chrA", 20, 10, 3),
         ("chrNone", 0, 100, 5)]
# file -> regions (chrom, start, end, size)
REGIONS = {
    "genes.bb": GENES,
    "genes.z.bb": GENES[:6],
    "genes.be.bb": GENES[:6] + GENES[12:15],
    "hand.bb": [("chrA", 3, 63, 4), ("chrB", 3, 63, 4), ("chrA", 0, 1000, 1), ("chrB", 0, 100, 10)],
    "straddle.bb": [W.STRADDLE_CASE, ("chrS", 0, 50000, 200), ("chrS", 100, 7300, 199), ("chrS", 17, 1017, 65), ("chrS", 39000, 41000, 64),
                    ("chrS", 5, 6, 1), ("chrS", 2000, 2126, 63), ("chrS", 2000, 2101, 101), ("chrS", 3, 10083, 3)],
    "long.bb": [("chrL", 0, 200000, 100), ("chrL", 0, 200000, 1), ("chrL", 7000, 9000, 64), ("chrL", 30000, 34000, 200), ("chrL", 38000, 38130, 65),
                ("chrL", 60000, 62000, 2), ("chrL", 199000, 200000, 3), ("chrL", 20000, 28000, 63)],
    # desired reduction = ((end - start) // size) // 2: full data (desired 1 and 15), the first level (16 .. 63), the second (>= 64)
    "zoom.bb": [("chrZ", 1000, 1300, 100), ("chrZ", 900, 4000, 100), ("chrZ", 1000, 4200, 100), ("chrZ", 0, 20000, 100), ("chrZ", 0, 20000, 65),
                ("chrZ", 960, 12000, 64), ("chrZ", 1000, 9000, 200), ("chrZ", 2500, 2900, 1), ("chrZ", 8000, 8128, 1), ("chrY", 0, 700, 2),
                ("chrY", 0, 700, 20), ("chrY", 40, 200, 5), ("chrZ", 5000, 5000, 4), ("chrNone", 0, 10000, 10)],
}
# file -> regions (chrom, start, end) of `get`
GETS = {
    "genes.bb": [("chrA", 0, 2000), ("chrA", 124, 126), ("chrA", 125, 126), ("chrA", 125, 125), ("chrA", 131, 200), ("chrA", 640, 650), ("chrA", 1522, 1523),
                 ("chrBB", 0, 400), ("chrBB", 62, 280), ("chrBB", 27, 41), ("chrA", 30, 20), ("chrNone", 0, 10)],
    "genes.be.bb": [("chrA", 0, 2000), ("chrBB", 0, 400)],
    "genes.z.bb": [("chrA", 0, 2000), ("chrBB", 0, 400)],
    "hand.bb": [("chrA", 0, 1000), ("chrB", 0, 100), ("chrA", 6, 8)],
    "long.bb": [("chrL", 100, 200)],
}
PLANES = ("valid_count", "min_val", "max_val", "sum_data", "sum_squares")
QUERY_KEYS = ("mean", "max", "min", "coverage", "std_dev")


def ones_track(items):
    s, e, _ = items
    return s, e, np.ones(len(s), dtype=np.float32)


def check_straddle(golden):
    import summary_model as M
    from bxmi import bigbed

    track = ones_track(bigbed.read_items_file(os.path.join(golden, "straddle.bb"))["chrS"])
    _, s, e, size = W.STRADDLE_CASE
    plain, other = M.summarize_region(track, s, e, size), M.summarize_region(track, s, e, size, reverse=True)
    changed = sum(1 for j in range(size) if plain[3][j] != other[3][j])
    depth = [int(((track[0] < s + 40 * (j + 1)) & (track[1] > s + 40 * j)).sum()) for j in range(size)]
    print("straddle case: %d of %d bins change when reversed; %d - %d records per bin" % (changed, size, min(depth), max(depth)))
    assert changed >= 32, "the straddle case cannot see a reversed chain"
    return changed


def main(libdir, golden=os.path.join(HERE, "..", "tests", "golden", "bigbed")):
    import summary_model as M
    from bxmi import bigbed

    W.main(golden)
    changed = check_straddle(golden)
    sys.path.insert(0, libdir)
    from bx.bbi.bigbed_file import BigBedFile

    manifest = {"straddle": {"file": "straddle.bb", "region": list(W.STRADDLE_CASE), "bins_changed_when_reversed": changed}, "files": []}
    for name, regions in REGIONS.items():
        path = os.path.join(golden, name)
        items = bigbed.read_items_file(path)
        full, picked, queries, cases, gets, at = [], [], [], [], [], 0
        with open(path, "rb") as f, np.errstate(all="ignore"):
            bb = BigBedFile(f)
            reductions = [int(level.reduction_level) for level in bb.level_list]
            for chrom, start, end, size in regions:
                sd = bb.summarize_from_full(chrom.encode(), start, end, size)
                if sd is None:
                    assert bb.summarize(chrom, start, end, size) is None and bb.query(chrom, start, end, size) is None
                    cases.append({"chrom": chrom, "start": start, "end": end, "size": size, "none": True, "level": None})
                    continue
                desired = ((end - start) // size) // 2
                level = None
                if desired > 1:
                    diffs = [(desired - r, k) for k, r in enumerate(reductions) if desired - r >= 0]
                    level = min(diffs)[1] if diffs else None
                sm, own = bb.summarize(chrom, start, end, size), bb.query(chrom, start, end, size)
                sd_planes, sm_planes = [np.array(getattr(sd, p)) for p in PLANES], [np.array(getattr(sm, p)) for p in PLANES]
                # (the model, which the tests use, equals the reference's from-full arrays bit for bit)
                assert all(M.same_bits(a, b) for a, b in zip(sd_planes, M.summarize_region(ones_track(items[chrom]), start, end, size))), (name, chrom, start, end)
                if level is None:
                    assert all(M.same_bits(a, b) for a, b in zip(sd_planes, sm_planes)), (name, chrom, start, end)
                types = sorted({"%s:%s" % (k, type(row[k]).__name__) for row in own for k in QUERY_KEYS})
                full.append(np.array(sd_planes, dtype=np.float64))
                picked.append(np.array(sm_planes, dtype=np.float64))
                queries.append(np.array([[float(row[k]) for row in own] for k in QUERY_KEYS], dtype=np.float64))
                cases.append({"chrom": chrom, "start": start, "end": end, "size": size, "none": False, "level": level, "at": at, "query_types": types})
                at += size
            str_chrom = {}
            for method, args in (("summarize_from_full", ("chrA", 0, 10, 1)), ("get", ("chrA", 0, 10))):
                try:
                    getattr(bb, method)(*args)
                    str_chrom[method] = "accepted"
                except TypeError:
                    str_chrom[method] = "TypeError"
            for chrom, start, end in GETS.get(name, []):
                got = bb.get(chrom.encode(), start, end)
                rows = None if got is None else [{"chrom": repr(iv.chrom), "start": iv.start, "end": iv.end, "strand": iv.strand,
                                                   "fields": [x if isinstance(x, str) else repr(x) for x in iv.fields]} for iv in got]
                gets.append({"chrom": chrom, "start": start, "end": end, "rows": rows})
        np.save(os.path.join(golden, name + ".planes.npy"), np.concatenate(full, axis=1))
        np.save(os.path.join(golden, name + ".summarize.npy"), np.concatenate(picked, axis=1))
        np.save(os.path.join(golden, name + ".query.npy"), np.concatenate(queries, axis=1))
        manifest["files"].append({"file": name, "chroms": bigbed.chroms(path), "reductions": reductions, "planes": name + ".planes.npy",
                                  "summarize": name + ".summarize.npy", "query": name + ".query.npy", "str_chrom": str_chrom, "cases": cases, "gets": gets})
        print(name, len(cases), "regions,", at, "bins,", sum(c["level"] is not None for c in cases), "of them from a zoom level,", len(gets), "get regions")
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
