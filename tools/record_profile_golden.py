#!/usr/bin/env python
"""
Record what the reference computes for the cases of tests/golden/profile (run where a built reference is at hand; the engine is
not involved).  Per bigWig file: ``BigWigFile.get_as_array`` over a list of regions, concatenated into one float32 .npy, and the
chromosome sizes.  Per profile case: `totals`, `valid` and the ``savetxt`` text of scripts/bed_bigwig_profile.py:29-41, the
lines read from the script and executed as they are on the reference's own ``BigWigFile`` and ``GenomicIntervalReader``.  The
script itself cannot be run under Python 3: ``get_as_array`` takes ``char *chrom`` and the reader yields ``str`` (TypeError:
expected bytes, str found), so the rows reach those lines with their chromosome as bytes and nothing else is changed.  manifest.json lists the files, regions, cases and results.

The small bigWig files and the BEDs come from tools/write_bigwig_fixture.py (written first where missing); test.bw and
test.wig(.gz) are copies of the reference's test_data/bbi_tests files.  Also recorded: whether test.bw / test.wig and bg.bw /
bg.wig describe the same tracks (bigWig through the reference, wiggle through tests/profile_model.py's dense loader).

The synthetic wide-range case of tests/test_profile_model_golden.py needs no reference; its order-sensitivity is asserted here
as well: at least half of its columns have an ordered sum that differs from the same chain split in two halves.

Building the reference's modules (a writable copy of its lib/ and src/, Cython and numpy, nothing else):

    from setuptools import setup, Extension
    from Cython.Build import cythonize
    import numpy
    names = ["bx.bbi.bpt_file", "bx.bbi.cirtree_file", "bx.bbi.bbi_file", "bx.bbi.bigwig_file", "bx.intervals.intersection"]
    exts = [Extension(n, ["lib/" + n.replace(".", "/") + ".pyx"], include_dirs=[numpy.get_include()]) for n in names]
    # bx.intervals.io imports bx.bitset: built as oracle/build_pyref.sh builds it (a copy of the reference's src/ beside lib/)
    exts.append(Extension("bx.bitset", ["lib/bx/bitset.pyx", "src/binBits.c", "src/kent/bits.c", "src/kent/common.c"], include_dirs=["src/kent", "src"]))
    setup(name="bxbbi", package_dir={"": "lib"}, ext_modules=cythonize(exts, language_level=3), script_args=["build_ext", "--inplace"])

usage: record_profile_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR [REFERENCE_ROOT]]
(REFERENCE_ROOT holds scripts/ and test_data/; default: the parent of REFERENCE_LIB_DIR)
"""
import gzip
import io
import json
import os
import shutil
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)

# file -> regions (chrom, start, end); starts are never negative and chromosomes are known (the reference crashes otherwise)
REGIONS = {
    "bg.bw": [("chr1", 0, 400), ("chr1", 5, 33), ("chr1", 120, 131), ("chr1", 395, 450)],
    "bg.z.bw": [("chr1", 0, 400), ("chr1", 28, 37)],
    "fs.bw": [("chrF", 0, 250), ("chrF", 98, 112), ("chrF", 150, 166)],
    "fs.z.bw": [("chrF", 0, 250)],
    "two.z.bw": [("chrA", 0, 100), ("chrBB", 0, 50), ("chrA", 18, 62), ("chrBB", 40, 60)],
    "two.be.bw": [("chrA", 0, 100), ("chrBB", 0, 50)],
    "test.bw": [("chr1", 10000, 21000), ("chr1", 10917, 10919), ("chr1", 15000, 15100), ("chr1", 0, 64), ("chr1", 20800, 21200)],
}
# name -> (scores, bed, padding)
PROFILES = {
    "bg": ("bg.bw", "bg.bed", 25),
    "bg.z": ("bg.z.bw", "bg.bed", 4),
    "bg.gap": ("bg.bw", "gap.bed", 40),
    "fs": ("fs.bw", "fs.bed", 10),
    "fs.z": ("fs.z.bw", "fs.bed", 30),
    "two.z": ("two.z.bw", "two.bed", 12),
    "two.be": ("two.be.bw", "two.bed", 1),
    "test": ("test.bw", "test.bed", 100),
}
TWINS = [("test.bw", "test.wig.gz"), ("bg.bw", "bg.wig")]
TWIN_EXTENT = 1 << 22  # twins are compared over [0, this) of every chromosome (test.bw: 247 Mbp, data below 21 kbp)


SCRIPT_LINES = (28, 41)  # of scripts/bed_bigwig_profile.py: from `padding = ...` to the savetxt; line 27 opens the file in text mode


def reference_profile(script_path, BigWigFile, GenomicIntervalReader, score_path, bed_path, padding):
    """Lines 28-41 of the reference's script, read from it and executed unchanged, around a BigWigFile opened in binary mode and a
    reader whose rows carry their chromosome as bytes."""
    import types

    import numpy

    with open(script_path) as f:
        body = "".join(f.readlines()[SCRIPT_LINES[0] - 1:SCRIPT_LINES[1]])

    class Row:
        def __init__(self, interval):
            self.chrom, self.start, self.end = interval.chrom.encode(), interval.start, interval.end

    out = io.StringIO()
    with open(score_path, "rb") as score_file, open(bed_path) as bed_file:
        fake_sys = types.SimpleNamespace(argv=["bed_bigwig_profile.py", score_path, str(padding)], stdin=bed_file, stdout=out)
        scope = {name: getattr(numpy, name) for name in ("float64", "floor", "int32", "isnan", "savetxt", "zeros")}
        scope.update(sys=fake_sys, bw=BigWigFile(score_file), GenomicIntervalReader=lambda lines: (Row(r) for r in GenomicIntervalReader(lines)))
        with np.errstate(all="ignore"):
            exec(compile(body, script_path, "exec"), scope)
    return scope["totals"], scope["valid"], out.getvalue()


def dense_from_reference(bw, chrom, size):
    return bw.get_as_array(chrom.encode(), 0, size)


def check_synthetic():
    import profile_model as M

    frac = M.fraction_split_sensitive(*M.wide_range_case())
    print("wide-range case: %.0f %% of the columns differ from the chain split in two" % (100 * frac))
    assert frac >= 0.5, "the synthetic case cannot tell an ordered chain from anything else"


def main(libdir, golden=os.path.join(HERE, "..", "tests", "golden", "profile"), reference=None):
    reference = reference or os.path.join(libdir, "..")
    import profile_model as M
    import write_bigwig_fixture as W

    W.main(golden)
    check_synthetic()
    sys.path.insert(0, libdir)
    from bx.bbi.bigwig_file import BigWigFile
    from bx.bbi.bpt_file import BPTFile
    from bx.intervals.io import GenomicIntervalReader

    data_dir = os.path.join(reference, "test_data", "bbi_tests")
    script = os.path.join(reference, "scripts", "bed_bigwig_profile.py")
    if not os.path.exists(os.path.join(golden, "test.bw")):
        shutil.copy(os.path.join(data_dir, "test.bw"), os.path.join(golden, "test.bw"))
    if not os.path.exists(os.path.join(golden, "test.wig.gz")):
        with open(os.path.join(data_dir, "test.wig"), "rb") as src, open(os.path.join(golden, "test.wig.gz"), "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
                f.write(src.read())

    manifest = {"files": [], "profiles": [], "twins": []}
    sizes = {}
    for name, regions in REGIONS.items():
        with open(os.path.join(golden, name), "rb") as f:
            bw = BigWigFile(f)
            arrays = [bw.get_as_array(c.encode(), s, e) for c, s, e in regions]
            # (the file's B+ tree of chromosomes is not reachable through BigWigFile: the reference's BPTFile is attached by hand)
            f.seek(0)
            head = f.read(16)
            order = ">" if struct.unpack(">I", head[:4])[0] == 0x888FFC26 else "<"
            f.seek(struct.unpack(order + "Q", head[8:16])[0])
            bpt = BPTFile(f)
            chroms = {chrom: int(struct.unpack(order + "II", bpt.find(chrom.encode()))[1]) for chrom in sorted({r[0] for r in regions})}
        assert all(a.dtype == np.float32 and len(a) == e - s for a, (_, s, e) in zip(arrays, regions))
        np.save(os.path.join(golden, name + ".regions.npy"), np.concatenate(arrays))
        sizes[name] = chroms
        manifest["files"].append({"file": name, "chroms": chroms, "regions": [list(r) for r in regions], "arrays": name + ".regions.npy"})
        print(name, chroms, sum(len(a) for a in arrays))
    for name, (scores, bed, padding) in PROFILES.items():
        totals, valid, text = reference_profile(script, BigWigFile, GenomicIntervalReader, os.path.join(golden, scores), os.path.join(golden, bed), padding)
        np.save(os.path.join(golden, name + ".totals.npy"), totals)
        np.save(os.path.join(golden, name + ".valid.npy"), valid)
        with open(os.path.join(golden, name + ".profile.txt"), "w") as f:
            f.write(text)
        rows = sum(1 for line in open(os.path.join(golden, bed)) if line.strip())
        manifest["profiles"].append({"name": name, "scores": scores, "bed": bed, "padding": padding, "rows": rows, "totals": name + ".totals.npy",
                                     "valid": name + ".valid.npy", "text": name + ".profile.txt"})
        print(name, rows, int(valid.sum()))
    for bigwig_name, wiggle_name in TWINS:
        same = True
        with open(os.path.join(golden, bigwig_name), "rb") as f:
            bw = BigWigFile(f)
            tracks = M.load_wiggle(os.path.join(golden, wiggle_name))
            for chrom, size in sizes[bigwig_name].items():
                size = min(size, TWIN_EXTENT)
                ref = dense_from_reference(bw, chrom, size)
                mine = np.full(size, np.nan, dtype=np.float32)
                t = tracks.get(chrom, np.zeros(0, dtype=np.float32))
                mine[:min(len(t), size)] = t[:size]
                same = same and ref.tobytes() == mine.tobytes()
        manifest["twins"].append({"bigwig": bigwig_name, "wiggle": wiggle_name, "same": bool(same)})
        print(bigwig_name, wiggle_name, "same track" if same else "DIFFERENT tracks")
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
