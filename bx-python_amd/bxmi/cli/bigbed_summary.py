#!/usr/bin/env python
"""
Summarize a bigBed file over every interval of a BED file: SIZE equal bins per interval, one statistic per bin, every row
answered as the reference's BigBedFile.summarize / query would answer it: from the zoom level its rule picks for the row, or
from the file's records where it picks none; with -f, always from the records (summarize_from_full).  One output line per BED
row: chrom, start, end and SIZE values, separated by tabs.  A row whose chromosome the bigBed file does not have, or whose
interval is empty, prints n/a for every value.  The default statistic is coverage, the share of a bin's bases that records
cover (counted once per record), which is the one that means something for bigBed.

usage: %prog feats.bb SIZE [-t coverage|mean|min|max|std] [-f] < bed_file.bed
"""
# The line format is bxmi.cli.bigwig_summary's: the values are those of `query`, printed with %.17g so that they read back as
# the same float64; the whole BED file is ONE device call per kind of track (bxmi.summary.BedSet.summarize).
import sys

import numpy as np

from bxmi import summary
from bxmi.genomic import track_rows

KINDS = ("coverage", "mean", "min", "max", "std")


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    kind = "coverage"
    full = "-f" in argv
    if full:
        argv.remove("-f")
    if "-t" in argv:
        at = argv.index("-t")
        if at + 1 >= len(argv):
            sys.exit(__doc__.replace("%prog", "bigbed_summary"))
        kind = argv[at + 1]
        del argv[at:at + 2]
    if len(argv) != 2 or kind not in KINDS:
        sys.exit(__doc__.replace("%prog", "bigbed_summary"))
    out = out or sys.stdout
    size = int(argv[1])
    beds = summary.BedSet.from_bigbed(argv[0])
    try:
        rows, track_of = track_rows(stdin or sys.stdin, beds.full)
        starts = np.array([r.start for r in rows], dtype=np.int64)
        ends = np.array([r.end for r in rows], dtype=np.int64)
        res = beds.summarize(track_of, starts, ends, size, zoom=not full)
        answered = (track_of >= 0) & (starts < ends)
        if kind == "min":
            values = res.min_val
        elif kind == "max":
            values = res.max_val
        else:
            safe_ends = np.where(answered, ends, starts + 1)
            mean, coverage, std_dev = summary.stats(res, starts, safe_ends, size)
            values = {"mean": mean, "coverage": coverage, "std": std_dev}[kind]
        for i, r in enumerate(rows):
            cells = ["%.17g" % x for x in values[i]] if answered[i] else ["n/a"] * size
            out.write("\t".join([r.chrom, str(r.start), str(r.end)] + cells) + "\n")
        out.flush()
    finally:
        beds.close()


if __name__ == "__main__":
    main()
