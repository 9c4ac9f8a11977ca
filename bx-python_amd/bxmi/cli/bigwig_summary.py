#!/usr/bin/env python
"""
Summarize a bigWig file over every interval of a BED file: SIZE equal bins per interval, one statistic per bin, computed from
the file's full-resolution data; with -z, every row is answered as the reference's BigWigFile.summarize / query would answer
it: from the zoom level its rule picks for the row, or from full data where it picks none.  One output line per BED row: chrom,
start, end and SIZE values, separated by tabs.  A row whose chromosome the bigWig file does not have, or whose interval is
empty, prints n/a for every value.  (Full data without -z is the default kept for compatibility with tests that pin it; it is
meant to flip later.)

usage: %prog score.bw SIZE [-t mean|min|max|coverage|std] [-z] < bed_file.bed
"""
# There is no reference script for this: the reference offers BigWigFile.summarize / query (lib/bx/bbi/bbi_file.pyx:187-260) as
# calls only, one region at a time; the line format here is this project's own.  The values are those of `query` from full data
# (summarize_from_full), printed with %.17g so that they read back as the same float64; the whole BED file is ONE device call
# (bxmi.summary.summarize); with -z it is bxmi.summary.TrackSet.summarize(zoom=True): one call per kind of track.  Comment and
# header lines of the BED are skipped.
import sys

import numpy as np

from bxmi import _ffi, summary
from bxmi.genomic import track_rows

KINDS = ("mean", "min", "max", "coverage", "std")


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    kind = "mean"
    use_zoom = "-z" in argv
    if use_zoom:
        argv.remove("-z")
    if "-t" in argv:
        at = argv.index("-t")
        if at + 1 >= len(argv):
            sys.exit(__doc__.replace("%prog", "bigwig_summary"))
        kind = argv[at + 1]
        del argv[at:at + 2]
    if len(argv) != 2 or kind not in KINDS:
        sys.exit(__doc__.replace("%prog", "bigwig_summary"))
    out = out or sys.stdout
    size = int(argv[1])
    file_tracks = summary.TrackSet.from_bigwig(argv[0]) if use_zoom else None
    tracks = file_tracks.spans if use_zoom else summary.SpanTrack.from_bigwig(argv[0])
    try:
        rows, track_of = track_rows(stdin or sys.stdin, tracks)
        starts = np.array([r.start for r in rows], dtype=np.int64)
        ends = np.array([r.end for r in rows], dtype=np.int64)
        if use_zoom:
            res = file_tracks.summarize(track_of, starts, ends, size, zoom=True)
        else:
            res = summary.summarize(tracks.values(), track_of, starts, ends, size)
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
        if use_zoom:
            file_tracks.close()
        else:
            _ffi.close_all(tracks.values())


if __name__ == "__main__":
    main()
