#!/usr/bin/env python
"""
The per-base signal of a bigWig file around the centre of every interval of a BED file: the site x base matrix behind a
base-resolution heatmap.  Row i holds the 2 * PADDING values from (start + end) // 2 - PADDING on, nan where the file has no data
(a chromosome it does not have, a base outside it).  With -o the matrix is saved as a float32 .npy array [rows, 2 * PADDING];
without it one line is printed per BED row: chrom, start, end and the values, separated by tabs.

usage: %prog score.bw PADDING [-o out.npy] < bed_file.bed
"""
# The windows are those of the reference's scripts/bed_bigwig_profile.py:29-33, which calls BigWigFile.get_as_array once per
# interval and adds the arrays up; here the arrays themselves are the result and the whole BED file is ONE device call
# (bxmi.summary.matrix) over the file's items (SpanTrack): no dense per-chromosome array is built.  Values are printed with %.9g,
# which reads back as the same float32.  Comment and header lines of the BED are skipped.
import sys

import numpy as np

from bxmi import _ffi, summary
from bxmi.genomic import track_rows


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    save = None
    if "-o" in argv:
        at = argv.index("-o")
        if at + 1 >= len(argv):
            sys.exit(__doc__.replace("%prog", "bigwig_matrix"))
        save = argv[at + 1]
        del argv[at:at + 2]
    try:
        padding = int(argv[1]) if len(argv) == 2 else 0
    except ValueError:
        padding = 0
    if padding < 1:
        sys.exit(__doc__.replace("%prog", "bigwig_matrix"))
    out = out or sys.stdout
    tracks = summary.SpanTrack.from_bigwig(argv[0])
    try:
        rows, track_of = track_rows(stdin or sys.stdin, tracks)
        starts = np.array([(r.start + r.end) // 2 - padding for r in rows], dtype=np.int64)
        values = summary.matrix(tracks.values(), track_of, starts, 2 * padding)
        if save is not None:
            with open(save, "wb") as f:  # (the name as given: np.save on a name would append .npy)
                np.save(f, values)
            return
        for r, row in zip(rows, values):
            out.write("\t".join([r.chrom, str(r.start), str(r.end)] + ["%.9g" % x for x in row]) + "\n")
        out.flush()
    finally:
        _ffi.close_all(tracks.values())


if __name__ == "__main__":
    main()
