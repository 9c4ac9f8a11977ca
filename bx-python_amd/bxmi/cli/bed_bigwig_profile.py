#!/usr/bin/env python
"""
Create a site profile: the average signal of a score file at every offset around the centre of each interval of a BED file,
over all the intervals that have data at that offset.  One line per offset, 2 * padding lines.

usage: %prog score_file padding < bed_file.bed
"""
# The command-line counterpart of the reference's scripts/bed_bigwig_profile.py:27-41 -- same arguments, same lines -- with ONE
# device call for the whole BED file (bxmi.scores.profile) where the reference reads and adds an array per interval in Python.
# score_file is bigWig, or wiggle text (.gz too) when the bigWig magic number is absent.  A window that starts below zero and a
# chromosome the score file does not have are crashes in the reference (OverflowError, and `isnan(None)`); here those positions
# have no data.  Comment and header lines of the BED are skipped.
import sys

import numpy as np

from bxmi import _ffi, bigwig, scores, wiggle
from bxmi.genomic import track_rows


def load_tracks(path):
    """{chrom: ScoreTrack}: a bigWig's tracks have its chromosome sizes, a wiggle's reach to their largest span end."""
    if bigwig.is_bigwig(path):
        sizes, spans = bigwig.chroms(path), bigwig.read_spans_file(path)
    else:
        spans = wiggle.read_spans_file(path)
        sizes = {chrom: max(int(e.max()) if len(e) else 0, 0) for chrom, (s, e, v) in spans.items()}
    tracks = {}
    for chrom, size in sizes.items():
        t = tracks[chrom] = scores.ScoreTrack(size)
        t.set_spans(*spans[chrom])
    return tracks


def main(argv=None, stdin=None, out=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        sys.exit(__doc__.replace("%prog", "bed_bigwig_profile"))
    out = out or sys.stdout
    padding = int(argv[1])
    tracks = load_tracks(argv[0])
    try:
        rows, track_of = track_rows(stdin or sys.stdin, tracks)
        starts = np.array([(r.start + r.end) // 2 - padding for r in rows], dtype=np.int64)
        if padding > 0:
            res = scores.profile(tracks.values(), track_of, starts, 2 * padding)
            with np.errstate(all="ignore"):
                np.savetxt(out, res.totals / res.valid)
        out.flush()
    finally:
        _ffi.close_all(tracks.values())


if __name__ == "__main__":
    main()
