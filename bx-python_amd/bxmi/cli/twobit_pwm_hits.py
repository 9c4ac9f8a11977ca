#!/usr/bin/env python
"""
Read a BED file, a 2bit file and a position weight matrix, print every position of the sequence under the intervals where the
matrix scores at least THRESHOLD, as BED6: chrom, start and end of the site, the interval it was found in as "chrom:start-end",
the score, and the strand -- "+" for the matrix, "-" for its reverse complement, which -r scans as well.  An offset that cannot be
scored (a letter outside the alphabet in the window, or fewer letters left than the matrix is wide) is never a site.  Intervals
are clipped to their sequence.  The lines come in the order of the BED file's intervals, then by position, "+" before "-".  The
matrix file holds the alphabet's letters on its first line and one row of numbers per matrix position after it.  Masked bases
are lower case, and so outside an upper-case alphabet, unless -u is given.  With -s column 6 of the BED decides the strand (a
missing column or "." means "+"): an interval on "-" is scanned on its reverse complement, its sites are printed at their genomic
coordinates, and the strand printed is the interval's for the matrix and the opposite one for its reverse complement.

In place of the 2bit file a FASTA file (.gz too), a nib file or a directory of nib files may be given (the sequence is then the
file's stem); a letter outside ACGTN, in either case, is refused.

usage: %prog seq.2bit matrix.txt THRESHOLD [-r] [-u] [-s] < bed_file.bed
"""
# A site is an offset of the reference's bx.motif.pwm.ScoringMatrix.score_string on an interval's sequence whose score is >=
# THRESHOLD (pwm.py:141-149); here the whole BED file is ONE device call (bxmi.sequence.TwoBitSet.hits) that writes the sites
# alone.  Comment and header lines of the BED are skipped.
import math
import sys

import numpy as np

from bxmi import motif, sequence
from bxmi.genomic import track_rows


def _usage():
    sys.exit(__doc__.replace("%prog", "twobit_pwm_hits"))


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    flags = [a for a in argv if a in ("-r", "-u", "-s")]
    files = [a for a in argv if a not in ("-r", "-u", "-s")]  # (a THRESHOLD may begin with "-")
    if len(files) != 3:
        _usage()
    try:
        threshold = float(files[2])
    except ValueError:
        _usage()
    if math.isnan(threshold) or files[0].startswith("-") or files[1].startswith("-"):
        _usage()
    out = out or sys.stdout
    with open(files[1]) as f:
        matrices = [motif.read_matrix(f)]
    if "-r" in flags:
        matrices.append(matrices[0].reverse_complement())
    genome = sequence.TwoBitSet.open(files[0], do_mask="-u" not in flags)
    try:
        rows, track_of = track_rows(stdin or sys.stdin, genome.tracks)
        starts, ends = [r.start for r in rows], [r.end for r in rows]
        strands = [r.strand for r in rows] if "-s" in flags else None
        mat_hits, row, pos, score = genome.hits(track_of, starts, ends, matrices, threshold, strands)
        strand = np.repeat(np.arange(len(matrices)), np.diff(mat_hits))
        width = matrices[0].width
        # the sites' genomic starts: an offset of a minus interval counts from the clipped interval's end
        first, lengths = sequence._clip([tr.size for tr in genome.tracks.values()], np.asarray(track_of, dtype=np.int64), np.asarray(starts, dtype=np.int64),
                                        np.asarray(ends, dtype=np.int64))
        minus = np.array([s == "-" for s in strands], dtype=bool) if strands is not None else np.zeros(len(rows), dtype=bool)
        site = motif.site_starts(first[row], lengths[row], pos, width, minus[row])
        strand = strand ^ minus[row]  # (the reverse complement matrix finds the sites of the opposite strand)
        for k in np.lexsort((strand, site, row)):
            r = rows[row[k]]
            at = int(site[k])
            out.write("%s\t%d\t%d\t%s:%d-%d\t%s\t%s\n" % (r.chrom, at, at + width, r.chrom, r.start, r.end, repr(float(score[k])), "+-"[strand[k]]))
        out.flush()
    finally:
        genome.close()


if __name__ == "__main__":
    main()
