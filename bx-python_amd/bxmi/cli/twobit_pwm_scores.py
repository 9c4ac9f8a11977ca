#!/usr/bin/env python
"""
Read a BED file, a 2bit file and a position weight matrix, print the matrix's score at every offset of the sequence under every
interval: a header line "> chrom start end" and then, per matrix, one line of space-separated scores ("nan" where an offset cannot
be scored: a letter outside the alphabet in the window, or fewer letters left than the matrix is wide).  Intervals are clipped to
their sequence; one that is empty, or on a sequence the file does not have, prints its header and empty lines.  The matrix file
holds the alphabet's letters on its first line and one row of numbers per matrix position after it.  With -r the reverse
complement of the matrix is scored as a second matrix.  Masked bases are lower case, and so outside an upper-case alphabet,
unless -u is given.  With -b one tab-separated line is printed per interval instead: chrom, start, end and, per matrix, the best
score and the first offset that holds it ("nan" and -1 where nothing could be scored).  With -s column 6 of the BED decides the
strand (a missing column or "." means "+"): an interval on "-" is scored on its reverse complement, the header line gains the
strand as a fourth field ("> chrom start end strand"; with -b the line gains it after end), the scores come in the order of the
strand's string and -b prints the offset in that string.  (-r on a "+" interval is not the same numbers: it adds the same terms in
the opposite order.)

In place of the 2bit file a FASTA file (.gz too), a nib file or a directory of nib files may be given (the sequence is then the
file's stem); a letter outside ACGTN, in either case, is refused.

usage: %prog seq.2bit matrix.txt [-r] [-b] [-u] [-s] < bed_file.bed
"""
# The scores are those of the reference's bx.motif.pwm.ScoringMatrix.score_string on each interval's sequence (pwm.py:141-149); here
# the whole BED file is ONE device call (bxmi.sequence.TwoBitSet.scores / best).  Comment and header lines of the BED are skipped.
import sys

from bxmi import motif, sequence
from bxmi.genomic import track_rows


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    flags = [a for a in argv if a.startswith("-")]
    files = [a for a in argv if not a.startswith("-")]
    if len(files) != 2 or any(f not in ("-r", "-b", "-u", "-s") for f in flags):
        sys.exit(__doc__.replace("%prog", "twobit_pwm_scores"))
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
        if "-b" in flags:
            score, pos = genome.best(track_of, starts, ends, matrices, strands)
            for i, r in enumerate(rows):
                hits = ["%s\t%d" % (repr(float(score[m, i])), pos[m, i]) for m in range(len(matrices))]
                out.write("\t".join([r.chrom, str(r.start), str(r.end)] + ([r.strand] if strands is not None else []) + hits) + "\n")
        else:
            planes, offsets = genome.scores(track_of, starts, ends, matrices, strands)
            for i, r in enumerate(rows):
                out.write("> %s %d %d%s\n" % (r.chrom, r.start, r.end, " " + r.strand if strands is not None else ""))
                for m in range(len(matrices)):
                    out.write(" ".join(repr(float(x)) for x in planes[m, offsets[i]:offsets[i + 1]]) + "\n")
        out.flush()
    finally:
        genome.close()


if __name__ == "__main__":
    main()
