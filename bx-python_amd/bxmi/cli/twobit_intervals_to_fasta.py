#!/usr/bin/env python
"""
Read a BED file and a 2bit file, print the sequence under every interval to stdout: a header line "> chrom start end" and the
letters wrapped at 50 columns.  Intervals are clipped to their sequence; one that is empty, or on a sequence the file does not
have, prints its header only.  Masked bases are lower case unless -u is given.  With -c one tab-separated line is printed per
interval instead: chrom, start, end and the counts A, C, G, T, N, masked.  With -s column 6 of the BED decides the strand (a
missing column or "." means "+"): an interval on "-" prints its reverse complement, the header line gains the strand as a fourth
field ("> chrom start end strand") and -c counts the strand's letters (the line gains the strand after end).

In place of the 2bit file a FASTA file (.gz too), a nib file or a directory of nib files may be given (the sequence is then the
file's stem); a letter outside ACGTN, in either case, is refused.

usage: %prog seq.2bit [-c] [-u] [-s] < bed_file.bed
"""
# The output format is that of the reference's scripts/nib_intervals_to_fasta.py:25-38, which reads one slice per interval; here the
# whole BED file is ONE device call (bxmi.sequence.TwoBitSet.strings / composition).  Comment and header lines of the BED are skipped.
# -s is what twoBitToFa -bed and bedtools getfasta -s do: the reference's SeqFile.reverse_complement (lib/bx/seq/seq.py:108-109).
import sys

from bxmi import sequence
from bxmi.genomic import track_rows


def print_wrapped(s, out):
    for c in range(0, len(s), 50):
        out.write(s[c:c + 50] + "\n")


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    flags = [a for a in argv if a.startswith("-")]
    files = [a for a in argv if not a.startswith("-")]
    if len(files) != 1 or any(f not in ("-c", "-u", "-s") for f in flags):
        sys.exit(__doc__.replace("%prog", "twobit_intervals_to_fasta"))
    out = out or sys.stdout
    genome = sequence.TwoBitSet.open(files[0], do_mask="-u" not in flags)
    try:
        rows, track_of = track_rows(stdin or sys.stdin, genome.tracks)
        starts, ends = [r.start for r in rows], [r.end for r in rows]
        strands = [r.strand for r in rows] if "-s" in flags else None
        if "-c" in flags:
            for r, counts in zip(rows, genome.composition(track_of, starts, ends, strands).tolist()):
                out.write("\t".join([r.chrom, str(r.start), str(r.end)] + ([r.strand] if strands is not None else []) + [str(c) for c in counts]) + "\n")
        else:
            for r, s in zip(rows, genome.strings(track_of, starts, ends, strands)):
                out.write("> %s %d %d%s\n" % (r.chrom, r.start, r.end, " " + r.strand if strands is not None else ""))
                print_wrapped(s, out)
        out.flush()
    finally:
        genome.close()


if __name__ == "__main__":
    main()
