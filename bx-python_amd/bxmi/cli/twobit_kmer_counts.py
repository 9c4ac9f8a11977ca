#!/usr/bin/env python
"""
Read a BED file and a 2bit file, count how often every word of K letters over A, C, G, T occurs in the sequence under every
interval.  A header line of the words, tab separated after "#chrom start end", then one line per interval: its first three fields
and the counts, tab separated.  Intervals are clipped to their sequence; one that is empty, shorter than K, or on a sequence the
file does not have counts nothing.  A word over an N is not counted.  Masked bases are lower case and so without a digit, unless
-u (no masking) or -i (case-insensitive: lower case counts as upper case) is given.  With -c the two strands are collapsed: a word
and its reverse complement are counted together, under the one that comes first in the header's order, and only those columns are
printed.  With -o the int32 [intervals, words] array is saved to out.npy instead and nothing is printed.  With -s column 6 of the
BED decides the strand (a missing column or "." means "+"): the words of an interval on "-" are those of its reverse complement,
and every line gains the strand as a fourth field (the header "strand").

In place of the 2bit file a FASTA file (.gz too), a nib file or a directory of nib files may be given (the sequence is then the
file's stem); a letter outside ACGTN, in either case, is refused.

usage: %prog seq.2bit K [-u] [-i] [-c] [-o out.npy] [-s] < bed_file.bed
"""
# The counts are those of the reference's bx.intseq.ngramcount.count_ngrams over bx.seqmapping.DNA's digits (ngramcount.pyx:34-85),
# every window of an interval included; here the whole BED file is ONE device call (bxmi.sequence.TwoBitSet.kmer_counts).  Comment and
# header lines of the BED are skipped.
import sys

import numpy as np

from bxmi import kmers, sequence
from bxmi.genomic import track_rows


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = __doc__.replace("%prog", "twobit_kmer_counts")
    flags, files, save = [], [], None
    while argv:
        a = argv.pop(0)
        if a == "-o":
            if not argv:
                sys.exit(usage)
            save = argv.pop(0)
        elif a.startswith("-"):
            flags.append(a)
        else:
            files.append(a)
    if len(files) != 2 or any(f not in ("-u", "-i", "-c", "-s") for f in flags) or not files[1].isdigit() or int(files[1]) < 1:
        sys.exit(usage)
    k = int(files[1])
    kmers.bins_of(k, 4)
    out = out or sys.stdout
    genome = sequence.TwoBitSet.open(files[0], do_mask="-u" not in flags)
    try:
        rows, track_of = track_rows(stdin or sys.stdin, genome.tracks)
        strands = [r.strand for r in rows] if "-s" in flags else None
        table = genome.kmer_counts(track_of, [r.start for r in rows], [r.end for r in rows], k, case_sensitive="-i" not in flags, strands=strands)
    finally:
        genome.close()
    names = kmers.words(k)
    if "-c" in flags:
        keep = kmers.canonical_columns(k)
        table = kmers.fold_reverse_complement(table, k)[:, keep]
        names = [names[i] for i in keep]
    if save is not None:
        np.save(save, table)
        return
    out.write("\t".join(["#chrom", "start", "end"] + (["strand"] if strands is not None else []) + names) + "\n")
    for r, line in zip(rows, table.tolist()):
        out.write("\t".join([r.chrom, str(r.start), str(r.end)] + ([r.strand] if strands is not None else []) + [str(c) for c in line]) + "\n")
    out.flush()


if __name__ == "__main__":
    main()
