#!/usr/bin/env python
"""
Read a set of ranges "chrom start end" from stdin and a directory of nib files, print the portions of nib_dir/chrom.nib under those
ranges to stdout: per range a header line "> chrom start end" and the letters wrapped at 50 columns, in the order of the input.

A range outside its sequence raises the AssertionError of bx.seq's ``get`` for the first such line of its chromosome, BEFORE ANY
OUTPUT: the ranges of a nib file go to the device in one call.  (The reference prints the records before that line first.)

usage: %prog nib_dir < range_file
"""
# The reference's scripts/nib_chrom_intervals_to_fasta.py reads one slice per range; here every nib file is ONE device call
# (bx.seq.nib.NibFile.get_batch), the files in the order in which the input first names them.
import os
import sys

import bx.seq.nib
from bxmi.cli.nib_intervals_to_fasta import print_wrapped


def main(argv=None, stdin=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) != 1:
        sys.exit(__doc__.replace("%prog", "nib_chrom_intervals_to_fasta"))
    out = out or sys.stdout
    ranges = [(f[0], int(f[1]), int(f[2])) for f in (line.split() for line in (stdin or sys.stdin))]
    rows_of = {}
    for i, (chrom, _, _) in enumerate(ranges):
        rows_of.setdefault(chrom, []).append(i)
    texts = [None] * len(ranges)
    for chrom, rows in rows_of.items():
        with open(os.path.join(argv[0], chrom + ".nib"), "rb") as nib_file:
            nib = bx.seq.nib.NibFile(nib_file)
            try:
                got = nib.get_batch([ranges[i][1] for i in rows], [ranges[i][2] - ranges[i][1] for i in rows])
            finally:
                nib.release()
        for i, text in zip(rows, got):
            texts[i] = text
    for (chrom, start, end), text in zip(ranges, texts):
        out.write("> %s %d %d\n" % (chrom, start, end))
        print_wrapped(text, out)
    out.flush()


if __name__ == "__main__":
    main()
