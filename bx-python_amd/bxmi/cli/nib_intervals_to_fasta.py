#!/usr/bin/env python
"""
Read a set of ranges and a nib file, print the portions of the nib under those ranges to stdout: per line "start end" of the range
file a header line "> start end" and the letters wrapped at 50 columns.

A range outside the sequence raises the AssertionError of bx.seq's ``get`` for the FIRST such line, BEFORE ANY OUTPUT: all ranges go
to the device in one call.  (The reference prints the records before that line first.)

usage: %prog range_file nib_file
"""
# The reference's scripts/nib_intervals_to_fasta.py reads one slice per range; here the whole range file is ONE device call
# (bx.seq.nib.NibFile.get_batch).
import sys

import bx.seq.nib


def print_wrapped(s, out):
    for c in range(0, len(s), 50):
        out.write(s[c:c + 50] + "\n")


def main(argv=None, out=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) != 2:
        sys.exit(__doc__.replace("%prog", "nib_intervals_to_fasta"))
    out = out or sys.stdout
    with open(argv[0]) as range_file:
        ranges = [(int(f[0]), int(f[1])) for f in (line.split() for line in range_file)]
    with open(argv[1], "rb") as nib_file:
        nib = bx.seq.nib.NibFile(nib_file)
        try:
            texts = nib.get_batch([s for s, _ in ranges], [e - s for s, e in ranges])
        finally:
            nib.release()
    for (start, end), text in zip(ranges, texts):
        out.write("> %d %d\n" % (start, end))
        print_wrapped(text, out)
    out.flush()


if __name__ == "__main__":
    main()
