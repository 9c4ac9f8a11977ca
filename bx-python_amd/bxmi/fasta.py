"""
Reader of FASTA files (what the reference's bx.seq.fasta.FastaFile accepts, lib/bx/seq/fasta.py:50-79): every record's letters as a
uint8 array, for bxmi.sequence to build a 2bit track from on the device (TwoBitTrack.from_letters, TwoBitSet.from_fasta).

As FastaFile parses: a line that starts with ">" is a header and its record's name is the first word after the ">", or "" without
one; every other line is split on whitespace and its words joined, so all whitespace inside sequence lines is dropped; lines
before the first header make a headerless first record named ""; a header without lines gives a record of size 0.  A duplicate
name raises ValueError -- the reference reads records by position, this module's callers by name.  The whole file is handled as
numpy arrays: no Python runs per base, only per record.
"""
import gzip

import numpy as np

# what str.split() takes for whitespace among the ASCII bytes
_SPACE = np.zeros(256, dtype=bool)
_SPACE[[9, 10, 11, 12, 13, 28, 29, 30, 31, 32]] = True


def _bytes_of(path, data):
    if data is None:
        with open(path, "rb") as f:
            data = f.read()
    data = bytes(data)
    if data[:2] == b"\x1f\x8b":  # (.gz, by what it is and not by its name)
        data = gzip.decompress(data)
    return data


def read_file(path=None, data=None):
    """{name: uint8 letters} of a FASTA file (`path`, .gz accepted, or `data`: its bytes), in file order"""
    a = np.frombuffer(_bytes_of(path, data), dtype=np.uint8)
    newline = np.flatnonzero(a == 10)
    line_start = np.concatenate([[0], newline + 1])
    line_start = line_start[line_start < len(a)]
    head = line_start[a[line_start] == ord(">")]               # where the header lines start
    head_end = np.concatenate([newline, [len(a)]])[np.searchsorted(newline, head)]  # ... and end: their newline, or the file's end
    keep = ~_SPACE[a]
    inside = np.zeros(len(a) + 1, dtype=np.int32)              # (a header's bytes are no letters)
    np.add.at(inside, head, 1)
    np.add.at(inside, head_end, -1)
    keep &= np.cumsum(inside[:-1]) == 0
    kept_before = np.concatenate([[0], np.cumsum(keep)])       # letters among the file's bytes [0, i)
    letters = a[keep]
    out = {}
    first = int(head[0]) if len(head) else len(a)
    if first > 0:  # (any line before the first header, a blank one too: FastaFile's text is no longer None)
        out[""] = letters[:kept_before[first]]
    bounds = np.concatenate([head, [len(a)]])
    for k in range(len(head)):
        words = a[head[k] + 1:head_end[k]].tobytes().decode("latin-1").split()
        name = words[0] if words else ""
        if name in out:
            raise ValueError("FASTA file holds two records named %r" % name)
        out[name] = letters[kept_before[head_end[k]]:kept_before[bounds[k + 1]]]
    return out
