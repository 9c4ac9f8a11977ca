#!/usr/bin/env python
"""
Write the two generated nib files of tests/golden/seqfile: BIG-endian (the reference's own test.nib is little-endian), of ODD length
(the last byte holds one base), with N and lower case at both ends and runs of them that begin and end at odd and at even positions,
so that blocks cross the bytes' boundaries both ways.  The letters are seeded; the file is magic, length, nibbles (lib/bx/seq/nib.py
of the reference: codes T=0 C=1 A=2 G=3 N=4, bit 3 = lower case, the first base of a byte in its high nibble).

usage: write_nib_fixture.py [GOLDEN_DIR]
"""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden", "seqfile")
MAGIC = 0x6BE93D3A
CODES = {ch: code for code, ch in enumerate("TCAGN")}


def nib_bytes(text, byte_order=">"):
    v = [CODES[ch.upper()] | (8 if ch.islower() else 0) for ch in text] + [0] * (len(text) & 1)
    body = bytes(v[i] << 4 | v[i + 1] for i in range(0, len(v), 2))
    return struct.pack(">L", MAGIC)[::1 if byte_order == ">" else -1] + struct.pack(byte_order + "L", len(text)) + body


def edges_text():
    """75 bases: N at both ends, lower case next to them, short runs at odd and even positions"""
    return "NNN" + "nnacg" + "ACGTTGCA" + "N" + "AC" + "nn" + "GTACGTA" + "ttt" + "CAGTCAGTCA" + "NN" + "acgtnNNnacgt" + "GATTACA" + "c" + "TTGCATG" + "gca" + "Nn"


def random_text(seed=77, size=131):
    rng = np.random.default_rng(seed)
    out, at = [], 0
    while at < size:
        step = min(int(rng.integers(1, 12)), size - at)
        kind = int(rng.integers(0, 4))  # plain, lower case, N, n
        for _ in range(step):
            ch = "ACGT"[int(rng.integers(0, 4))]
            out.append((ch, ch.lower(), "N", "n")[kind])
        at += step
    out[0], out[-1] = "n", "N"
    return "".join(out)


def main(argv):
    golden = argv[0] if argv else GOLDEN
    os.makedirs(golden, exist_ok=True)
    for name, text in (("edges_be.nib", edges_text()), ("random_be.nib", random_text())):
        assert len(text) % 2 == 1
        with open(os.path.join(golden, name), "wb") as f:
            f.write(nib_bytes(text))
        print("%s: %d bases" % (name, len(text)))


if __name__ == "__main__":
    main(sys.argv[1:])
