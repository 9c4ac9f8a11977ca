#!/usr/bin/env python
"""
A minimal bigBed writer, for test fixtures only: the header, the chromosome B+ tree as one leaf, data blocks of records
``(uint32 chrom_id, uint32 start, uint32 end, rest, NUL)``, compressed or not, in either byte order, and a one-level R-tree whose
leaf entries run from ``(chrom, start)`` of a block's first record to ``(chrom, furthest end)`` of its last chromosome -- so a
block may cross a chromosome boundary, as in real files.  Optional zoom levels are tools/write_bigwig_zoom_fixture.py's (bigBed
zoom records have the same format); the file itself is written by that writer with the bigBed magic number and these blocks.
Nothing in the reference writes bigBed; that the reference's reader reads these files (tools/record_bigbed_golden.py) is the
proof they are valid.

`FIXTURES` below is the definition of the files under tests/golden/bigbed; run as a script it writes the missing ones.

usage: write_bigbed_fixture.py [GOLDEN_DIR]
"""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import write_bigwig_zoom_fixture as Z  # noqa: E402

BIGBED_MAGIC = 0x8789F2EB


def bed_block(order, records):
    """((start chrom, start base, end chrom, end base), bytes) of one data block; records = [(chrom_id, start, end, rest)]"""
    raw = b"".join(struct.pack(order + "III", c, s, e) + rest.encode() + b"\0" for c, s, e, rest in records)
    last = records[-1][0]
    return (records[0][0], records[0][1], last, max(e for c, _, e, _ in records if c == last)), raw


def write_bigbed(path, chroms, blocks, levels=(), compress=False, order="<"):
    """chroms: [(name, size)], ids in list order.  blocks: [[(chrom_id, start, end, rest)]] in file order.  levels: as
    write_bigwig_zoom_fixture.write_bigwig_zoom."""
    Z.write_bigwig_zoom(path, chroms, blocks, list(levels), compress=compress, order=order, magic=BIGBED_MAGIC, full_block=bed_block)


def blocks_of(records, per_block):
    return [records[k:k + per_block] for k in range(0, len(records), per_block)]


# ---- a gene-like track: nested and overlapping features, equal starts, zero-length records, two chromosomes in one block ----
GENES_A = [(0, 120, 980, "geneA\t900\t+"), (0, 120, 400, "geneA.t1\t0\t+"), (0, 120, 131, "geneA.e1\t10\t+"), (0, 125, 125, "snpA\t1\t."),
           (0, 200, 260, "geneA.e2\t10\t+"), (0, 240, 700, "geneB\t500\t-"), (0, 250, 251, "site\t3\t-"), (0, 300, 400, "geneA.e3\t10\t+"),
           (0, 399, 640, "geneC\t7\t+"), (0, 640, 640, "snpB\t1\t."), (0, 650, 700, "geneB.e1\t10\t-"), (0, 900, 980, "geneA.e4\t10\t+"),
           (0, 1500, 1522, "lone\t0\t+"), (0, 1510, 1800, "tail\t0\t-")]
GENES_B = [(1, 5, 300, "geneD\t100\t-"), (1, 5, 27, "geneD.e1\t1\t-"), (1, 40, 62, ""), (1, 61, 90, "plain\t0\t+"), (1, 280, 300, "geneD.e2\t1\t-")]
GENES_BLOCKS = [GENES_A[:6], GENES_A[6:11], GENES_A[11:] + GENES_B[:2], GENES_B[2:]]  # the third block holds both chromosomes

# ---- the issue's hand-written case: five records and one of a second chromosome in the same block ----
HAND_BLOCKS = [[(0, 0, 1000, "all"), (0, 3, 25, "a"), (0, 3, 10, "b"), (0, 7, 7, "zero"), (0, 20, 42, "c"), (1, 40, 62, "other")]]

# ---- the straddle track: 1000 bins of 40 bases from base 3, every bin under 4 - 8 overlapping records ----
STRADDLE_SEED = 11
STRADDLE_CASE = ("chrS", 3, 40021, 1000)  # step 40, a remainder of 18 bases


def straddle_records(seed=STRADDLE_SEED):
    """Records sorted by start, laid out against the bins of STRADDLE_CASE.  Over every bin edge lie two to four records of n
    bases, a of them on one side, with (n, a) among the pairs with n <= 40 whose weight n * (a / n) is NOT the integer a
    (22 * (15 / 22), ...); the other side's weight, n - a, is an integer.  Every bin is therefore the chain of 4 - 8 weights of
    overlapping records, about half of them not integers, small enough for their last bits to survive in the sum: the order of
    the chain shows.  Equal starts keep the order they were drawn in, so ends descend often."""
    rng = np.random.default_rng(seed)
    odd = sorted((n, a) for n in range(2, 41) for a in range(1, n) if n * (a / n) != a)
    assert len(odd) >= 10, odd
    _, first, _, _ = STRADDLE_CASE
    out = []
    for edge in range(first, first + 40 * 1001, 40):
        for _ in range(int(rng.integers(2, 5))):
            n, a = odd[int(rng.integers(len(odd)))]
            begin = edge - (n - a) if rng.random() < 0.5 else edge - a
            if begin >= 0:
                out.append((begin, begin + n))
    out.sort(key=lambda r: r[0])  # (stable)
    return [(0, s, e, "s%d" % i) for i, (s, e) in enumerate(out)]


# ---- a chromosome-long first record, then 1200 short ones with holes: chunks that are skipped between chunks that count ----
def long_records():
    rng = np.random.default_rng(5)
    out, at = [(0, 0, 200000, "chromosome")], 10
    for i in range(1200):
        at += int(rng.integers(0, 60)) + (20000 if i in (300, 900) else 0)
        out.append((0, at, at + int(rng.integers(0, 90)), "r%d" % i))
    return out


# ---- a file with zoom levels that contradict its records on purpose (a summary of 1000 per covered base, never 1) ----
ZOOM_BLOCKS = [[(0, 1000, 1400, "a"), (0, 1000, 1100, "a1"), (0, 3000, 3064, "b")], [(0, 9000, 9900, "c"), (0, 9100, 9200, "c1"), (1, 50, 90, "d")]]
ZOOM_LEVELS = [dict(reduction=16, records=Z.level_records(51, 0, 16, 1000, 120, gaps={40: 900, 80: 3000}, odd_lengths=True)
                    + Z.level_records(52, 1, 16, 48, 9), per_block=7, fanout=4),
               dict(reduction=64, records=Z.level_records(53, 0, 64, 960, 60, gaps={10: 1024}) + Z.level_records(54, 1, 64, 0, 3),
                    per_block=5, fanout=3)]

# name -> (chromosomes, blocks, zoom levels, compressed, byte order)
FIXTURES = {
    "genes.bb": ([("chrA", 2000), ("chrBB", 400)], GENES_BLOCKS, [], False, "<"),
    "genes.z.bb": ([("chrA", 2000), ("chrBB", 400)], GENES_BLOCKS, [], True, "<"),
    "genes.be.bb": ([("chrA", 2000), ("chrBB", 400)], GENES_BLOCKS, [], False, ">"),
    "hand.bb": ([("chrA", 1000), ("chrB", 100)], HAND_BLOCKS, [], False, "<"),
    "straddle.bb": ([("chrS", 50000)], blocks_of(straddle_records(), 300), [], True, "<"),
    "long.bb": ([("chrL", 200000)], blocks_of(long_records(), 256), [], True, "<"),
    "zoom.bb": ([("chrZ", 20000), ("chrY", 700)], ZOOM_BLOCKS, ZOOM_LEVELS, False, "<"),
}


def main(golden=os.path.join(HERE, "..", "tests", "golden", "bigbed")):
    os.makedirs(golden, exist_ok=True)
    for name, (chroms, blocks, levels, compress, order) in FIXTURES.items():
        path = os.path.join(golden, name)
        if not os.path.exists(path):
            write_bigbed(path, chroms, blocks, levels, compress=compress, order=order)
            print("wrote", path)


if __name__ == "__main__":
    main(*sys.argv[1:])
