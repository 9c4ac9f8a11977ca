#!/usr/bin/env python
"""
A minimal bigWig writer, for test fixtures only: the header, the chromosome B+ tree as one leaf, the data blocks of a chosen
kind (bedGraph 1, variableStep 2, fixedStep 3), compressed or not, and an R-tree of one leaf that lists every block; no zoom
levels, no total summary.  Nothing in the reference writes bigWig, so this is where bedGraph and fixedStep blocks and a
big-endian file come from; that the reference's reader reads them (tools/record_profile_golden.py) is the proof they are valid.

`FIXTURES` below is the definition of the small files under tests/golden/profile; run as a script it writes the missing ones,
a bed-style wiggle twin of bg.bw included (the same track for bxmi.wiggle).

usage: write_bigwig_fixture.py [GOLDEN_DIR]
"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

BIGWIG_MAGIC, BPT_MAGIC, CIRTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
BEDGRAPH, VARIABLE_STEP, FIXED_STEP = 1, 2, 3


def block_bytes(order, chrom_id, kind, items, start=0, step=0, span=0):
    """One data block.  items: bedGraph (start, end, value), variableStep (start, value), fixedStep value."""
    if kind == BEDGRAPH:
        first, last = items[0][0], max(e for _, e, _ in items)
        body = b"".join(struct.pack(order + "IIf", s, e, v) for s, e, v in items)
    elif kind == VARIABLE_STEP:
        first, last = items[0][0], max(s for s, _ in items) + span
        body = b"".join(struct.pack(order + "If", s, v) for s, v in items)
    else:
        first, last = start, start + (len(items) - 1) * step + span
        body = b"".join(struct.pack(order + "f", v) for v in items)
    head = struct.pack(order + "IIIIIBBH", chrom_id, first, last, step, span, kind, 0, len(items))
    return (chrom_id, first, last), head + body


def write_bigwig(path, chroms, blocks, compress=False, order="<"):
    """chroms: [(name, size)], ids in list order.  blocks: [dict(chrom_id, kind, items[, start, step, span])] in file order."""
    key_size = max(len(name) for name, _ in chroms)
    tree = struct.pack(order + "IIIIQQ", BPT_MAGIC, len(chroms), key_size, 8, len(chroms), 0)
    tree += struct.pack(order + "BBH", 1, 0, len(chroms))
    for chrom_id, (name, size) in enumerate(chroms):
        tree += name.encode().ljust(key_size, b"\0") + struct.pack(order + "II", chrom_id, size)
    chrom_tree_offset = 64
    data_offset = chrom_tree_offset + len(tree)
    data = struct.pack(order + "Q", len(blocks))
    leaves, biggest = [], 0
    for b in blocks:
        (chrom_id, first, last), raw = block_bytes(order, **b)
        biggest = max(biggest, len(raw))
        stored = zlib.compress(raw) if compress else raw
        leaves.append((chrom_id, first, chrom_id, last, data_offset + len(data), len(stored)))
        data += stored
    index_offset = data_offset + len(data)
    lo, hi = min((l[0], l[1]) for l in leaves), max((l[2], l[3]) for l in leaves)
    index = struct.pack(order + "IIQIIIIQII", CIRTREE_MAGIC, len(leaves), len(leaves), lo[0], lo[1], hi[0], hi[1], index_offset, 1, 0)
    index += struct.pack(order + "BBH", 1, 0, len(leaves))
    for leaf in leaves:
        index += struct.pack(order + "IIIIQQ", *leaf)
    header = struct.pack(order + "IHHQQQHHQQIQ", BIGWIG_MAGIC, 4, 0, chrom_tree_offset, data_offset, index_offset, 0, 0, 0, 0,
                         biggest if compress else 0, 0)
    assert len(header) == 64
    with open(path, "wb") as f:
        f.write(header + tree + data + index)


def f32(x):
    return float(np.float32(x))


# bedGraph: gaps, overlaps (the later span wins), zeros of both signs, a denormal, an item that is empty, a second block
BG_BLOCKS = [
    dict(chrom_id=0, kind=BEDGRAPH, items=[(3, 10, 1.5), (10, 12, 0.0), (12, 15, -0.0), (20, 40, f32(0.001)), (30, 35, -2.25), (50, 50, 9.0),
                                           (60, 61, 1e-45), (70, 130, f32(0.3))]),
    dict(chrom_id=0, kind=BEDGRAPH, items=[(125, 140, 7.0), (200, 260, f32(1e30)), (260, 300, f32(-1e30)), (390, 400, 0.125)]),
]
# fixedStep: span == step, span < step (the reference places item i at start + i * span, whatever the step), span > 1
FS_BLOCKS = [
    dict(chrom_id=0, kind=FIXED_STEP, start=5, step=1, span=1, items=[f32(0.1 * k) for k in range(1, 70)]),
    dict(chrom_id=0, kind=FIXED_STEP, start=100, step=5, span=2, items=[1.0, 2.0, 3.0, 4.0]),
    dict(chrom_id=0, kind=FIXED_STEP, start=150, step=3, span=3, items=[-1.0, 0.5, 0.25, 1e-40, 8.0]),
]
# two chromosomes, every kind of block, the second chromosome's blocks around the first one's in the file
TWO_BLOCKS = [
    dict(chrom_id=0, kind=VARIABLE_STEP, span=2, items=[(0, 1.0), (4, 2.0), (5, 3.0), (90, f32(0.7))]),
    dict(chrom_id=1, kind=BEDGRAPH, items=[(0, 30, f32(0.25)), (30, 45, 4.0)]),
    dict(chrom_id=0, kind=FIXED_STEP, start=20, step=1, span=1, items=[f32(k / 8.0) for k in range(40)]),
    dict(chrom_id=1, kind=VARIABLE_STEP, span=1, items=[(44, -4.0), (46, f32(1e-3)), (49, 6.5)]),
]

# name -> (chromosomes, blocks, compressed, byte order)
FIXTURES = {
    "bg.bw": ([("chr1", 400)], BG_BLOCKS, False, "<"),
    "bg.z.bw": ([("chr1", 400)], BG_BLOCKS, True, "<"),
    "fs.bw": ([("chrF", 250)], FS_BLOCKS, False, "<"),
    "fs.z.bw": ([("chrF", 250)], FS_BLOCKS, True, "<"),
    "two.z.bw": ([("chrA", 100), ("chrBB", 50)], TWO_BLOCKS, True, "<"),
    "two.be.bw": ([("chrA", 100), ("chrBB", 50)], TWO_BLOCKS, False, ">"),
}

# window centres come from these rows ((start + end) // 2); some windows hang off an end of their chromosome, none starts
# below zero or names an unknown chromosome (the reference crashes on both)
BEDS = {
    "bg.bed": "".join("chr1\t%d\t%d\n" % (s, e) for s, e in [(60, 80), (100, 101), (30, 31), (250, 270), (380, 420), (200, 330), (8, 92), (61, 62)]),
    "fs.bed": "".join("chrF\t%d\t%d\tname\t0\t+\n" % (s, e) for s, e in [(20, 40), (100, 120), (150, 170), (240, 250), (60, 61), (30, 30)]),
    "two.bed": "".join("%s\t%d\t%d\n" % r for r in [("chrA", 20, 40), ("chrBB", 30, 50), ("chrA", 50, 60), ("chrBB", 40, 41), ("chrA", 90, 100),
                                                     ("chrBB", 20, 30), ("chrA", 24, 25)]),
    "gap.bed": "chr1\t310\t330\nchr1\t316\t320\n",  # around a stretch without data: columns that print nan
    "test.bed": "".join("chr1\t%d\t%d\n" % (s, s + 10) for s in range(10900, 20900, 137)),
}


def bed_style_wiggle(blocks, chrom):
    """The bedGraph blocks as bed-style wiggle lines (values as repr of the float32's double: they round back to it)."""
    lines = ["track type=wiggle_0 name=twin\n"]
    for b in blocks:
        lines += ["%s\t%d\t%d\t%r\n" % (chrom, s, e, f32(v)) for s, e, v in b["items"]]
    return "".join(lines)


def main(golden=os.path.join(HERE, "..", "tests", "golden", "profile")):
    os.makedirs(golden, exist_ok=True)
    for name, (chroms, blocks, compress, order) in FIXTURES.items():
        path = os.path.join(golden, name)
        if not os.path.exists(path):
            write_bigwig(path, chroms, blocks, compress=compress, order=order)
            print("wrote", path)
    texts = dict(BEDS)
    texts["bg.wig"] = bed_style_wiggle(BG_BLOCKS, "chr1")
    for name, text in texts.items():
        path = os.path.join(golden, name)
        if not os.path.exists(path):
            with open(path, "w") as f:
                f.write(text)
            print("wrote", path)


if __name__ == "__main__":
    main(*sys.argv[1:])
