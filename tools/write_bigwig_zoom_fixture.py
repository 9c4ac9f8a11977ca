#!/usr/bin/env python
"""
bigWig files WITH ZOOM LEVELS, for test fixtures only: tools/write_bigwig_fixture.py's full-data blocks and one-leaf index, and
per zoom level the 32-byte summary records in blocks of a chosen number of records under a real R-tree (a chosen number of
entries per node, as many tree levels as that takes).  A leaf entry runs from its block's first record (chromosome id, start) to
its last record's (chromosome id, end) -- the extremes, where the records are not in order -- so with blocks that cross
chromosomes the entries span chromosome ids, as in real files.  Zoom headers follow the file header (24 bytes each from offset
64); the levels are written in the order given, which need not be sorted.  That the reference's reader answers from these
levels (tools/record_zoom_golden.py) is the proof they are valid.

The records are NOT derived from the full data and need not agree with it: a file whose zoom levels disagree with its items
shows which of the two answered.

`FIXTURES` below is the definition of the small files under tests/golden/zoom; run as a script it writes the missing ones.

usage: write_bigwig_zoom_fixture.py [GOLDEN_DIR]
"""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import write_bigwig_fixture as W  # noqa: E402

NAN = float("nan")


def rtree_bytes(order, leaves, fanout, at):
    """The R-tree over `leaves` = [(start chrom, start base, end chrom, end base, offset, size)], its 48-byte header at file offset
    `at`, `fanout` entries per node."""
    nodes = [("leaf", leaves[k:k + fanout]) for k in range(0, len(leaves), fanout)] or [("leaf", [])]

    def extent(node):
        kind, items = node
        entries = items if kind == "leaf" else [extent(child) for child in items]
        lo, hi = min((e[0], e[1]) for e in entries), max((e[2], e[3]) for e in entries)
        return lo + hi

    while len(nodes) > 1:
        nodes = [("parent", nodes[k:k + fanout]) for k in range(0, len(nodes), fanout)]
    root = nodes[0]

    def size_of(node):
        kind, items = node
        return 4 + 32 * len(items) if kind == "leaf" else 4 + 24 * len(items) + sum(size_of(child) for child in items)

    def emit(node, off):
        kind, items = node
        out = struct.pack(order + "BBH", kind == "leaf", 0, len(items))
        if kind == "leaf":
            return out + b"".join(struct.pack(order + "IIIIQQ", *leaf) for leaf in items)
        child_at, below = off + 4 + 24 * len(items), b""
        for child in items:
            out += struct.pack(order + "IIIIQ", *(extent(child) + (child_at,)))
            below += emit(child, child_at)
            child_at += size_of(child)
        return out + below

    lo_hi = extent(root) if leaves else (0, 0, 0, 0)
    head = struct.pack(order + "IIQIIIIQII", W.CIRTREE_MAGIC, fanout, len(leaves), *lo_hi, at, 1, 0)
    return head + emit(root, at + 48)


def wiggle_block(order, block):
    """((start chrom, start base, end chrom, end base), bytes) of one full-data block of a bigWig file"""
    (chrom_id, first, last), raw = W.block_bytes(order, **block)
    return (chrom_id, first, chrom_id, last), raw


def write_bigwig_zoom(path, chroms, blocks, levels, compress=False, order="<", magic=W.BIGWIG_MAGIC, full_block=wiggle_block):
    """chroms, blocks: as write_bigwig_fixture.write_bigwig.  levels: [dict(reduction, records, per_block, fanout)] in file order,
    records = [(chrom_id, start, end, valid_count, min, max, sum, sum_squares)] in file order.  `magic` and `full_block` (what turns
    one entry of `blocks` into its leaf range and its bytes) are what tools/write_bigbed_fixture.py replaces to write bigBed."""
    key_size = max(len(name) for name, _ in chroms)
    tree = struct.pack(order + "IIIIQQ", W.BPT_MAGIC, len(chroms), key_size, 8, len(chroms), 0)
    tree += struct.pack(order + "BBH", 1, 0, len(chroms))
    for chrom_id, (name, size) in enumerate(chroms):
        tree += name.encode().ljust(key_size, b"\0") + struct.pack(order + "II", chrom_id, size)
    chrom_tree_offset = 64 + 24 * len(levels)
    data_offset = chrom_tree_offset + len(tree)
    body = struct.pack(order + "Q", len(blocks))  # everything from data_offset on
    biggest = 0

    def store(raw):
        nonlocal body, biggest
        biggest = max(biggest, len(raw))
        stored = zlib.compress(raw) if compress else raw
        at = data_offset + len(body)
        body += stored
        return at, len(stored)

    leaves = []
    for b in blocks:
        extent, raw = full_block(order, b)
        leaves.append(extent + store(raw))
    index_offset = data_offset + len(body)
    body += rtree_bytes(order, leaves, max(len(leaves), 1), index_offset)
    zoom_headers = b""
    for level in levels:
        records, per = level["records"], level["per_block"]
        zoom_data_offset = data_offset + len(body)
        body += struct.pack(order + "I", len(records))
        leaves = []
        for k in range(0, len(records), per):
            chunk = records[k:k + per]
            raw = b"".join(struct.pack(order + "IIIIffff", *r) for r in chunk)
            lo, hi = min((r[0], r[1]) for r in chunk), max((r[0], r[2]) for r in chunk)
            leaves.append(lo + hi + store(raw))
        zoom_index_offset = data_offset + len(body)
        body += rtree_bytes(order, leaves, level["fanout"], zoom_index_offset)
        zoom_headers += struct.pack(order + "IIQQ", level["reduction"], 0, zoom_data_offset, zoom_index_offset)
    header = struct.pack(order + "IHHQQQHHQQIQ", magic, 4, len(levels), chrom_tree_offset, data_offset, index_offset, 0, 0, 0, 0,
                         biggest if compress else 0, 0)
    assert len(header) == 64
    with open(path, "wb") as f:
        f.write(header + zoom_headers + tree + body)


def f32(x):
    return float(np.float32(x))


def level_records(seed, chrom_id, reduction, first, count, gaps=(), odd_lengths=False):
    """`count` records of `reduction` bases from `first` on, touching, except: before record k of `gaps` lie gaps[k] bases without
    data; with `odd_lengths` a record covers 3 .. reduction bases (overlap / length is then rarely exact).  valid_count <= length;
    sums with 24 significant bits, of mixed sign."""
    rng = np.random.default_rng(seed)
    out, at = [], first
    gaps = dict(gaps)
    for k in range(count):
        at += gaps.get(k, 0)
        length = int(rng.integers(3, reduction + 1)) if odd_lengths else reduction
        valid = int(rng.integers(1, length + 1))
        lo, hi = sorted(f32(x) for x in rng.normal(0.0, 2.0, size=2))
        total = f32(rng.normal(0.0, 1.0) * valid)
        out.append((chrom_id, at, at + length, valid, lo, hi, total, f32(abs(total) * rng.uniform(0.5, 3.0))))
        at += length if odd_lengths else reduction
    return out


BEDGRAPH = W.BEDGRAPH
# full data that the zoom levels contradict on purpose: one value, 1000, wherever there is any
LEAVES_FULL = [dict(chrom_id=0, kind=BEDGRAPH, items=[(1000, 1400, 1000.0), (3000, 3064, 1000.0), (9000, 9900, 1000.0)])]
# leaves of 7 records = 112 bases; gaps of 700 - 3000 bases, wider than a leaf, so that the front record of a bin that lies in a
# gap is the first one behind the gap: it gives min and max without overlapping the bin
LEAVES_16 = level_records(11, 0, 16, 1000, 301, gaps={40: 900, 41: 700, 120: 3000, 200: 1500, 201: 16, 290: 2048}, odd_lengths=True)
LEAVES_64 = level_records(12, 0, 64, 960, 90, gaps={10: 1024, 50: 4096})

CHROMS_FULL = [dict(chrom_id=0, kind=BEDGRAPH, items=[(0, 40, 1000.0)]), dict(chrom_id=1, kind=BEDGRAPH, items=[(100, 160, 1000.0)]),
               dict(chrom_id=2, kind=BEDGRAPH, items=[(8, 16, 1000.0)])]
CHROMS_8 = (level_records(21, 0, 8, 0, 23, gaps={9: 64}) + level_records(22, 1, 8, 96, 17, gaps={5: 40}, odd_lengths=True)
            + level_records(23, 2, 8, 8, 26, gaps={20: 200}))
CHROMS_32 = level_records(24, 0, 32, 0, 6) + level_records(25, 1, 32, 96, 5) + level_records(26, 2, 32, 0, 7)

BIG = f32(3.0e38)
ODD_FULL = [dict(chrom_id=0, kind=BEDGRAPH, items=[(0, 500, 1000.0)])]
# valid_count above 2^24 (its product with the factor is not exact even in float64), lengths 7, 11, 13 (overlap / length inexact),
# NaN min and max at the front of a run and inside it, two sums whose float32 sum overflows
ODD_10_FIRST = [(0, 0, 7, 16777217, -1.0, 1.0, f32(0.1), f32(0.7)), (0, 7, 18, 33554435, NAN, NAN, f32(1.3), f32(2.9)),
                (0, 18, 31, 50331653, -2.5, 0.5, f32(-7.7), f32(60.1)), (0, 31, 44, 16777219, -0.5, NAN, BIG, BIG),
                (0, 44, 51, 4000000001, NAN, 3.0, BIG, BIG), (0, 51, 62, 7, -4.0, 4.0, f32(-1e-3), f32(1e-6)),
                (0, 100, 113, 20000003, NAN, NAN, f32(5.5), f32(31.0)), (0, 113, 120, 3, -9.0, -8.0, f32(-25.5), f32(217.0)),
                (0, 120, 131, 11, 0.25, 0.5, f32(4.1), f32(1.6)), (0, 131, 144, 13, -BIG, BIG, -BIG, BIG), (0, 144, 157, 13, -1.0, 1.0, -BIG, BIG)]
ODD_10_FIRST += level_records(31, 0, 10, 200, 30, odd_lengths=True)
ODD_10_SECOND = level_records(32, 0, 10, 0, 50)  # the same reduction again, later in the file: never chosen
ODD_40 = level_records(33, 0, 40, 0, 12, odd_lengths=True)

UNORDERED_FULL = [dict(chrom_id=0, kind=BEDGRAPH, items=[(0, 100, 1.0)])]
UNORDERED_8 = level_records(41, 0, 8, 0, 20)[::-1]

# name -> (chromosomes, full-data blocks, zoom levels in file order, compressed, byte order)
FIXTURES = {
    "leaves.bw": ([("chrL", 20000)], LEAVES_FULL, [dict(reduction=16, records=LEAVES_16, per_block=7, fanout=4),
                                                  dict(reduction=64, records=LEAVES_64, per_block=7, fanout=4)], True, "<"),
    "chroms.bw": ([("chrA", 400), ("chrB", 400), ("chrC", 600)], CHROMS_FULL, [dict(reduction=8, records=CHROMS_8, per_block=7, fanout=3),
                                                                              dict(reduction=32, records=CHROMS_32, per_block=4, fanout=3)], False, ">"),
    "odd.bw": ([("chrO", 1000)], ODD_FULL, [dict(reduction=40, records=ODD_40, per_block=5, fanout=4),
                                            dict(reduction=10, records=ODD_10_FIRST, per_block=6, fanout=4),
                                            dict(reduction=10, records=ODD_10_SECOND, per_block=6, fanout=4)], True, "<"),
    "unordered.z.bw": ([("chrU", 200)], UNORDERED_FULL, [dict(reduction=8, records=UNORDERED_8, per_block=6, fanout=3)], False, "<"),
}


def main(golden=os.path.join(HERE, "..", "tests", "golden", "zoom")):
    os.makedirs(golden, exist_ok=True)
    for name, (chroms, blocks, levels, compress, order) in FIXTURES.items():
        path = os.path.join(golden, name)
        if not os.path.exists(path):
            write_bigwig_zoom(path, chroms, blocks, levels, compress=compress, order=order)
            print("wrote", path)


if __name__ == "__main__":
    main(*sys.argv[1:])
