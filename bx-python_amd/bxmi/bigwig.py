"""
bigWig -> per-chromosome span arrays on the host, in plain Python (``struct`` + ``zlib``): what ``BigWigFile.get_as_array``
(lib/bx/bbi/bigwig_file.pyx:46-88, 122-137, 200-211) would assign position by position, collected for ``ScoreTrack.set_spans``
in the shape ``bxmi.wiggle.read_spans_file`` returns: {chrom: (starts, ends, values)}, int32 / int32 / float32, in file order
(a later span overwrites an earlier one, as the reference's assignment does).

Read: the header in either byte order (fields in the order of lib/bx/bbi/bbi_file.pyx:138-152), the chromosome B+ tree (names,
ids, sizes; bpt_file.pyx), the R-tree over the full-resolution data (cirtree_file.pyx) leaf by leaf, left to right, and the
three kinds of data block: bedGraph (1), variableStep (2), fixedStep (3), inflated when ``uncompress_buf_size > 0``.  As in the
reference, item i of a fixedStep block starts at ``block start + i * span`` (its ``step`` field is read and not used), and a
block of another kind contributes nothing.  ``zoom_reductions`` reads the zoom headers' reduction levels (what the reference's
choice between a zoom level and the full data depends on); ``read_zoom_file`` reads the levels themselves: every level's R-tree
in the reference's traversal order and the 32-byte summary records of its blocks (bbi_file.pyx:304-353), per chromosome, with
the leaf entries that decide which records the reference loads for a region.  ``chroms``, ``read_spans_file``,
``zoom_reductions`` and ``read_zoom_file`` take a path, or ``data=`` the file's bytes already in memory.
"""
import collections
import struct
import zlib

import numpy as np

BIGWIG_MAGIC = 0x888FFC26
BIGBED_MAGIC = 0x8789F2EB
BPT_MAGIC = 0x78CA8C91
CIRTREE_MAGIC = 0x2468ACE0
BEDGRAPH, VARIABLE_STEP, FIXED_STEP = 1, 2, 3


def byte_order(head, magic=BIGWIG_MAGIC):
    """'<' or '>' when the first four bytes are the bigWig magic number (or `magic`) in that order, else None."""
    if len(head) >= 4:
        for order in (">", "<"):
            if struct.unpack(order + "I", head[:4])[0] == magic:
                return order
    return None


def is_bigwig(path):
    with open(path, "rb") as f:
        return byte_order(f.read(4)) is not None


_KIND = {BIGWIG_MAGIC: "bigWig", BIGBED_MAGIC: "bigBed"}


class _Header:
    """The 64-byte header of a file of the kind `magic` names (bigWig unless bxmi.bigbed asks for bigBed)."""

    def __init__(self, data, magic=BIGWIG_MAGIC):
        self.kind = _KIND[magic]
        order = byte_order(data, magic)
        if order is None:
            found = data[:4]
            other = BIGBED_MAGIC if magic == BIGWIG_MAGIC else BIGWIG_MAGIC
            if byte_order(found, other) is not None:
                raise ValueError("a %s file, not a %s file" % (_KIND[other], self.kind))
            raise ValueError("not a %s file: bad magic number %r" % (self.kind, found.hex()))
        if len(data) < 64:
            raise ValueError("not a %s file: the header is cut short" % self.kind)
        self.order = order
        (self.version, self.zoom_levels, self.chrom_tree_offset, self.unzoomed_data_offset, self.unzoomed_index_offset, self.field_count,
         self.defined_field_count, self.as_offset, self.total_summary_offset, self.uncompress_buf_size) = struct.unpack_from(order + "HHQQQHHQQI", data, 4)


def _sub_order(data, at, magic, what):
    for order in (">", "<"):
        if struct.unpack_from(order + "I", data, at)[0] == magic:
            return order
    raise ValueError("bigWig file: bad magic number of the %s at offset %d" % (what, at))


def _chrom_tree(data, at):
    """[(name, id, size)] of the B+ tree at `at`, leaves left to right."""
    order = _sub_order(data, at, BPT_MAGIC, "chromosome tree")
    block_size, key_size, value_size, item_count = struct.unpack_from(order + "IIIQ", data, at + 4)
    if value_size != 8:
        raise ValueError("bigWig file: chromosome tree values of %d bytes (8 expected)" % value_size)
    out = []

    def walk(off):
        is_leaf, _, count = struct.unpack_from(order + "BBH", data, off)
        off += 4
        for _ in range(count):
            key = data[off:off + key_size]
            if is_leaf:
                chrom_id, size = struct.unpack_from(order + "II", data, off + key_size)
                out.append((key.rstrip(b"\0").decode(), chrom_id, size))
            else:
                walk(struct.unpack_from(order + "Q", data, off + key_size)[0])
            off += key_size + 8

    walk(at + 32)
    return out


def _leaf_blocks(data, at):
    """[(offset, size)] of every data block the R-tree at `at` lists, leaves left to right."""
    order = _sub_order(data, at, CIRTREE_MAGIC, "R-tree")
    out = []

    def walk(off):
        is_leaf, _, count = struct.unpack_from(order + "BBH", data, off)
        off += 4
        for _ in range(count):
            if is_leaf:
                out.append(struct.unpack_from(order + "QQ", data, off + 16))
                off += 32
            else:
                walk(struct.unpack_from(order + "Q", data, off + 16)[0])
                off += 24

    walk(at + 48)
    return out


def _block_spans(block, order):
    """(chrom id, starts, ends, values) of one inflated data block"""
    chrom_id, b_start, _b_end, _step, span, kind, _, count = struct.unpack_from(order + "IIIIIBBH", block, 0)
    if kind == BEDGRAPH:
        rec = np.frombuffer(block, dtype=np.dtype([("s", order + "u4"), ("e", order + "u4"), ("v", order + "f4")]), count=count, offset=24)
        return chrom_id, rec["s"].astype(np.int64), rec["e"].astype(np.int64), rec["v"].astype(np.float32)
    if kind == VARIABLE_STEP:
        rec = np.frombuffer(block, dtype=np.dtype([("s", order + "u4"), ("v", order + "f4")]), count=count, offset=24)
        s = rec["s"].astype(np.int64)
        return chrom_id, s, s + span, rec["v"].astype(np.float32)
    if kind == FIXED_STEP:
        v = np.frombuffer(block, dtype=order + "f4", count=count, offset=24).astype(np.float32)
        s = b_start + np.arange(count, dtype=np.int64) * span
        return chrom_id, s, s + span, v
    empty = np.zeros(0, dtype=np.int64)
    return chrom_id, empty, empty, np.zeros(0, dtype=np.float32)


def _read(path, data=None, magic=BIGWIG_MAGIC):
    if data is None:
        with open(path, "rb") as f:
            data = f.read()
    return data, _Header(data, magic)


def zoom_reductions(path=None, data=None):
    """[reduction_level] of the zoom headers (bbi_file.pyx:156-164: 24 bytes each from offset 64), in file order."""
    return _zoom_reductions(*_read(path, data))


def _zoom_reductions(data, h):
    if len(data) < 64 + 24 * h.zoom_levels:
        raise ValueError("not a %s file: the zoom headers are cut short" % h.kind)
    return [struct.unpack_from(h.order + "I", data, 64 + 24 * i)[0] for i in range(h.zoom_levels)]


def chroms(path=None, data=None):
    """{name: size} of the file's chromosomes, in the order of the chromosome tree."""
    data, h = _read(path, data)
    return {name: size for name, _, size in _chrom_tree(data, h.chrom_tree_offset)}


def read_spans_file(path=None, data=None):
    """{chrom: (starts int32, ends int32, values float32)} of the full-resolution data, spans in file order.  A chromosome
    without data has empty arrays.  Raises ValueError for a file that is not bigWig (bigBed included)."""
    data, h = _read(path, data)
    tree = _chrom_tree(data, h.chrom_tree_offset)
    by_id = {chrom_id: name for name, chrom_id, _ in tree}
    per = {name: ([], [], []) for name, _, _ in tree}
    for offset, size in _leaf_blocks(data, h.unzoomed_index_offset):
        block = data[offset:offset + size]
        if h.uncompress_buf_size > 0:
            block = zlib.decompress(block)
        chrom_id, s, e, v = _block_spans(block, h.order)
        name = by_id.get(chrom_id)
        if name is None:
            raise ValueError("bigWig file: a data block of chromosome id %d, which the chromosome tree does not list" % chrom_id)
        lists = per[name]
        lists[0].append(s), lists[1].append(e), lists[2].append(v)
    out = {}
    for name, (s, e, v) in per.items():
        s = np.concatenate(s) if s else np.zeros(0, dtype=np.int64)
        e = np.concatenate(e) if e else np.zeros(0, dtype=np.int64)
        if len(e) and e.max() > 2147483647:
            raise ValueError("bigWig file: a span of %s ends beyond 2^31 - 1" % name)
        out[name] = (s.astype(np.int32), e.astype(np.int32), np.concatenate(v) if v else np.zeros(0, dtype=np.float32))
    return out


# One chromosome's part of one zoom level.  start .. sumsq: its summary records in LOAD ORDER (leaves in the order the reference's
# traversal meets them, records in block order).  leaf_lo / leaf_hi: the base range of every leaf entry that holds one of them,
# as the reference's overlap test sees it for this chromosome (-1: the entry starts on an earlier chromosome; 2^31-1: it ends on a
# later one, or beyond 2^31-1); leaf k holds records [leaf_first[k], leaf_first[k + 1]).  A region [s, e) loads the records of
# every leaf with  s < leaf_hi and e > leaf_lo  (cirtree_file.pyx:5-20, 64-77), whole.
ZoomArrays = collections.namedtuple("ZoomArrays", "start end valid min max sum sumsq leaf_lo leaf_hi leaf_first")
ZOOM_RECORD = 32
INT32_MAX = 2147483647


def _zoom_leaves(data, at):
    """[(start chrom, start base, end chrom, end base, offset, size)] of the leaf entries of the R-tree at `at`, in the order of
    the reference's traversal (r_find_overlapping: depth first, children in node order).  That traversal visits a leaf only
    through parents that overlap the query too, so the leaf test alone decides exactly when every child lies inside its
    parent's range: a child that does not raises ValueError."""
    order = _sub_order(data, at, CIRTREE_MAGIC, "R-tree of a zoom level")
    out = []

    def walk(off, parent):
        is_leaf, _, count = struct.unpack_from(order + "BBH", data, off)
        off += 4
        for _ in range(count):
            sc, sb, ec, eb = struct.unpack_from(order + "IIII", data, off)
            if parent is not None and ((sc, sb) < parent[:2] or (ec, eb) > parent[2:]):
                raise ValueError("bigWig file: an R-tree entry (%d, %d)-(%d, %d) is not contained in its parent's range (%d, %d)-(%d, %d)"
                                 % ((sc, sb, ec, eb) + parent))
            if is_leaf:
                out.append((sc, sb, ec, eb) + struct.unpack_from(order + "QQ", data, off + 16))
                off += 32
            else:
                walk(struct.unpack_from(order + "Q", data, off + 16)[0], (sc, sb, ec, eb))
                off += 24

    walk(at + 48, None)
    return out


def ordered_level(z):
    """None when the level part `z` (ZoomArrays) is ORDERED -- record starts and ends both non-decreasing, leaf_lo and leaf_hi both
    non-decreasing, start <= end everywhere -- which is what the device takes (bxmi_zoom_create); else the first condition that
    fails, in words."""
    for name, a in (("record starts", z.start), ("record ends", z.end), ("leaf_lo", z.leaf_lo), ("leaf_hi", z.leaf_hi)):
        if len(a) > 1 and np.any(np.diff(a.astype(np.int64)) < 0):
            return "%s are not non-decreasing" % name
    if np.any(z.start > z.end):
        return "a record has start > end"
    return None


def read_zoom_file(path=None, data=None):
    """[(reduction_level, {chrom: ZoomArrays})] of the file's zoom levels, in file order; every chromosome of the chromosome tree
    is listed (empty arrays where a level has nothing for it).  start, end, leaf_lo, leaf_hi: int32; valid: uint32; min, max, sum,
    sumsq: float32; leaf_first: int64, n_leaves + 1 offsets.  Records of a chromosome in a leaf whose entry does not reach that
    chromosome can never be loaded and are left out, like leaves without a record of the chromosome.  Raises ValueError for a
    record beyond 2^31 - 1, a block that is not whole records, or an R-tree whose children leave their parents."""
    return _read_zoom(*_read(path, data))


def _read_zoom(data, h):
    """read_zoom_file's body; bigBed zoom levels have the same format (bxmi.bigbed.read_zoom_file)"""
    if len(data) < 64 + 24 * h.zoom_levels:
        raise ValueError("not a %s file: the zoom headers are cut short" % h.kind)
    tree = _chrom_tree(data, h.chrom_tree_offset)
    rec = np.dtype([(k, h.order + t) for k, t in (("chrom", "u4"), ("start", "u4"), ("end", "u4"), ("valid", "u4"), ("min", "f4"), ("max", "f4"),
                                                  ("sum", "f4"), ("sumsq", "f4"))])
    levels = []
    for i in range(h.zoom_levels):
        reduction, _, _, index_offset = struct.unpack_from(h.order + "IIQQ", data, 64 + 24 * i)
        per = {chrom_id: ([], [], [], [0]) for _, chrom_id, _ in tree}  # record arrays, leaf_lo, leaf_hi, leaf_first
        for sc, sb, ec, eb, offset, size in _zoom_leaves(data, index_offset):
            block = data[offset:offset + size]
            if h.uncompress_buf_size > 0:
                block = zlib.decompress(block)
            if len(block) % ZOOM_RECORD:
                raise ValueError("bigWig file: a zoom block of %d bytes is not whole summary records" % len(block))
            records = np.frombuffer(block, dtype=rec)
            for chrom_id in np.unique(records["chrom"]):
                chrom_id = int(chrom_id)
                if chrom_id not in per or not sc <= chrom_id <= ec:
                    continue
                mine = records[records["chrom"] == chrom_id]
                if max(int(mine["end"].max()), int(mine["start"].max())) > INT32_MAX:
                    raise ValueError("bigWig file: a zoom record of chromosome id %d ends beyond 2^31 - 1" % chrom_id)
                arrays, lo, hi, first = per[chrom_id]
                arrays.append(mine)
                lo.append(-1 if sc < chrom_id else min(sb, INT32_MAX))
                hi.append(INT32_MAX if ec > chrom_id else min(eb, INT32_MAX))
                first.append(first[-1] + len(mine))
        out = {}
        for name, chrom_id, _ in tree:
            arrays, lo, hi, first = per[chrom_id]
            r = np.concatenate(arrays) if arrays else np.zeros(0, dtype=rec)
            out[name] = ZoomArrays(r["start"].astype(np.int32), r["end"].astype(np.int32), r["valid"].astype(np.uint32),
                                   *[r[k].astype(np.float32) for k in ("min", "max", "sum", "sumsq")],
                                   np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), np.array(first, dtype=np.int64))
        levels.append((reduction, out))
    return levels
