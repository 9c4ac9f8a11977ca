"""
bigBed -> per-chromosome record arrays on the host, in plain Python (``struct`` + ``zlib``), beside ``bxmi.bigwig`` and on its
helpers: what ``BigBedFile``'s block handlers (lib/bx/bbi/bigbed_file.pyx:27-55) meet, record by record, collected for
``bxmi.summary.BedTrack`` and for ``bx.bbi.bigbed_file.BigBedFile.get``.

A bigBed file is a bigWig file with another magic number and other data blocks: the header, the chromosome B+ tree, the zoom
headers, the zoom levels (the same 32-byte summary records under the same R-trees) and the R-tree over the full data are read by
``bxmi.bigwig``'s code.  A data block is a run of records ``(uint32 chrom_id, uint32 start, uint32 end, NUL-terminated rest)``;
one block may hold records of several chromosomes.  ``read_items_file`` reads the blocks leaf by leaf, left to right -- the order
in which the reference visits them -- inflates them when ``uncompress_buf_size > 0`` and splits them per record by chromosome id.

Every function takes a path, or ``data=`` the file's bytes already in memory, and raises ValueError for a file that is not
bigBed (a bigWig file: "a bigWig file, not a bigBed file"), a cut-short file, a record beyond 2^31 - 1 and a chromosome id that
the chromosome tree does not list.
"""
import struct
import zlib

import numpy as np

from . import bigwig
from .bigwig import BIGBED_MAGIC, INT32_MAX


def byte_order(head):
    """'<' or '>' when the first four bytes are the bigBed magic number in that order, else None."""
    return bigwig.byte_order(head, BIGBED_MAGIC)


def is_bigbed(path):
    with open(path, "rb") as f:
        return byte_order(f.read(4)) is not None


def _read(path, data=None):
    return bigwig._read(path, data, BIGBED_MAGIC)


def _whole(read, *args):
    """`read(*args)`, a cut-short or damaged file reported as ValueError"""
    try:
        return read(*args)
    except (struct.error, zlib.error, IndexError) as err:
        raise ValueError("not a bigBed file: cut short or damaged (%s)" % err)


def chroms(path=None, data=None):
    """{name: size} of the file's chromosomes, in the order of the chromosome tree."""
    data, h = _read(path, data)
    return {name: size for name, _, size in _whole(bigwig._chrom_tree, data, h.chrom_tree_offset)}


def zoom_reductions(path=None, data=None):
    """[reduction_level] of the zoom headers, in file order."""
    return bigwig._zoom_reductions(*_read(path, data))


def read_zoom_file(path=None, data=None):
    """[(reduction_level, {chrom: bigwig.ZoomArrays})] of the file's zoom levels, as bxmi.bigwig.read_zoom_file."""
    return _whole(bigwig._read_zoom, *_read(path, data))


def _block_records(block, order):
    """[(chrom id, start, end, rest bytes)] of one inflated data block, in block order"""
    out, at, head = [], 0, struct.Struct(order + "III")
    while at < len(block):
        chrom_id, s, e = head.unpack_from(block, at)
        nul = block.find(b"\0", at + 12)
        if nul < 0:
            raise ValueError("bigBed file: a record without its terminating NUL")
        out.append((chrom_id, s, e, block[at + 12:nul]))
        at = nul + 1
    return out


def _items(data, h):
    tree = bigwig._chrom_tree(data, h.chrom_tree_offset)
    by_id = {chrom_id: name for name, chrom_id, _ in tree}
    per = {name: ([], [], []) for name, _, _ in tree}
    for offset, size in bigwig._leaf_blocks(data, h.unzoomed_index_offset):
        block = data[offset:offset + size]
        if len(block) < size:
            raise ValueError("not a bigBed file: a data block is cut short")
        if h.uncompress_buf_size > 0:
            block = zlib.decompress(block)
        for chrom_id, s, e, rest in _block_records(block, h.order):
            name = by_id.get(chrom_id)
            if name is None:
                raise ValueError("bigBed file: a record of chromosome id %d, which the chromosome tree does not list" % chrom_id)
            if s > INT32_MAX or e > INT32_MAX:
                raise ValueError("bigBed file: a record of %s lies beyond 2^31 - 1" % name)
            lists = per[name]
            lists[0].append(s), lists[1].append(e), lists[2].append(rest.decode())
    return {name: (np.array(s, dtype=np.int32), np.array(e, dtype=np.int32), rest) for name, (s, e, rest) in per.items()}


def read_items_file(path=None, data=None):
    """{chrom: (starts int32, ends int32, rest)} of the full-resolution data, records in file order; `rest` is a list of str, one
    per record: the record's remaining BED columns, tab-separated ("" when it has none).  A chromosome without records has empty
    arrays."""
    return _whole(_items, *_read(path, data))
