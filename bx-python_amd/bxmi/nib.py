"""
Reader of nib files (what the reference's bx.seq.nib.NibFile accepts, lib/bx/seq/nib.py:9-50): one sequence, four bits per base.

    offset 0: magic 0x6BE93D3A read big-endian (0x3A3DE96B: the file is little-endian)
    offset 4: the number of bases, 32 bits in the file's byte order
    offset 8: (size + 1) // 2 bytes, the first base of a byte in its high nibble: codes 0-3 = T C A G, 4 = N, 5-7 = what the
              reference prints as X (_nib.pyx:20-21), bit 3 = lower case

The nibble bytes go to the device as they are (bxmi.sequence.TwoBitTrack.from_nib): the byte order concerns the length alone.
"""
import struct

import numpy as np

MAGIC = 0x6BE93D3A
MAGIC_SWAP = 0x3A3DE96B


def read_file(path=None, data=None):
    """(size, uint8 nibble bytes [(size + 1) // 2], byte_order ">" or "<") of a nib file (`path`, or `data`: its bytes)"""
    if data is None:
        with open(path, "rb") as f:
            data = f.read()
    data = bytes(data)
    magic = struct.unpack(">L", data[:4])[0] if len(data) >= 4 else None
    if magic == MAGIC:
        byte_order = ">"
    elif magic == MAGIC_SWAP:
        byte_order = "<"
    else:
        raise Exception("Not a NIB file")  # (the reference's words)
    if len(data) < 8:
        raise ValueError("nib file is truncated")
    size = struct.unpack(byte_order + "L", data[4:8])[0]
    nibbles = np.frombuffer(data, dtype=np.uint8, offset=8)[:(size + 1) // 2]
    if len(nibbles) != (size + 1) // 2:
        raise ValueError("nib file is truncated")
    return size, nibbles, byte_order
