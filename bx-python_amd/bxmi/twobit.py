"""
Reader of .2bit files (the format of UCSC's twoBit tools; what the reference's bx.seq.twobit.TwoBitFile accepts,
lib/bx/seq/twobit.py:59-136): per-sequence numpy arrays, read when asked for, for bxmi.sequence to put on the device.

Layout, every integer 32 bits in the file's byte order:
    magic 0x1A412743 (read big-endian; 0x4327411A means the file is little-endian), version (0), sequence count, reserved;
    the index: per sequence a length byte, the name, the offset of its record;
    a record: size; N block count, starts[], sizes[]; mask block count, starts[], sizes[]; reserved; (size + 3) // 4 packed bytes,
    4 bases per byte, the first base in the two most significant bits, codes T=0 C=1 A=2 G=3.
"""
import collections
import contextlib
import io
import struct

import numpy as np

MAGIC = 0x1A412743
MAGIC_SWAP = 0x4327411A
VERSION = 0

# size: bases; n_starts / n_sizes, m_starts / m_sizes: the N and the mask blocks (uint32 as in the file); packed: uint8[(size + 3) // 4]
Sequence = collections.namedtuple("Sequence", "size n_starts n_sizes m_starts m_sizes packed")


class TwoBitReader:
    """The index of a .2bit file; `load(name)` reads one sequence's arrays (each name once: they are kept), `load_all()` all of
    them in file order.  `source`: a path, bytes, or a binary file object that can seek.  Only the header and the index are read
    when the reader is made; a sequence's record is sought and read when it is loaded, so one chromosome of a genome costs that
    chromosome's bytes.  A path is opened for each read and closed again; a file object is the caller's and must stay open for as
    long as sequences are loaded from it, as the reference's TwoBitFile requires.  A file that ends before what its header, its
    index or a record announces raises ValueError ("truncated")."""

    def __init__(self, source):
        if isinstance(source, (bytes, bytearray, memoryview)):
            self._bytes, self._file, self._path = bytes(source), None, None
        elif hasattr(source, "read"):
            self._bytes, self._file, self._path = None, source, None
        else:
            self._bytes, self._file, self._path = None, None, source
        with self._opened() as f:
            f.seek(0)
            head = f.read(4)
            magic = struct.unpack(">L", head)[0] if len(head) == 4 else None
            if magic == MAGIC:
                self.byte_order = ">"
            elif magic == MAGIC_SWAP:
                self.byte_order = "<"
            else:
                raise Exception("Not a NIB file")  # (the reference's words for a bad magic number)
            self.version, self.seq_count, self.reserved = struct.unpack(self.byte_order + "3L", self._exactly(f, 12))
            if self.version != VERSION:
                raise Exception(f"File is version '{self.version}' but I only know about '{VERSION}'")
            self.offsets = {}
            for _ in range(self.seq_count):
                length = self._exactly(f, 1)[0]
                entry = self._exactly(f, length + 4)
                self.offsets[entry[:length].decode()] = struct.unpack(self.byte_order + "L", entry[length:])[0]
        self.names = list(self.offsets)
        self._loaded = {}

    @contextlib.contextmanager
    def _opened(self):
        """the file to seek and read in: the caller's own object is left open"""
        if self._file is not None:
            yield self._file
        elif self._bytes is not None:
            yield io.BytesIO(self._bytes)
        else:
            with open(self._path, "rb") as f:
                yield f

    @staticmethod
    def _exactly(f, count):
        data = f.read(count)
        if len(data) != count:
            raise ValueError("2bit file is truncated")
        return data

    def _u32(self, f, count):
        return np.frombuffer(self._exactly(f, 4 * count), dtype=self.byte_order + "u4").astype(np.uint32)

    def load(self, name):
        if name not in self._loaded:
            at = self.offsets[name]
            with self._opened() as f:
                f.seek(at)
                size = int(self._u32(f, 1)[0])
                blocks = []
                for _ in range(2):
                    count = int(self._u32(f, 1)[0])
                    blocks += [self._u32(f, count), self._u32(f, count)]
                self._exactly(f, 4)  # reserved
                packed = np.frombuffer(self._exactly(f, (size + 3) // 4), dtype=np.uint8)
            self._loaded[name] = Sequence(size, *blocks, packed)
        return self._loaded[name]

    def load_all(self):
        return {name: self.load(name) for name in self.names}


def read_file(path=None, data=None):
    """{name: Sequence} of a .2bit file, in file order"""
    return TwoBitReader(data if data is not None else path).load_all()
