"""
Classes to support nib files: ``NibFile`` and ``NibReader`` of the reference's lib/bx/seq/nib.py, with ``get`` answered on the MI355X
(bx.seq.seq.SeqFile: ``get_batch(starts, lengths)`` is the call to make).  The header is read when the object is made; the nibbles
are read, and put on the device as they are (bxmi.sequence.TwoBitTrack.from_nib), the first time letters are asked for.  The codes
5-7, which the reference prints as "X", are refused then, or with ``other="N"`` read back as N.
"""
import struct

from bx.seq.seq import SeqFile, SeqReader
from bxmi import nib as _reader

NIB_MAGIC_NUMBER, NIB_MAGIC_NUMBER_SWAP = _reader.MAGIC, _reader.MAGIC_SWAP
NIB_MAGIC_SIZE = 4
NIB_LENGTH_SIZE = 4


class NibFile(SeqFile):
    def __init__(self, file, revcomp=False, name="", gap=None, other="error"):
        SeqFile.__init__(self, file, revcomp, name, gap, other)
        head = file.read(NIB_MAGIC_SIZE)
        magic = struct.unpack(">L", head)[0] if len(head) == NIB_MAGIC_SIZE else None
        if magic == NIB_MAGIC_NUMBER:
            self.byte_order = ">"
        elif magic == NIB_MAGIC_NUMBER_SWAP:
            self.byte_order = "<"
        else:
            raise Exception("Not a NIB file")
        self.magic = magic
        self.length = struct.unpack(self.byte_order + "L", file.read(NIB_LENGTH_SIZE))[0]

    def _make_track(self):
        from bxmi import sequence

        self.file.seek(NIB_MAGIC_SIZE + NIB_LENGTH_SIZE)
        return sequence.TwoBitTrack.from_nib(self.file.read((self.length + 1) // 2), self.length, self.other)


class NibReader(SeqReader):
    def __next__(self):
        if self.seqs_read != 0:
            return None  # (a nib file holds one sequence)
        self.seqs_read += 1
        return NibFile(self.file, self.revcomp, self.name, self.gap)
