"""
Classes to support "biological sequence" files: ``SeqFile``, ``SeqReader`` and ``DNA_COMP`` of the reference's lib/bx/seq/seq.py, with
the letters read on the MI355X.  A subclass (``bx.seq.fasta.FastaFile``, ``bx.seq.nib.NibFile``) puts its sequence on the device as a
2bit track built there from its letters (bxmi.sequence.TwoBitTrack.from_letters / from_nib) the first time letters are asked of it.

``get(start, length)`` has the reference's three assertions and their texts, and its ``revcomp`` schemes (seq.py:41-50, 97-103):
"-5'" is the minus strand counted from its own 5' end (the start is mirrored), "-3'" the reverse complement of the same plus-strand
interval.  The constructor maps ``revcomp`` as the reference's does, and that maps EVERY true value -- True, "maf", "+3'", "-5'",
and "+5'" and "-3'" too, which its first test catches before the branches meant for them -- to "-5'"; the "-3'" scheme is
reached by setting the attribute.  Both minus schemes are the device's strand rows, not a translation here.

PER-CALL ``get`` IS SLOW: one device call for one row, as ``TwoBitSequence.get`` is.  ``get_batch(starts, lengths)`` answers a whole
list in ONE device call and is the call to make; it raises the AssertionError ``get`` would raise for the first row that is out
of range, before anything is read.

Letters outside ``ACGTNacgtn`` are not served byte for byte: they are refused when the sequence goes to the device (BxmiError), or
with ``other="N"`` read back as N / n.
"""


def _complement_table():
    """the 256-character table that complements the IUPAC letters in either case, keeps "-" and blanks everything else"""
    pairs = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
             "N": "N", "X": "X"}
    table = [" "] * 256
    table[ord("-")] = "-"
    for a, b in pairs.items():
        table[ord(a)], table[ord(a.lower())] = b, b.lower()
    return "".join(table)


DNA_COMP = _complement_table()


class SeqFile:
    """A sequence of letters held in a file; see the module's text for `revcomp`.  `name`: used unless the file has one; `gap`: the
    character aligners should use for gaps in this sequence ("-")."""

    def __init__(self, file=None, revcomp=False, name="", gap=None, other="error"):
        self.file = file
        # as seq.py:41-50 maps it: its first test, `if revcomp`, catches every true value, "+5'" and "-3'" among them
        self.revcomp = "-5'" if revcomp else revcomp
        self.name = name
        self.gap = "-" if gap is None else gap
        self.text = None  # (subclasses fill in text and length, or length and _make_track)
        self.length = 0
        self.other = other
        self._device = None

    def close(self):
        assert self.file is not None
        self.release()
        self.file.close()
        self.file = None

    def release(self):
        """Free the device copy of the sequence (it is made again on the next read)."""
        if self._device is not None:
            self._device.close()
            self._device = None

    def extract_name(self, line):
        words = line.split()
        return words[0] if words else ""

    def set_text(self, text):
        self.release()
        self.text = text
        self.length = len(text)

    def __str__(self):
        return (self.name + " " if self.name is not None else "") + self.get(0, self.length)

    def _make_track(self):
        from bxmi import sequence

        return sequence.TwoBitTrack.from_letters(self.text or "", self.other)

    def _track(self):
        if self._device is None:
            self._device = self._make_track()
        return self._device

    def _check(self, start, length):
        assert length >= 0, f"Length must be non-negative (got {length})"
        assert start >= 0, f"Start must be greater than 0 (got {start})"
        assert start + length <= self.length, f"Interval beyond end of sequence ({start}..{start + length} > {self.length})"

    def get(self, start, length):
        """The `length` letters from `start`, as the reference's SeqFile.get: picky about its parameters (AssertionError), the
        string has exactly `length` characters.  One device call; see get_batch."""
        return self.get_batch([start], [length])[0]

    def get_batch(self, starts, lengths):
        """[str]: `get(starts[i], lengths[i])` for a whole list in ONE device call.  The AssertionError of the first row `get`
        would refuse is raised before anything is read."""
        from bxmi import sequence

        starts, lengths = [int(s) for s in starts], [int(n) for n in lengths]
        if len(starts) != len(lengths):
            raise ValueError("starts and lengths must be of equal length")
        for start, length in zip(starts, lengths):
            self._check(start, length)
        if not self.revcomp:
            strands = None
        else:
            assert self.revcomp in ("-5'", "-3'"), "unrecognized reverse complement scheme"
            strands = ["-"] * len(starts)
            if self.revcomp == "-5'":
                starts = [self.length - (s + n) for s, n in zip(starts, lengths)]
        ends = [s + n for s, n in zip(starts, lengths)]
        return sequence.strings([self._track()], [0] * len(starts), starts, ends, True, strands)

    def raw_fetch(self, start, length):
        """the plus strand's letters [start, start + length), whatever `revcomp` is"""
        from bxmi import sequence

        return sequence.strings([self._track()], [0], [start], [start + length], True)[0]

    def reverse_complement(self, text):
        return text.translate(DNA_COMP)[::-1]


class SeqReader:
    """Iterate over all sequences in a file in order"""

    def __init__(self, file, revcomp=False, name="", gap=None):
        self.file, self.revcomp, self.name, self.gap = file, revcomp, name, gap
        self.seqs_read = 0

    def close(self):
        self.file.close()

    def __iter__(self):
        return SeqReaderIter(self)

    def __next__(self):
        return None  # (subclasses return the next SeqFile read from self.file, or None at the end)


class SeqReaderIter:
    def __init__(self, reader):
        self.reader = reader

    def __iter__(self):
        return self

    def __next__(self):
        seq = next(self.reader)
        if not seq:
            raise StopIteration
        return seq
