"""
Access to files containing sequence data in 'twobit' format: ``TwoBitFile`` and ``TwoBitSequence`` of the reference's
lib/bx/seq/twobit.py, with the letters read on the MI355X (bxmi.sequence) from the file's packed bytes held in HBM.

``TwoBitFile(file, do_mask=True)`` is a Mapping of names to ``TwoBitSequence``; ``seq[a:b]``, ``seq.get(start, end)``,
``len(seq)`` and the attributes ``size``, ``n_block_starts``, ``n_block_sizes``, ``masked_block_starts``, ``masked_block_sizes`` are
the reference's, exception texts included.  Only the index is read when the object is made; a sequence's record is read when the
sequence is first asked for (`tbf[name]`), and it goes to the device the first time letters are asked of it.  `file` must stay
open for as long as sequences are loaded from it, as the reference requires.

PER-SLICE CALLS ARE SLOW: every ``get`` and every slice is one device call for one row -- a launch, a copy back and a
synchronisation for a handful of bytes -- as ``IntervalTree.find`` is one device call per query.  They exist for compatibility.
``get_batch(chroms, starts, ends)`` answers a whole list of regions in ONE device call, each clipped as ``get`` clips it, and is
the call to make; a region for which ``get`` would raise ("end before start") or whose name the file does not have is ``""``.
"""
from collections.abc import Mapping

from bxmi import twobit as _reader

# the reference's module-level names, with the reader's values
TWOBIT_MAGIC_NUMBER, TWOBIT_MAGIC_NUMBER_SWAP, TWOBIT_VERSION = _reader.MAGIC, _reader.MAGIC_SWAP, _reader.VERSION
TWOBIT_MAGIC_SIZE = 4


class TwoBitSequence:
    """One sequence of a TwoBitFile.  `size` and the four block lists are there once the file has loaded the sequence (`tbf[name]`
    does); the letters come from the device."""

    def __init__(self, tbf, name, header_offset=None):
        self.tbf, self.name, self.header_offset = tbf, name, header_offset
        self.size, self.loaded = None, False

    def _load(self):
        seq = self.tbf._reader.load(self.name)
        self.size = seq.size
        self.n_block_starts, self.n_block_sizes = seq.n_starts.tolist(), seq.n_sizes.tolist()
        self.masked_block_starts, self.masked_block_sizes = seq.m_starts.tolist(), seq.m_sizes.tolist()
        self.loaded = True

    def _read(self, first, past):
        """the letters of [first, past), which lies inside the sequence and is not empty: one device call for one row"""
        from bxmi import sequence

        return sequence.strings([self.tbf._track(self.name)], [0], [first], [past], self.tbf.do_mask)[0]

    def __len__(self):
        return self.size

    def __getitem__(self, key):
        first, past, step = key.indices(self.size)
        assert step == 1, "Striding in slices not supported"
        return self._read(first, past) if past > first else ""

    def get(self, start, end):
        first, past = max(start, 0), min(end, self.size)
        if past <= first:
            raise Exception("end before start (%d,%d)" % (first, past))
        return self._read(first, past)


class TwoBitFile(Mapping):
    """A .2bit file as a Mapping of sequence names, in file order, to TwoBitSequence."""

    def __init__(self, file, do_mask=True):
        self.do_mask = do_mask
        self._reader = _reader.TwoBitReader(file)  # (raises the reference's "Not a NIB file" / version message)
        self.file = file
        self.byte_order = self._reader.byte_order
        self.magic = TWOBIT_MAGIC_NUMBER if self.byte_order == ">" else TWOBIT_MAGIC_NUMBER_SWAP
        self.version = self._reader.version
        self.seq_count = self._reader.seq_count
        self.reserved = self._reader.reserved
        self.index = {name: TwoBitSequence(self, name, offset) for name, offset in self._reader.offsets.items()}
        self._tracks = {}

    def __len__(self):
        return len(self.index)

    def __iter__(self):
        return iter(self.index)

    def __getitem__(self, name):
        self.load_sequence(name)  # (KeyError for a name the file does not have)
        return self.index[name]

    def load_sequence(self, name):
        if not self.index[name].loaded:
            self.index[name]._load()

    def _track(self, name):
        """the sequence on the device, put there on first use"""
        if name not in self._tracks:
            from bxmi import sequence

            self._tracks[name] = sequence.TwoBitTrack(self._reader.load(name))
        return self._tracks[name]

    def close(self):
        """Free the device copies of the sequences (they are made again on the next read)."""
        for t in self._tracks.values():
            t.close()
        self._tracks = {}

    def get_batch(self, chroms, starts, ends):
        """[str]: `TwoBitSequence.get(starts[i], ends[i])` of sequence chroms[i] for a whole list of regions in ONE device call;
        "" where `get` would raise or the file has no such sequence."""
        from bxmi import sequence

        names = [c.decode() if isinstance(c, (bytes, bytearray)) else c for c in chroms]
        used = [n for n in dict.fromkeys(names) if n in self.index]
        where = {n: k for k, n in enumerate(used)}
        return sequence.strings([self._track(n) for n in used], [where.get(n, -1) for n in names], starts, ends, self.do_mask)
