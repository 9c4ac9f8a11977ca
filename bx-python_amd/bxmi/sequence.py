"""
The sequence of .2bit files on the MI355X: ``TwoBitSequence.get`` / ``__getitem__`` (reference: lib/bx/seq/twobit.py:34-56 over
``_twobit.read``, lib/bx/seq/_twobit.pyx:22-137) for a whole array of regions per call, and the base counts of those regions.

``TwoBitTrack`` is one sequence resident in HBM (``bxmi_twobit_*`` of include/bxmi.h): its packed bytes, its N blocks and its mask
blocks.  ``TwoBitSet`` is a whole file on the device.  ``sequences`` / ``strings`` give every row's letters exactly as the
reference's string has them -- TCAG by code, N inside an N block, lower case inside a mask block when ``do_mask`` is set --
``matrix`` the site x base matrix uint8 [n, width] with a pad byte outside the sequence, ``composition`` the int32 [n, 6] counts
A, C, G, T, N, masked of every row at a cost that does not depend on the row's length.  The ``_dev`` forms take and return torch
tensors on the caller's stream; the matrix stays on the device, where a lookup on the byte tensor gives codes or one-hot planes.
Everything is integer work: the outputs are the reference's byte for byte.

``strands`` (every function and method here; None: all plus) gives the minus rows as their reverse complement, the reference's
``SeqFile.reverse_complement`` (lib/bx/seq/seq.py:108-109: ``text.translate(DNA_COMP)[::-1]``): the letters reversed and
complemented with the case kept and N left N, the pad of ``matrix`` mirrored with them and never complemented; the base counts with
A and T, C and G exchanged.  The host forms take a sequence of "+" / "-", bools or 0 / 1, the ``_dev`` forms an int8, uint8 or bool
tensor on the device (any non-zero entry is minus; nothing is read back).

Tracks are also BUILT on the device from letters (csrc/twobit_build.hpp): ``TwoBitTrack.from_letters`` (bytes, str or a uint8 array),
``from_letters_dev`` (a uint8 tensor in HBM -- the output of ``matrix_dev`` or ``sequences_dev``, edited or not -- with no host copy)
and ``from_nib`` (nibbles as a nib file holds them); ``TwoBitSet.from_fasta``, ``from_nib`` and ``open`` (which looks at the file) make
whole sets from what the reference reads through the same ``SeqFile.get`` as 2bit.  The N blocks and the mask blocks of a built track
are the maximal runs of N / n and of lower case, its packed code under N is 0: the arrays a .2bit file of the same letters holds
(``TwoBitTrack.arrays`` reads them back).  A letter outside ``TCAGNtcagn`` raises BxmiError naming the lowest such position
(``other="error"``), or becomes N and, if it is lower case, masked (``other="N"``).  One track per record: a FASTA file of very many
records loads slowly.

Only files whose blocks are sorted, non-empty, disjoint and inside the sequence are accepted -- every real file; for those the
reference's walk over the blocks is plain coverage.  Anything else raises BxmiError (EINVAL) naming the condition.
"""
import ctypes as C
import glob
import os
import struct

import numpy as np

from . import _ffi, fasta, nib, twobit
from ._ffi import as_i32, call, ptr
from .summary import _rows_i32, _Track

COLUMNS = ("A", "C", "G", "T", "N", "masked")  # of `composition`


class TwoBitTrack(_Track):
    """One sequence on the device."""

    _destroy = "bxmi_twobit_destroy"

    def __init__(self, seq):
        """seq: a bxmi.twobit.Sequence"""
        _ffi.require_gpu()
        blocks = [as_i32(a) for a in (seq.n_starts, seq.n_sizes, seq.m_starts, seq.m_sizes)]
        packed = np.ascontiguousarray(seq.packed, dtype=np.uint8)
        size = int(seq.size)
        if blocks[0].shape != blocks[1].shape or blocks[2].shape != blocks[3].shape or any(b.ndim != 1 for b in blocks):
            raise ValueError("block starts and sizes must be 1-d arrays of equal length")
        if packed.ndim != 1 or (0 <= size and len(packed) < (size + 3) // 4):
            raise ValueError("packed must hold (size + 3) // 4 bytes")
        self._create("bxmi_twobit_create", ptr(packed), size, ptr(blocks[0]), ptr(blocks[1]), len(blocks[0]), ptr(blocks[2]), ptr(blocks[3]),
                     len(blocks[2]))
        self.size, self.n_blocks, self.m_blocks = self._info("bxmi_twobit_info", C.c_int64, C.c_int64, C.c_int64)

    @classmethod
    def from_arrays(cls, packed, size, n_starts=(), n_sizes=(), m_starts=(), m_sizes=()):
        u32 = [np.asarray(a, dtype=np.int64) for a in (n_starts, n_sizes, m_starts, m_sizes)]
        return cls(twobit.Sequence(size, *u32, np.asarray(packed, dtype=np.uint8)))

    @classmethod
    def _built(cls, symbol, *args, stream=()):
        """a track the library builds from letters: `symbol`(*args, &handle[, stream])"""
        _ffi.require_gpu()
        self = cls.__new__(cls)
        h = C.c_void_p()
        call(symbol, *args, C.byref(h), *stream)
        self._h = h
        self.size, self.n_blocks, self.m_blocks = self._info("bxmi_twobit_info", C.c_int64, C.c_int64, C.c_int64)
        return self

    @classmethod
    def from_letters(cls, letters, other="error"):
        """The track of a sequence given as its letters: bytes, str or a uint8 array.  N blocks and mask blocks are the maximal runs
        of N / n and of lower case.  A letter outside TCAGNtcagn raises BxmiError (EINVAL) naming the lowest such position and its
        value under other="error"; under other="N" it becomes N, masked as well if it is a lower-case letter."""
        if isinstance(letters, str):
            letters = letters.encode("latin-1")
        if isinstance(letters, (bytes, bytearray, memoryview)):
            letters = np.frombuffer(bytes(letters), dtype=np.uint8)
        letters = np.ascontiguousarray(letters)
        if letters.dtype != np.uint8 or letters.ndim != 1:
            raise ValueError("letters must be bytes, str or a 1-d uint8 array")
        return cls._built("bxmi_twobit_create_letters", ptr(letters), len(letters), _other(other))

    @classmethod
    def from_letters_dev(cls, letters, other="error", stream=None):
        """`from_letters` of a contiguous uint8 torch tensor on the GPU, of any shape (its elements in memory order are the
        sequence): the output of `matrix_dev` / `sequences_dev`, edited or not.  Nothing of the letters is read on the host.  The
        kernels run on torch's current stream (or `stream`), which is synchronised before this returns: the tensor may then be
        changed or dropped."""
        import torch

        if not isinstance(letters, torch.Tensor) or letters.dtype != torch.uint8 or not letters.is_cuda or not letters.is_contiguous():
            raise ValueError("from_letters_dev takes a contiguous uint8 tensor on the device (host letters: from_letters)")
        if stream is None:
            stream = torch.cuda.current_stream(letters.device).cuda_stream
        return cls._built("bxmi_twobit_create_letters_dev", letters.data_ptr(), letters.numel(), _other(other), stream=(stream,))

    @classmethod
    def from_nib(cls, nibbles, size, other="error"):
        """The track of `size` bases held as nibbles, (size + 1) // 2 bytes as a nib file holds them (bxmi.nib.read_file).  The codes
        5-7, which the reference prints as X, are what `other` is about; the mask bit makes them lower case."""
        nibbles = np.ascontiguousarray(np.frombuffer(bytes(nibbles), dtype=np.uint8) if isinstance(nibbles, (bytes, bytearray, memoryview)) else nibbles)
        size = int(size)
        if nibbles.dtype != np.uint8 or nibbles.ndim != 1 or (size >= 0 and len(nibbles) < (size + 1) // 2):
            raise ValueError("nibbles must hold (size + 1) // 2 bytes")
        return cls._built("bxmi_twobit_create_nib", ptr(nibbles), size, _other(other))

    def arrays(self):
        """The track's arrays as a .2bit file holds them, read back from the device -> bxmi.twobit.Sequence.  For a track made from
        a file's arrays they are those arrays; for a built one, the arrays the builder derived."""
        packed = np.zeros((self.size + 3) // 4, dtype=np.uint8)
        blocks = [np.zeros(k, dtype=np.int32) for k in (self.n_blocks, self.n_blocks, self.m_blocks, self.m_blocks)]
        call("bxmi_twobit_arrays", self._h, ptr(packed), *[ptr(b) for b in blocks])
        return twobit.Sequence(self.size, *[b.astype(np.uint32) for b in blocks], packed)


_OTHER = {"error": 0, "N": 1}  # BXMI_TB_OTHER_REFUSE, BXMI_TB_OTHER_N


def _other(other):
    if other not in _OTHER:
        raise ValueError("other must be 'error' or 'N', not %r" % (other,))
    return _OTHER[other]


def _pad_byte(pad):
    if isinstance(pad, (bytes, str)):
        if len(pad) != 1:
            raise ValueError("pad must be one byte")
        return ord(pad)
    return int(pad)


def _strands(strands, n):
    """None, or int8 [n] of 0 (plus) and 1 (minus) from a sequence of "+" / "-", bools or 0 / 1; anything else is a ValueError"""
    if strands is None:
        return None
    given = strands.tolist() if isinstance(strands, np.ndarray) else list(strands)
    if len(given) != n:
        raise ValueError("strands must have one entry per row: %d for %d rows" % (len(given), n))
    out = np.zeros(n, dtype=np.int8)
    for i, v in enumerate(given):
        if isinstance(v, (bytes, np.bytes_)):
            v = v.decode("ascii", "replace")
        if isinstance(v, str):
            if v not in ("+", "-"):
                raise ValueError("strands[%d] = %r is neither '+' nor '-'" % (i, v))
            out[i] = v == "-"
        elif isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and v in (0, 1)):
            out[i] = int(v)
        else:
            raise ValueError("strands[%d] = %r is none of '+', '-', a bool, 0 or 1" % (i, v))
    return out


def _strands_dev(strands, n, dev, who):
    """None, or the int8 view / copy of an int8, uint8 or bool tensor [n] on `dev` (nothing is read back: any non-zero entry is minus)"""
    if strands is None:
        return None
    import torch

    if not isinstance(strands, torch.Tensor) or strands.dtype not in (torch.int8, torch.uint8, torch.bool):
        raise ValueError("%s: strands must be an int8, uint8 or bool tensor on the device" % who)
    if strands.device != dev or tuple(strands.shape) != (n,):
        raise ValueError("%s: strands must be a tensor of %d entries on the device of the rows" % (who, n))
    strands = strands.contiguous()
    return strands.view(torch.int8) if strands.dtype != torch.int8 else strands


def _clip(sizes, track_of, s, e):
    """the rows as TwoBitSequence.get clips them (twobit.py:44-51): start below 0 is 0, end beyond the size is the size; a row the
    reference refuses ("end before start") or whose sequence is unknown is empty -> (starts, lengths) int64.  A track_of beyond
    the list is left to the C check that follows: its row is empty here."""
    table = np.array(list(sizes) + [0], dtype=np.int64)  # (the last entry: rows without a track)
    named = (track_of >= 0) & (track_of < len(sizes))
    size = table[np.where(named, track_of, len(sizes))]
    first = np.maximum(s.astype(np.int64), 0)
    return first, np.maximum(np.minimum(e.astype(np.int64), size) - first, 0)


def sequences(tracks, track_of, starts, ends, do_mask=True, strands=None):
    """The letters of regions [starts[i], ends[i]) of tracks[track_of[i]], clipped as TwoBitSequence.get clips them -> (bytes
    uint8[total], offsets int64[n + 1]): row i is bytes[offsets[i]:offsets[i + 1]].  Where the reference raises "end before start"
    the row is empty; track_of[i] < 0 (unknown name) gives an empty row.  One device pass over the OUTPUT."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    s64, lengths = _clip([tr.size for tr in tracks], t, s, e)
    offsets = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    out = np.empty(int(offsets[-1]), dtype=np.uint8)
    strand = _strands(strands, len(t))
    if strand is None:
        call("bxmi_twobit_bases", _ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), len(t), 0, ptr(offsets), len(out), int(bool(do_mask)),
             ord("N"), ptr(out))
    else:  # (a minus row: the reverse complement of the clipped region)
        call("bxmi_twobit_bases_strand", _ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), ptr(strand), len(t), 0, ptr(offsets), len(out),
             int(bool(do_mask)), ord("N"), ptr(out))
    return out, offsets


def strings(tracks, track_of, starts, ends, do_mask=True, strands=None):
    """`sequences` as a list of str"""
    data, offsets = sequences(tracks, track_of, starts, ends, do_mask, strands)
    text = data.tobytes().decode("ascii")
    return [text[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]


def matrix(tracks, track_of, starts, width, pad=b"N", do_mask=True, strands=None):
    """The windows [starts[i], starts[i] + width) of tracks[track_of[i]] -> uint8 [n, width] of letters, the byte `pad` where a
    position is outside the sequence or the row names no track.  width < 1 raises BxmiError (EINVAL)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s = _rows_i32("track_of and starts", track_of, starts)
    width = int(width)
    out = np.empty((len(t), max(width, 0)), dtype=np.uint8)
    strand = _strands(strands, len(t))
    if strand is None:
        call("bxmi_twobit_bases", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), width, None, out.size, int(bool(do_mask)), _pad_byte(pad),
             ptr(out))
    else:
        call("bxmi_twobit_bases_strand", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(strand), len(t), width, None, out.size, int(bool(do_mask)),
             _pad_byte(pad), ptr(out))
    return out


def composition(tracks, track_of, starts, ends, do_mask=True, strands=None):
    """int32 [n, 6] = A, C, G, T, N, masked of [starts[i], ends[i]) clipped to the sequence: what counting the characters of the
    reference's string gives (case folded for the first five, the lower-case ones for the sixth; masked is 0 without do_mask).  An
    unknown sequence or an empty row gives zeros.  A row's cost does not depend on its length."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    out = np.zeros((len(t), 6), dtype=np.int32)
    strand = _strands(strands, len(t))
    if strand is None:
        call("bxmi_twobit_composition", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(e), len(t), int(bool(do_mask)), ptr(out))
    else:
        call("bxmi_twobit_composition_strand", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(strand), ptr(e), len(t), int(bool(do_mask)), ptr(out))
    return out


def matrix_dev(tracks, track_of, starts, width, pad=b"N", do_mask=True, stream=None, out=None, strands=None):
    """`matrix` on device arrays: int32 torch tensors on the GPU in, the uint8 [n, width] tensor out -- `out` if given (contiguous
    uint8 [n, width] on the same device; 16-byte aligned it is written by 16-byte stores, otherwise byte by byte, with the same
    result), else a new one.  Queued on torch's current stream (or `stream`), nothing is waited for.  A track_of outside
    [0, len(tracks)) gives a row of `pad`.  ONE 2bit call at a time per process may be in flight: the table of tracks the kernel
    reads belongs to the library and is rewritten by every call on that call's stream."""
    import torch

    tracks = list(tracks)
    (track_of, starts), n, dev, stream = _ffi.device_args("matrix_dev", "matrix", ("track_of", "starts"), (track_of, starts), stream)
    width = int(width)
    if out is None:
        out = torch.empty((n, max(width, 0)), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, width) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous uint8 [n, width] tensor on the device of the rows")
    strand = _strands_dev(strands, n, dev, "matrix_dev")
    if strand is None:
        call("bxmi_twobit_bases_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), n, width, None, out.numel(),
             int(bool(do_mask)), _pad_byte(pad), out.data_ptr(), stream)
    else:
        call("bxmi_twobit_bases_strand_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), strand.data_ptr(), n, width, None,
             out.numel(), int(bool(do_mask)), _pad_byte(pad), out.data_ptr(), stream)
        if n and strand is not strands:
            _record(stream, dev, (strand,))
    return out


def _clip_dev(tracks, track_of, starts, ends, n, dev):
    """`_clip` by torch on its current stream, for the device forms -> (first int32 [n], offsets int64 [n + 1])"""
    import torch

    sizes = torch.tensor([tr.size for tr in tracks] + [0], dtype=torch.int64, device=dev)  # (the last: rows without a track)
    named = (track_of >= 0) & (track_of < len(tracks))
    size = sizes[torch.where(named, track_of, torch.full_like(track_of, len(tracks))).to(torch.int64)]
    first = starts.clamp(min=0)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum((torch.minimum(ends.to(torch.int64), size) - first.to(torch.int64)).clamp_(min=0), 0, out=offsets[1:])
    return first, offsets


def _record(stream, dev, tensors):
    """Tensors a device form made for itself are read or written by a kernel on `stream`; when that is not torch's current stream
    its allocator does not know them by it: a tensor dropped on return must not have its block handed out again before `stream`
    has passed this point.  (This protects the memory; it orders no work.)"""
    import torch

    if stream != torch.cuda.current_stream(dev).cuda_stream:
        used_on = torch.cuda.ExternalStream(stream, device=dev)
        for t in tensors:
            t.record_stream(used_on)


def sequences_dev(tracks, track_of, starts, ends, do_mask=True, stream=None, strands=None):
    """`sequences` on device arrays: int32 torch tensors on the GPU in, (bytes uint8[total], offsets int64[n + 1]) tensors out.
    The clipping and the offsets are computed by torch on its current stream and `total` is read back to size the output -- ONE
    synchronisation; the letters are then queued on torch's current stream (or `stream`: the tensors made here are then recorded
    as in use on it) and not waited for.  One 2bit call at a time, as `matrix_dev`."""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("sequences_dev", "sequences", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    first, offsets = _clip_dev(tracks, track_of, starts, ends, n, dev)
    total = int(offsets[-1].item()) if n else 0  # (the synchronisation: `first` and `offsets` are complete after it)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    strand = _strands_dev(strands, n, dev, "sequences_dev")
    if strand is None:
        call("bxmi_twobit_bases_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), n, 0, offsets.data_ptr(), total,
             int(bool(do_mask)), ord("N"), out.data_ptr(), stream)
    else:
        call("bxmi_twobit_bases_strand_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), strand.data_ptr(), n, 0,
             offsets.data_ptr(), total, int(bool(do_mask)), ord("N"), out.data_ptr(), stream)
    if total:
        _record(stream, dev, (first, offsets, out) + ((strand,) if strand is not None and strand is not strands else ()))
    return out, offsets


def composition_dev(tracks, track_of, starts, ends, do_mask=True, stream=None, strands=None):
    """`composition` on device arrays: int32 torch tensors in, the int32 [n, 6] tensor out, queued on torch's current stream (or
    `stream`), nothing waited for.  One 2bit call at a time, as `matrix_dev`."""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("composition_dev", "composition", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    out = torch.zeros((n, 6), dtype=torch.int32, device=dev)
    strand = _strands_dev(strands, n, dev, "composition_dev")
    if strand is None:
        call("bxmi_twobit_composition_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), ends.data_ptr(), n,
             int(bool(do_mask)), out.data_ptr(), stream)
    else:
        call("bxmi_twobit_composition_strand_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), strand.data_ptr(),
             ends.data_ptr(), n, int(bool(do_mask)), out.data_ptr(), stream)
        if n and strand is not strands:
            _record(stream, dev, (strand,))
    return out


class TwoBitSet:
    """A whole .2bit file on the device: one TwoBitTrack per sequence, `chroms` the names in file order.  Rows are given by name or
    by position in `chroms` (an int array; -1: unknown), as bxmi.summary.TrackSet takes them."""

    def __init__(self, seqs, do_mask=True):
        """seqs: bxmi.twobit.read_file's result"""
        self.do_mask = bool(do_mask)
        self.chroms = list(seqs)
        self.tracks = {name: TwoBitTrack(seqs[name]) for name in self.chroms}
        self.sizes = {name: self.tracks[name].size for name in self.chroms}

    @classmethod
    def from_file(cls, path=None, do_mask=True, data=None):
        return cls(twobit.read_file(path, data=data), do_mask)

    @classmethod
    def _of_tracks(cls, tracks, do_mask):
        self = cls.__new__(cls)
        self.do_mask = bool(do_mask)
        self.chroms = list(tracks)
        self.tracks = dict(tracks)
        self.sizes = {name: self.tracks[name].size for name in self.chroms}
        return self

    @classmethod
    def from_fasta(cls, path=None, do_mask=True, other="error", data=None):
        """A FASTA file (bxmi.fasta.read_file: .gz accepted) on the device, one track per record, built there from the letters.
        `other`: as TwoBitTrack.from_letters."""
        tracks = {}
        try:
            for name, letters in fasta.read_file(path, data=data).items():
                tracks[name] = TwoBitTrack.from_letters(letters, other)
        except Exception:
            _ffi.close_all(tracks.values())
            raise
        return cls._of_tracks(tracks, do_mask)

    @classmethod
    def from_nib(cls, paths_or_dir, do_mask=True, other="error"):
        """nib files on the device, one track each, named by the files' stems: a path, a list of paths, or a directory (its *.nib
        files in sorted order)."""
        if isinstance(paths_or_dir, (str, os.PathLike)):
            paths = sorted(glob.glob(os.path.join(paths_or_dir, "*.nib"))) if os.path.isdir(paths_or_dir) else [paths_or_dir]
        else:
            paths = list(paths_or_dir)
        tracks = {}
        try:
            for path in paths:
                name = os.path.splitext(os.path.basename(path))[0]
                if name in tracks:
                    raise ValueError("two nib files named %r" % name)
                size, nibbles, _ = nib.read_file(path)
                tracks[name] = TwoBitTrack.from_nib(nibbles, size, other)
        except Exception:
            _ffi.close_all(tracks.values())
            raise
        return cls._of_tracks(tracks, do_mask)

    @classmethod
    def open(cls, path, do_mask=True, other="error"):
        """Whatever sequence file `path` is: a directory (of nib files), or by its first four bytes a .2bit file or a nib file, and
        otherwise FASTA."""
        if os.path.isdir(path):
            return cls.from_nib(path, do_mask, other)
        with open(path, "rb") as f:
            head = f.read(4)
        magic = struct.unpack(">L", head)[0] if len(head) == 4 else None
        if magic in (twobit.MAGIC, twobit.MAGIC_SWAP):
            return cls.from_file(path, do_mask)
        if magic in (nib.MAGIC, nib.MAGIC_SWAP):
            return cls.from_nib(path, do_mask, other)
        return cls.from_fasta(path, do_mask, other)

    def close(self):
        _ffi.close_all(self.tracks.values())

    def _track_of(self, chroms):
        chroms = np.asarray(chroms)
        if chroms.dtype.kind in "iu":
            track_of = as_i32(chroms)
        else:
            index = {chrom: k for k, chrom in enumerate(self.chroms)}
            track_of = np.array([index.get(c, -1) for c in chroms.tolist()], dtype=np.int32)
        if track_of.ndim != 1:
            raise ValueError("chroms, starts and ends must be 1-d arrays of equal length")
        if len(track_of) and track_of.max() >= len(self.chroms):
            raise ValueError("a sequence position beyond the file's %d sequences" % len(self.chroms))
        return track_of

    def sequences(self, chroms, starts, ends, strands=None):
        return sequences(self.tracks.values(), self._track_of(chroms), starts, ends, self.do_mask, strands)

    def strings(self, chroms, starts, ends, strands=None):
        return strings(self.tracks.values(), self._track_of(chroms), starts, ends, self.do_mask, strands)

    def matrix(self, chroms, starts, width, pad=b"N", strands=None):
        return matrix(self.tracks.values(), self._track_of(chroms), starts, width, pad, self.do_mask, strands)

    def composition(self, chroms, starts, ends, strands=None):
        return composition(self.tracks.values(), self._track_of(chroms), starts, ends, self.do_mask, strands)

    def matrix_dev(self, track_of, starts, width, pad=b"N", stream=None, out=None, strands=None):
        return matrix_dev(self.tracks.values(), track_of, starts, width, pad, self.do_mask, stream, out, strands)

    def sequences_dev(self, track_of, starts, ends, stream=None, strands=None):
        return sequences_dev(self.tracks.values(), track_of, starts, ends, self.do_mask, stream, strands)

    def composition_dev(self, track_of, starts, ends, stream=None, strands=None):
        return composition_dev(self.tracks.values(), track_of, starts, ends, self.do_mask, stream, strands)

    # position weight matrices over the rows (bxmi.motif, which builds on this module); `pwms`: a motif.MatrixSet, for the host
    # forms also a list of motif.ScoringMatrix
    def scores(self, chroms, starts, ends, pwms, strands=None):
        from . import motif

        return motif.scores(self.tracks.values(), self._track_of(chroms), starts, ends, pwms, self.do_mask, strands)

    def score_matrix(self, chroms, starts, width, pwms, strands=None):
        from . import motif

        return motif.score_matrix(self.tracks.values(), self._track_of(chroms), starts, width, pwms, self.do_mask, strands)

    def best(self, chroms, starts, ends, pwms, strands=None):
        from . import motif

        return motif.best(self.tracks.values(), self._track_of(chroms), starts, ends, pwms, self.do_mask, strands)

    def scores_dev(self, track_of, starts, ends, pwms, stream=None, strands=None):
        from . import motif

        return motif.scores_dev(self.tracks.values(), track_of, starts, ends, pwms, self.do_mask, stream, strands)

    def score_matrix_dev(self, track_of, starts, width, pwms, stream=None, out=None, strands=None):
        from . import motif

        return motif.score_matrix_dev(self.tracks.values(), track_of, starts, width, pwms, self.do_mask, stream, out, strands)

    def best_dev(self, track_of, starts, ends, pwms, stream=None, strands=None):
        from . import motif

        return motif.best_dev(self.tracks.values(), track_of, starts, ends, pwms, self.do_mask, stream, strands)

    def hits(self, chroms, starts, ends, pwms, thresholds, strands=None):
        from . import motif

        return motif.hits(self.tracks.values(), self._track_of(chroms), starts, ends, pwms, thresholds, self.do_mask, strands)

    def hits_dev(self, track_of, starts, ends, pwms, thresholds, max_hits=None, stream=None, strands=None):
        from . import motif

        return motif.hits_dev(self.tracks.values(), track_of, starts, ends, pwms, thresholds, self.do_mask, max_hits, stream, strands)

    # the k-mer spectrum of the rows (bxmi.kmers, which builds on this module)
    def kmer_counts(self, chroms, starts, ends, k, alphabet="ACGT", case_sensitive=True, drop_last=False, strands=None):
        from . import kmers

        return kmers.counts(self.tracks.values(), self._track_of(chroms), starts, ends, k, alphabet, case_sensitive, self.do_mask, drop_last, strands)

    def kmer_count_matrix(self, chroms, starts, width, k, alphabet="ACGT", case_sensitive=True, drop_last=False, strands=None):
        from . import kmers

        return kmers.count_matrix(self.tracks.values(), self._track_of(chroms), starts, width, k, alphabet, case_sensitive, self.do_mask, drop_last,
                                  strands)

    def kmer_counts_dev(self, track_of, starts, ends, k, alphabet="ACGT", case_sensitive=True, drop_last=False, stream=None, out=None, strands=None):
        from . import kmers

        return kmers.counts_dev(self.tracks.values(), track_of, starts, ends, k, alphabet, case_sensitive, self.do_mask, drop_last, stream, out, strands)

    def kmer_count_matrix_dev(self, track_of, starts, width, k, alphabet="ACGT", case_sensitive=True, drop_last=False, stream=None, out=None,
                              strands=None):
        from . import kmers

        return kmers.count_matrix_dev(self.tracks.values(), track_of, starts, width, k, alphabet, case_sensitive, self.do_mask, drop_last, stream, out,
                                      strands)
