"""
Position weight matrices scored over the sequence of .2bit files on the MI355X: ``ScoringMatrix.score_string`` (reference:
lib/bx/motif/pwm.py:141-149 over ``_pwm.score_string``, lib/bx/motif/_pwm.pyx:23-55) for a whole array of regions per call, read
straight from the packed bases (``bxmi_pwm_*`` / ``bxmi_twobit_pwm_*`` of include/bxmi.h; kernels: csrc/pwm.hpp).

``ScoringMatrix`` holds one matrix as the reference's ``from_rows`` lays it out; ``MatrixSet`` is one or more of them, over one
alphabet, resident in HBM -- a matrix and its reverse complement is the common case.  ``scores`` gives, per matrix, the score at
every offset of every region, ``score_matrix`` the same for windows of one width, ``best`` only the greatest score of every region
and the first offset that holds it.  A score is the reference's float32 chain ``((0 + v[0][c0]) + v[1][c1]) + ...`` bit for bit;
NaN (numpy's) where a letter of the window has no column -- with the alphabet ``ACGT`` an N or a soft-masked base -- and in the last
``width - 1`` offsets of a region.  The map is case sensitive, as the reference's: an alphabet with ``acgt`` or ``N`` scores them.
``hits`` lists the offsets whose score reaches a threshold -- a scan -- as (matrix, region, offset, score) in that order, without the
scores of the other offsets ever being written (``bxmi_twobit_pwm_hits*``; kernels: csrc/pwm_hits.hpp).  The ``_dev`` forms take and
return torch tensors on the caller's stream.

``strands`` (every function here; None: all plus) scores the minus rows on their reverse complement, the reference's
``matrix.score_string(seq.get(s, e).translate(DNA_COMP)[::-1])`` bit for bit (``bxmi_twobit_pwm_*_strand``): offsets, the first
of equal best scores and the order of hits are those of the strand's string, and ``site_starts`` turns such offsets into genomic
starts.  The reverse-complement matrix on the plus string is a different quantity: the same terms added in the opposite order,
equal to this one (mirrored) only where every partial sum is exact, as for small integer matrices.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import as_i32, call, ptr
from .sequence import _clip, _clip_dev, _record, _strands, _strands_dev
from .summary import _rows_i32, _Track

LETTERS = "TCAGNtcagn"  # the ten letters a 2bit string can hold, in the order of the handle's letter_col


class ScoringMatrix:
    """One matrix: `values` float32 [width, len(alphabet)], the columns in sorted-alphabet order; `char_to_index` int16 [256], -1
    for a character outside the alphabet.  `rows[j]` holds the values of position j in the order of `alphabet`."""

    def __init__(self, alphabet, rows):
        self.alphabet = list(alphabet)
        self.sorted_alphabet = sorted(self.alphabet)
        if len(set(self.alphabet)) != len(self.alphabet) or any(len(ch) != 1 or ord(ch) > 255 for ch in self.alphabet):
            raise ValueError("the alphabet must be distinct single characters")
        self.char_to_index = np.full(256, -1, dtype=np.int16)
        for i, ch in enumerate(self.sorted_alphabet):
            self.char_to_index[ord(ch)] = i
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, len(self.alphabet))
        order = [self.alphabet.index(ch) for ch in self.sorted_alphabet]
        self.values = np.ascontiguousarray(rows[:, order])

    @property
    def width(self):
        return self.values.shape[0]

    def reverse_complement(self):
        """the rows reversed and the columns reversed (for ACGT: A <-> T, C <-> G), as the reference's; the result's `alphabet` is
        the sorted one, the order its rows are in"""
        return ScoringMatrix(self.sorted_alphabet, self.values[::-1, ::-1])


def read_matrix(lines):
    """a matrix file: the alphabet's letters on the first line, then one row of numbers per matrix position"""
    lines = [ln for ln in (raw.strip() for raw in lines) if ln and not ln.startswith("#")]
    if len(lines) < 2:
        raise ValueError("a matrix file holds the alphabet and at least one row")
    alphabet = lines[0].split() if " " in lines[0] or "\t" in lines[0] else list(lines[0])
    return ScoringMatrix(alphabet, [[float(x) for x in ln.split()] for ln in lines[1:]])


class MatrixSet(_Track):
    """Matrices over one alphabet on the device.  A letter of the alphabet outside the ten a 2bit string can hold is a column no
    base ever selects."""

    _destroy = "bxmi_pwm_destroy"

    def __init__(self, matrices):
        matrices = [matrices] if isinstance(matrices, ScoringMatrix) else list(matrices)
        if not matrices:
            raise ValueError("a matrix set holds at least one matrix")
        if any(m.sorted_alphabet != matrices[0].sorted_alphabet for m in matrices):
            raise ValueError("the matrices of a set must share one alphabet")
        _ffi.require_gpu()
        self.matrices = matrices
        values = np.ascontiguousarray(np.concatenate([m.values for m in matrices]), dtype=np.float32)
        mat_off = np.concatenate([[0], np.cumsum([m.width for m in matrices])]).astype(np.int32)
        letter_col = np.array([matrices[0].char_to_index[ord(ch)] for ch in LETTERS], dtype=np.int8)
        self._create("bxmi_pwm_create", ptr(values), ptr(mat_off), len(matrices), values.shape[1], ptr(letter_col))
        self.n_mats, self.n_cols, self.max_width = self._info("bxmi_pwm_info", C.c_int32, C.c_int32, C.c_int32)

    def __len__(self):
        return self.n_mats


class _held:
    """`pwms` as a MatrixSet for the length of a call: one the caller made is left open, one made here from matrices is closed"""

    def __init__(self, pwms):
        self.own = not isinstance(pwms, MatrixSet)
        self.set = MatrixSet(pwms) if self.own else pwms

    def __enter__(self):
        return self.set

    def __exit__(self, *exc):
        if self.own:
            self.set.close()


def _stranded(name, strand, args):
    """the entry point and its arguments: the unstranded call, or its _strand sibling with the strand array after `start`"""
    if strand is None:
        return (name,) + tuple(args)
    head, dev = (name[:-4], "_dev") if name.endswith("_dev") else (name, "")
    return (head + "_strand" + dev,) + tuple(args[:4]) + (strand.data_ptr() if hasattr(strand, "data_ptr") else ptr(strand),) + tuple(args[4:])


def site_starts(starts, lengths, pos, width, strands=None):
    """The genomic start of the site at offset `pos` of the strand's string of a row that starts at `starts` (after clipping) and
    holds `lengths` bases, under a matrix of `width` rows: starts + pos on a plus row, starts + lengths - width - pos on a minus
    row.  Arrays broadcast against the rows; pos < 0 (no scored offset) gives -1.  Pure int64 arithmetic: no device is used."""
    starts, lengths, pos = (np.asarray(a, dtype=np.int64) for a in (starts, lengths, pos))
    minus = np.zeros(starts.shape, dtype=bool) if strands is None else _strands(strands, starts.size).astype(bool).reshape(starts.shape)
    at = np.where(minus, starts + lengths - int(width) - pos, starts + pos)
    return np.where(pos < 0, -1, at).astype(np.int64)


def scores(tracks, track_of, starts, ends, pwms, do_mask=True, strands=None):
    """The scores at every offset of regions [starts[i], ends[i]) of tracks[track_of[i]], clipped as `sequence.sequences` clips
    them -> (float32 [n_mats, total], offsets int64 [n + 1]): row i of plane m is [m, offsets[i]:offsets[i + 1]] and equals
    pwms[m].score_string(seq.get(start, end)) of the reference.  `pwms`: a MatrixSet, or matrices (put on the device for this call).
    A minus row (`strands`) is scored on its reverse complement."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    strand = _strands(strands, len(t))
    s64, lengths = _clip([tr.size for tr in tracks], t, s, e)
    offsets = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    with _held(pwms) as ms:
        out = np.empty((ms.n_mats, int(offsets[-1])), dtype=np.float32)
        call(*_stranded("bxmi_twobit_pwm_scores", strand, (_ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), len(t), 0, ptr(offsets),
                                                             out.shape[1], int(bool(do_mask)), ms._h, ptr(out))))
    return out, offsets


def score_matrix(tracks, track_of, starts, width, pwms, do_mask=True, strands=None):
    """The windows [starts[i], starts[i] + width) of tracks[track_of[i]] -> float32 [n_mats, n, width]; a position outside the
    sequence is unscoreable, as is every position of a row that names no track.  width < 1 raises BxmiError (EINVAL)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s = _rows_i32("track_of and starts", track_of, starts)
    strand = _strands(strands, len(t))
    width = int(width)
    with _held(pwms) as ms:
        out = np.empty((ms.n_mats, len(t), max(width, 0)), dtype=np.float32)
        call(*_stranded("bxmi_twobit_pwm_scores", strand, (_ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), width, None, len(t) * max(width, 0),
                                                             int(bool(do_mask)), ms._h, ptr(out))))
    return out


def best(tracks, track_of, starts, ends, pwms, do_mask=True, strands=None):
    """The best hit of every region (clipped as for `scores`) -> (float32 [n_mats, n], int32 [n_mats, n]): the greatest score
    that is not NaN and the first offset within the clipped region that holds it; NaN and -1 where the region has no scored
    offset.  No per-base output is written anywhere.  On a minus row (`strands`) the offset is one of the strand's string, and of
    equal scores the first THERE wins; `site_starts` gives the genomic start."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    strand = _strands(strands, len(t))
    s64, lengths = _clip([tr.size for tr in tracks], t, s, e)
    offsets = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    with _held(pwms) as ms:
        score = np.empty((ms.n_mats, len(t)), dtype=np.float32)
        pos = np.empty((ms.n_mats, len(t)), dtype=np.int32)
        call(*_stranded("bxmi_twobit_pwm_best", strand, (_ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), len(t), 0, ptr(offsets),
                                                           int(offsets[-1]), int(bool(do_mask)), ms._h, ptr(score), ptr(pos))))
    return score, pos


def _thresholds(thresholds, n_mats):
    """a scalar or one value per matrix -> float32 [n_mats]"""
    t = np.asarray(thresholds, dtype=np.float32)
    if t.ndim > 1 or (t.ndim == 1 and len(t) != n_mats):
        raise ValueError("thresholds must be a scalar or one value for each of the %d matrices" % n_mats)
    return np.ascontiguousarray(np.broadcast_to(t, (n_mats,)))


def hits(tracks, track_of, starts, ends, pwms, thresholds, do_mask=True, strands=None):
    """Every offset of regions [starts[i], ends[i]) (clipped as for `scores`) whose score under matrix m is not NaN and is >=
    thresholds[m] (a scalar: one threshold for all) -> (mat_hits int64 [n_mats + 1], rows int32, pos int32, score float32): the
    hits in ascending (matrix, region, offset), matrix m's being [mat_hits[m]:mat_hits[m + 1]] of the three arrays; `pos` is the
    offset within the clipped region, `score` bit for bit the element of `scores`.  In the reference's terms, per matrix and
    region, numpy.nonzero(pwms[m].score_string(seq.get(start, end)) >= thresholds[m]).  No score plane is written anywhere: a
    call that counts, then a call into arrays of exactly that size.  On a minus row (`strands`) `pos` is the offset in the strand's
    string and the hits of a row ascend in it."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    strand = _strands(strands, len(t))
    s64, lengths = _clip([tr.size for tr in tracks], t, s, e)
    offsets = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    with _held(pwms) as ms:
        least = _thresholds(thresholds, ms.n_mats)
        mat_hits = np.zeros(ms.n_mats + 1, dtype=np.int64)
        rows_of = (_ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), len(t), 0, ptr(offsets), int(offsets[-1]), int(bool(do_mask)), ms._h, ptr(least))
        call(*_stranded("bxmi_twobit_pwm_hits", strand, rows_of + (0, ptr(mat_hits), None, None, None)), allow=(_ffi.ERANGE,))
        found = int(mat_hits[-1])
        rows, pos, score = np.empty(found, dtype=np.int32), np.empty(found, dtype=np.int32), np.empty(found, dtype=np.float32)
        if found:
            call(*_stranded("bxmi_twobit_pwm_hits", strand, rows_of + (found, ptr(mat_hits), ptr(rows), ptr(pos), ptr(score))))
    return mat_hits, rows, pos, score


def _copied(strand, strands):
    """the strand tensor where it is a copy made here (of a non-contiguous one), to be recorded as in use on the stream"""
    return (strand,) if strand is not None and strand is not strands else ()


def _device_set(who, pwms):
    if not isinstance(pwms, MatrixSet):
        raise ValueError("%s takes a MatrixSet: the matrices must outlive the queued work" % who)
    return pwms


def scores_dev(tracks, track_of, starts, ends, pwms, do_mask=True, stream=None, strands=None):
    """`scores` on device arrays: int32 torch tensors on the GPU in, (float32 [n_mats, total], offsets int64 [n + 1]) tensors out.
    The clipping and the offsets are computed by torch on its current stream and `total` is read back to size the output -- ONE
    synchronisation; the scores are then queued on torch's current stream (or `stream`: the tensors made here are then recorded
    as in use on it) and not waited for.  `pwms` is a MatrixSet.  One 2bit call at a time, as `sequence.matrix_dev`."""
    import torch

    tracks, ms = list(tracks), _device_set("scores_dev", pwms)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("scores_dev", "scores", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    strand = _strands_dev(strands, n, dev, "scores_dev")
    first, offsets = _clip_dev(tracks, track_of, starts, ends, n, dev)
    total = int(offsets[-1].item()) if n else 0  # (the synchronisation: `first` and `offsets` are complete after it)
    out = torch.empty((ms.n_mats, total), dtype=torch.float32, device=dev)
    call(*_stranded("bxmi_twobit_pwm_scores_dev", strand, (_ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), n, 0, offsets.data_ptr(),
                                                             total, int(bool(do_mask)), ms._h, out.data_ptr(), stream)))
    if total:
        _record(stream, dev, (first, offsets, out) + _copied(strand, strands))
    return out, offsets


def score_matrix_dev(tracks, track_of, starts, width, pwms, do_mask=True, stream=None, out=None, strands=None):
    """`score_matrix` on device arrays: the float32 [n_mats, n, width] tensor -- `out` if given (contiguous, on the rows' device),
    else a new one -- queued on torch's current stream (or `stream`), nothing is waited for."""
    import torch

    tracks, ms = list(tracks), _device_set("score_matrix_dev", pwms)
    (track_of, starts), n, dev, stream = _ffi.device_args("score_matrix_dev", "score_matrix", ("track_of", "starts"), (track_of, starts), stream)
    strand = _strands_dev(strands, n, dev, "score_matrix_dev")
    width = int(width)
    shape = (ms.n_mats, n, max(width, 0))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        made = (out,)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 [n_mats, n, width] tensor on the device of the rows")
    else:
        made = ()
    call(*_stranded("bxmi_twobit_pwm_scores_dev", strand, (_ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), n, width, None,
                                                             n * max(width, 0), int(bool(do_mask)), ms._h, out.data_ptr(), stream)))
    made = made + _copied(strand, strands)
    if made and out.numel():
        _record(stream, dev, made)
    return out


def best_dev(tracks, track_of, starts, ends, pwms, do_mask=True, stream=None, strands=None):
    """`best` on device arrays: (float32 [n_mats, n], int32 [n_mats, n]) tensors, queued on torch's current stream (or `stream`);
    the clipping is torch's, on its current stream, and the host waits for NOTHING: the kernel reads where the rows end from the
    offsets themselves and is given only a bound of it, n times the longest sequence.  Ordering: when `stream` is not torch's
    current stream it is made to wait, on the device, for what the current stream has queued up to the clipping (an event, as
    `Stream.wait_stream`), so the kernels never read offsets that are still being written; the caller's own inputs must be
    complete on the current stream or on `stream`, as for every `_dev` form."""
    import torch

    tracks, ms = list(tracks), _device_set("best_dev", pwms)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("best_dev", "best", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    strand = _strands_dev(strands, n, dev, "best_dev")
    first, offsets = _clip_dev(tracks, track_of, starts, ends, n, dev)
    if stream != torch.cuda.current_stream(dev).cuda_stream:  # the kernels read what torch's current stream is still writing
        torch.cuda.ExternalStream(stream, device=dev).wait_stream(torch.cuda.current_stream(dev))
    score = torch.empty((ms.n_mats, n), dtype=torch.float32, device=dev)
    pos = torch.empty((ms.n_mats, n), dtype=torch.int32, device=dev)
    bound = n * max([tr.size for tr in tracks] + [0])
    call(*_stranded("bxmi_twobit_pwm_best_dev", strand, (_ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), n, 0, offsets.data_ptr(),
                                                           bound, int(bool(do_mask)), ms._h, score.data_ptr(), pos.data_ptr(), stream)))
    if n:
        _record(stream, dev, (first, offsets, score, pos) + _copied(strand, strands))
    return score, pos


def hits_dev(tracks, track_of, starts, ends, pwms, thresholds, do_mask=True, max_hits=None, stream=None, strands=None):
    """`hits` on device arrays: int32 torch tensors on the GPU in -> (mat_hits int64 [n_mats + 1], a HOST numpy array; rows int32,
    pos int32, score float32 tensors on the device).  The clipping is torch's and its total is read back (one synchronisation);
    the call itself waits once more, for the counts.  With `max_hits` the hits go into tensors of that capacity in ONE call -- two
    scoring passes -- and views of the filled part are returned; if they do not fit, BxmiError (ERANGE) with the totals in its
    message.  Without it a call that only counts comes first, so the regions are scored a THIRD time.  The hits are queued on
    torch's current stream (or `stream`) and not waited for.  `pwms` is a MatrixSet.  One 2bit call at a time."""
    import torch

    tracks, ms = list(tracks), _device_set("hits_dev", pwms)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("hits_dev", "hits", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    least = _thresholds(thresholds, ms.n_mats)
    strand = _strands_dev(strands, n, dev, "hits_dev")
    first, offsets = _clip_dev(tracks, track_of, starts, ends, n, dev)
    total = int(offsets[-1].item()) if n else 0  # (the synchronisation: `first` and `offsets` are complete after it)
    mat_hits = np.zeros(ms.n_mats + 1, dtype=np.int64)
    rows_of = (_ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), n, 0, offsets.data_ptr(), total, int(bool(do_mask)), ms._h, ptr(least))
    if max_hits is None:
        call(*_stranded("bxmi_twobit_pwm_hits_dev", strand, rows_of + (0, ptr(mat_hits), None, None, None, stream)), allow=(_ffi.ERANGE,))
        cap = int(mat_hits[-1])
    else:
        cap = int(max_hits)
        if cap < 0:
            raise ValueError("max_hits must not be negative")
    rows = torch.empty(cap, dtype=torch.int32, device=dev)
    pos = torch.empty(cap, dtype=torch.int32, device=dev)
    score = torch.empty(cap, dtype=torch.float32, device=dev)
    if cap or max_hits is not None:
        try:
            call(*_stranded("bxmi_twobit_pwm_hits_dev", strand, rows_of + (cap, ptr(mat_hits), rows.data_ptr() if cap else None,
                                                                   pos.data_ptr() if cap else None, score.data_ptr() if cap else None, stream)))
        except _ffi.BxmiError as err:
            if err.code == _ffi.ERANGE:
                raise _ffi.BxmiError(err.code, "%s (max_hits = %d; hits per matrix: %s)" % (err, cap, np.diff(mat_hits).tolist())) from None
            raise
    found = int(mat_hits[-1])
    if total:
        _record(stream, dev, (first, offsets, rows, pos, score) + _copied(strand, strands))
    return mat_hits, rows[:found], pos[:found], score[:found]
