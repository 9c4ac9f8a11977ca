"""
Per-base score tracks on the MI355X: the average, minimum and maximum of a score track (phastCons and the like) over a
whole array of intervals per call -- the engine under ``bxmi.cli.aggregate_scores_in_intervals`` (reference:
scripts/aggregate_scores_in_intervals.py:107-134 over lib/bx/binned_array.py).

``ScoreTrack`` is one chromosome's scores as a dense float32 array in HBM (``bxmi_scores_*`` of include/bxmi.h), NaN = no
score.  ``aggregate`` answers from host arrays, ``aggregate_dev`` from device arrays.  The sums are the reference's bit for
bit: float32, added in position order.

``profile`` / ``profile_dev`` are the site profile of scripts/bed_bigwig_profile.py:27-41 over any number of tracks: per offset of
a window, the float64 sum over all windows in input order and the number of windows with a score there -- the engine under
``bxmi.cli.bed_bigwig_profile``.
"""
import collections
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import as_i32, call, ptr

# per interval: valid bases, their ordered float32 sum, their smallest and largest score (+inf / -inf where count == 0)
Aggregate = collections.namedtuple("Aggregate", "count total minimum maximum")

# per window offset: the float64 sum over the windows in input order, the windows with a score there; and how many columns had to
# take the ordered chain because their parallel sum was not provably the same bits
Profile = collections.namedtuple("Profile", "totals valid chain_columns")

MIN_SENTINEL, MAX_SENTINEL = 100000000, -100000000  # aggregate_scores_in_intervals.py:112-113


def _mask_handle(mask):
    """The bxmi_bits_t behind a mask: None, a bxmi.bitset.DeviceBitSet, or a drop-in bx.bitset set (its queue is flushed)."""
    if mask is None:
        return None
    if hasattr(mask, "_flush"):
        mask._flush()
        mask = mask._d
    return mask._h


class ScoreTrack:
    """float32 scores of positions [0, size) resident on the device; every position starts without a score (NaN)."""

    def __init__(self, size):
        _ffi.require_gpu()
        h = C.c_void_p()
        call("bxmi_scores_create", int(size), C.byref(h))
        self._h = h
        self.size = int(size)

    def close(self):
        if self._h is not None:
            _ffi.load().bxmi_scores_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def values_dev(self):
        """(device pointer, n) of the float32 array."""
        p, n = C.c_void_p(), C.c_int64(0)
        call("bxmi_scores_values_dev", self._h, C.byref(p), C.byref(n))
        return p.value, n.value

    def write(self, offset, values):
        """values -> track[offset : offset + len(values)]"""
        v = np.ascontiguousarray(values, dtype=np.float32)
        call("bxmi_scores_write", self._h, int(offset), ptr(v), len(v))

    def read(self, offset=0, n=None):
        """track[offset : offset + n] as a numpy float32 array (to the end when n is None)"""
        n = self.size - int(offset) if n is None else int(n)
        out = np.empty(max(n, 0), dtype=np.float32)
        call("bxmi_scores_read", self._h, int(offset), ptr(out), n)
        return out

    def set_spans(self, starts, ends, values):
        """track[starts[i]:ends[i]] = values[i], in order: where spans overlap the later one wins.  Spans are clipped to the track."""
        s, e = as_i32(starts), as_i32(ends)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if not (s.shape == e.shape == v.shape) or s.ndim != 1:
            raise ValueError("starts, ends and values must be 1-d arrays of equal length")
        call("bxmi_scores_set_spans", self._h, ptr(s), ptr(e), ptr(v), len(s))

    def aggregate(self, starts, ends, mask=None):
        """count, ordered float32 sum, minimum and maximum of the valid scores of every [starts[i], ends[i]) -> Aggregate of numpy
        arrays.  Valid: not NaN, not +-0, and not set in `mask` (a DeviceBitSet or a bx.bitset set; None = nothing is masked)."""
        s, e = as_i32(starts), as_i32(ends)
        if s.shape != e.shape or s.ndim != 1:
            raise ValueError("starts and ends must be 1-d arrays of equal length")
        n = len(s)
        count = np.empty(n, dtype=np.int32)
        total, mn, mx = (np.empty(n, dtype=np.float32) for _ in range(3))
        call("bxmi_scores_aggregate", self._h, _mask_handle(mask), ptr(s), ptr(e), n, ptr(count), ptr(total), ptr(mn), ptr(mx))
        return Aggregate(count, total, mn, mx)

    def aggregate_ptrs(self, mask, start_ptr, end_ptr, n, count_ptr, total_ptr, min_ptr, max_ptr, stream=None):
        """bxmi_scores_aggregate_dev as it stands: device pointers in, nothing waited for."""
        call("bxmi_scores_aggregate_dev", self._h, _mask_handle(mask), start_ptr, end_ptr, int(n), count_ptr, total_ptr, min_ptr, max_ptr, stream)

    def aggregate_dev(self, starts, ends, mask=None, stream=None):
        """`aggregate` on device arrays: int32 torch tensors on the GPU in, an Aggregate of torch tensors out, queued on torch's
        current stream (or `stream`); nothing is waited for."""
        import torch

        (starts, ends), n, dev, stream = _ffi.device_args("aggregate_dev", "aggregate", ("starts", "ends"), (starts, ends), stream)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        total, mn, mx = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        self.aggregate_ptrs(mask, starts.data_ptr(), ends.data_ptr(), n, count.data_ptr(), total.data_ptr(), mn.data_ptr(), mx.data_ptr(),
                            stream=stream)
        return Aggregate(count, total, mn, mx)

    def profile(self, win_starts, width):
        """`profile` of windows that all lie on this track."""
        return profile([self], np.zeros(len(win_starts), dtype=np.int32), win_starts, width)


def profile(tracks, track_of, win_starts, width):
    """Site profile over windows [win_starts[i], win_starts[i] + width) of tracks[track_of[i]] (-1: no track) -> Profile of numpy
    arrays: totals (float64, the reference's `totals` of bed_bigwig_profile.py:38 bit for bit: one chain over the windows in input
    order, whatever tracks they interleave), valid (int32) and chain_columns (int).  Positions outside a track, NaN there and
    windows without a track have no score -- the reference raises OverflowError on a negative window start and fails on an
    unknown chromosome; here those positions have no data.  +-0 is a score.  The profile itself is totals / valid."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s = as_i32(track_of), as_i32(win_starts)
    if t.shape != s.shape or t.ndim != 1:
        raise ValueError("track_of and win_starts must be 1-d arrays of equal length")
    width = int(width)
    totals = np.zeros(max(width, 0), dtype=np.float64)
    valid = np.zeros(max(width, 0), dtype=np.int32)
    chain = C.c_int64(0)
    call("bxmi_scores_profile", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), width, ptr(totals), ptr(valid), C.byref(chain))
    return Profile(totals, valid, chain.value)


def profile_dev(tracks, track_of, win_starts, width, stream=None):
    """`profile` on device arrays: int32 torch tensors on the GPU in, a Profile of torch tensors out (totals float64[width], valid
    int32[width], chain_columns int64[1]), queued on torch's current stream (or `stream`); nothing is waited for.  An entry of
    track_of outside [0, len(tracks)) means no track (the device form cannot report it)."""
    import torch

    tracks = list(tracks)
    (track_of, win_starts), n, dev, stream = _ffi.device_args("profile_dev", "profile", ("track_of", "win_starts"), (track_of, win_starts), stream)
    width = int(width)
    totals = torch.empty(max(width, 0), dtype=torch.float64, device=dev)
    valid = torch.empty(max(width, 0), dtype=torch.int32, device=dev)
    chain = torch.empty(1, dtype=torch.int64, device=dev)
    call("bxmi_scores_profile_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), win_starts.data_ptr(), n, width, totals.data_ptr(),
         valid.data_ptr(), chain.data_ptr(), stream)
    return Profile(totals, valid, chain)


def format_row(chrom, start, stop, count, total, minimum, maximum):
    """One output line (without the newline) as aggregate_scores_in_intervals.py:127-134 prints it.  The average is the
    float32 quotient total / count; the reference's minimum starts as the int 100000000 and is replaced by a score only
    through min(score, minimum), so it survives -- and prints without a fraction -- when every valid score is above 1e8;
    likewise the maximum and -100000000."""
    if count > 0:
        avg = np.float32(total) / int(count)
        mn, mx = np.float32(minimum), np.float32(maximum)
        mn = mn if mn <= MIN_SENTINEL else MIN_SENTINEL
        mx = mx if mx >= MAX_SENTINEL else MAX_SENTINEL
    else:
        avg = mn = mx = "nan"
    return "\t".join(map(str, [chrom, start, stop, avg, mn, mx]))
