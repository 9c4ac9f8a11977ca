"""
Binned bigWig summaries on the MI355X: ``BigWigFile.summarize_from_full`` / ``query`` (reference: lib/bx/bbi/bbi_file.pyx:66-111,
187-260 under bigwig_file.pyx:93-108, 176-185) for a whole array of regions per call -- the site x bin matrix behind a heatmap in
one device pass -- and the engine under ``bx.bbi.bigwig_file`` and ``bxmi.cli.bigwig_summary``.

``SpanTrack`` is one chromosome's bigWig items (start, end, value) resident in HBM in file order (``bxmi_spans_*`` of
include/bxmi.h).  ``summarize`` answers from host arrays, ``summarize_dev`` from device arrays; both give the reference's five
arrays per region bit for bit: every bin is its ordered float64 chain over the items that overlap it, products and sums rounded
separately.  ``stats`` derives mean, coverage and standard deviation as ``query`` does.  Zoom levels are not used: these are the
answers from full data.
"""
import collections
import ctypes as C

import numpy as np

from . import _ffi, bigwig
from ._ffi import as_i32, call, ptr

# [n, size] float64 each: rounded sum of weights, smallest and largest value (+inf / -inf for an empty bin), sum of value * weight,
# sum of value^2 * weight
Summary = collections.namedtuple("Summary", "valid_count min_val max_val sum_data sum_squares")


class SpanTrack:
    """(start, end, value) items of one chromosome on the device, in the order given (file order).  `ordered`: starts and ends are
    both non-decreasing, which every real bigWig is; other tracks are summarized by a slow general path."""

    def __init__(self, starts, ends, values):
        _ffi.require_gpu()
        s, e = as_i32(starts), as_i32(ends)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if not (s.shape == e.shape == v.shape) or s.ndim != 1:
            raise ValueError("starts, ends and values must be 1-d arrays of equal length")
        h = C.c_void_p()
        call("bxmi_spans_create", ptr(s), ptr(e), ptr(v), len(s), C.byref(h))
        self._h = h
        n, ordered = C.c_int64(0), C.c_int(0)
        call("bxmi_spans_info", self._h, C.byref(n), C.byref(ordered))
        self.n, self.ordered = n.value, bool(ordered.value)

    @classmethod
    def from_bigwig(cls, path):
        """{chrom: SpanTrack} of a bigWig file, chromosomes without data included."""
        return {chrom: cls(*spans) for chrom, spans in bigwig.read_spans_file(path).items()}

    def close(self):
        if self._h is not None:
            _ffi.load().bxmi_spans_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def summarize(tracks, track_of, starts, ends, size):
    """summarize_from_full of regions [starts[i], ends[i]) of tracks[track_of[i]], `size` bins each -> Summary of [n, size] float64
    numpy arrays.  track_of[i] < 0 (unknown chromosome) or starts[i] >= ends[i] -- where the reference returns None -- gives an
    empty row: 0, +inf, -inf, 0, 0.  A negative coordinate or size < 1 raises BxmiError (EINVAL)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = as_i32(track_of), as_i32(starts), as_i32(ends)
    if not (t.shape == s.shape == e.shape) or t.ndim != 1:
        raise ValueError("track_of, starts and ends must be 1-d arrays of equal length")
    size = int(size)
    out = [np.empty((len(t), max(size, 0)), dtype=np.float64) for _ in range(5)]
    call("bxmi_spans_summarize", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(e), len(t), size, *[ptr(a) for a in out])
    return Summary(*out)


def summarize_dev(tracks, track_of, starts, ends, size, stream=None):
    """`summarize` on device arrays: int32 torch tensors on the GPU in, a Summary of [n, size] float64 torch tensors out, queued on
    torch's current stream (or `stream`); nothing is waited for.  An entry of track_of outside [0, len(tracks)) or a negative
    coordinate gives an empty row (the device form cannot report it).  The table of tracks the kernel reads belongs to the library and
    is rewritten by every call on that call's stream: ONE summary call at a time per process may be in flight on the device.  Calls
    on one stream follow each other; before a call on another stream, or with other tracks from another thread, wait for the one
    before it."""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("summarize_dev", "summarize", ("track_of", "starts", "ends"),
                                                                (track_of, starts, ends), stream)
    size = int(size)
    out = [torch.empty((n, max(size, 0)), dtype=torch.float64, device=dev) for _ in range(5)]
    call("bxmi_spans_summarize_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), ends.data_ptr(), n, size,
         *[a.data_ptr() for a in out], stream)
    return Summary(*out)


def stats(summary, starts, ends, size):
    """(mean, coverage, std_dev), [n, size] each, as BBIFile.query derives them (bbi_file.pyx:245-258):
        mean = sum / valid (0 / 0 is NaN); coverage = size / (end - start) * valid;
        variance = sum_squares - sum * sum / valid, divided by valid - 1 where valid > 1; std_dev = sqrt(max(variance, 0)), NaN kept.
    numpy arrays on the host; torch tensors (a summarize_dev result with `starts` / `ends` tensors) stay on the device, one
    elementwise operation per step -- neither form fuses a multiply into an add, which would change the variance's bits.  The host
    form is the reference's `query` bit for bit, and so is the torch form on the device (torch's float64 division and square
    root there are the IEEE ones: 4 M random inputs each agreed with numpy's).  Tensors on the CPU are another matter: torch's
    float64 square root there is one ulp off the correctly rounded root for about 1 % of inputs.  Rows
    with starts >= ends have no meaning here (their coverage divides by the span); the callers skip them."""
    valid, sm, sq = summary.valid_count, summary.sum_data, summary.sum_squares
    if isinstance(valid, np.ndarray):
        span = (np.asarray(ends, dtype=np.int64) - np.asarray(starts, dtype=np.int64)).astype(np.float64)[:, None]
        with np.errstate(all="ignore"):
            mean = sm / valid
            coverage = (float(size) / span) * valid
            variance = sq - (sm * sm) / valid
            variance = np.where(valid > 1, variance / (valid - 1), variance)
            std_dev = np.sqrt(np.where(variance < 0, 0.0, variance))
        return mean, coverage, std_dev
    import torch

    span = (ends.to(torch.int64) - starts.to(torch.int64)).to(torch.float64)[:, None]
    mean = sm / valid
    coverage = torch.div(torch.full_like(span, float(size)), span) * valid  # (scalar / tensor would be reciprocal * scalar: two roundings)
    product = sm * sm
    variance = sq - product / valid
    variance = torch.where(valid > 1, variance / (valid - 1), variance)
    std_dev = torch.sqrt(torch.where(variance < 0, torch.zeros_like(variance), variance))
    return mean, coverage, std_dev
