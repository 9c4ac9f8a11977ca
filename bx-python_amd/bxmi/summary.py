"""
Binned bigWig summaries on the MI355X: ``BigWigFile.summarize_from_full`` / ``query`` (reference: lib/bx/bbi/bbi_file.pyx:66-111,
187-260 under bigwig_file.pyx:93-108, 176-185) for a whole array of regions per call -- the site x bin matrix behind a heatmap in
one device pass -- and the engine under ``bx.bbi.bigwig_file`` and ``bxmi.cli.bigwig_summary``.

``SpanTrack`` is one chromosome's bigWig items (start, end, value) resident in HBM in file order (``bxmi_spans_*`` of
include/bxmi.h).  ``summarize`` answers from host arrays, ``summarize_dev`` from device arrays; both give the reference's five
arrays per region bit for bit: every bin is its ordered float64 chain over the items that overlap it, products and sums rounded
separately.  ``stats`` derives mean, coverage and standard deviation as ``query`` does.  These are the answers from full data.

``arrays`` / ``matrix`` (``arrays_dev`` / ``matrix_dev`` on device arrays) are the UNREDUCED form, ``BigWigFile.get_as_array``
(bigwig_file.pyx:122-137, 200-211) for a whole batch per call: every row's per-base float32 values, NaN where the file has no
data, the later item winning where items overlap -- ragged rows one after another, or the site x base matrix [n, width] behind a
base-resolution heatmap, which stays on the device with the ``_dev`` forms (``bxmi_spans_arrays*``).

``ZoomTrack`` is one chromosome's part of one zoom level (``bxmi_zoom_*``; bbi_file.pyx:296-432): ``summarize_zoom`` and
``summarize_zoom_dev`` answer a batch from such tracks as the reference's ``ZoomLevel._summarize`` does, bit for bit -- float32
accumulators fed by float64 products and sums.  ``pick_level`` is the reference's choice of a level, and ``TrackSet`` is a whole
file on the device: its ``summarize`` answers a mixed batch as ``BigWigFile.summarize`` would, each row from the level the rule
picks for it or from full data, in two device calls.  The drop-in ``bx.bbi.bigwig_file.BigWigFile`` and
``bxmi.cli.bigwig_summary`` use zoom levels only when asked (``use_zoom=True``, ``-z``): their default is kept for compatibility
with tests that pin the earlier behaviour, and is meant to flip later.

``BedTrack`` is one chromosome's bigBed records (start, end) in file order (``bxmi_beds_*``; lib/bx/bbi/bigbed_file.pyx):
``summarize_beds`` and ``summarize_beds_dev`` give ``BigBedFile.summarize_from_full`` -- the coverage of every bin by the records,
each weighted as a bigWig item of value 1 -- bit for bit, at the cost of a region's own records although their ends are not in
order.  ``BedSet`` is a whole bigBed file on the device, the counterpart of ``TrackSet``; it is the engine under
``bx.bbi.bigbed_file`` and ``bxmi.cli.bigbed_summary``.
"""
import collections
import ctypes as C

import numpy as np

from . import _ffi, bigbed, bigwig
from ._ffi import as_i32, call, ptr

# [n, size] float64 each: rounded sum of weights, smallest and largest value (+inf / -inf for an empty bin), sum of value * weight,
# sum of value^2 * weight
Summary = collections.namedtuple("Summary", "valid_count min_val max_val sum_data sum_squares")


class _Track:
    """What the three kinds of track share: the handle `_h` that `_create` makes and `close` (or the collector) gives back to
    the library's `_destroy`."""

    _destroy = None  # the C symbol
    _h = None

    def _create(self, symbol, *args):
        h = C.c_void_p()
        call(symbol, *args, C.byref(h))
        self._h = h

    def _info(self, symbol, *ctypes):
        """the values `symbol` reports about the handle"""
        out = [c(0) for c in ctypes]
        call(symbol, self._h, *[C.byref(o) for o in out])
        return [o.value for o in out]

    def close(self):
        if self._h is not None:
            getattr(_ffi.load(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rows_i32(names, *columns):
    """the columns of a batch as int32 arrays: 1-d and of one length, or ValueError naming them"""
    cols = [as_i32(c) for c in columns]
    if cols[0].ndim != 1 or any(c.shape != cols[0].shape for c in cols):
        raise ValueError("%s must be 1-d arrays of equal length" % names)
    return cols


def _summarize(symbol, tracks, track_of, starts, ends, size):
    """the host form of every kind: `symbol` is the C entry point"""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    size = int(size)
    out = [np.empty((len(t), max(size, 0)), dtype=np.float64) for _ in range(5)]
    call(symbol, _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(e), len(t), size, *[ptr(a) for a in out])
    return Summary(*out)


def _summarize_dev(symbol, name, tracks, track_of, starts, ends, size, stream):
    """the device form of every kind: `name` is the public function's, for _ffi.device_args' messages"""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args(name + "_dev", name, ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    size = int(size)
    out = [torch.empty((n, max(size, 0)), dtype=torch.float64, device=dev) for _ in range(5)]
    call(symbol, _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), ends.data_ptr(), n, size, *[a.data_ptr() for a in out], stream)
    return Summary(*out)


class SpanTrack(_Track):
    """(start, end, value) items of one chromosome on the device, in the order given (file order).  `ordered`: starts and ends are
    both non-decreasing, which every real bigWig is; other tracks are summarized by a slow general path."""

    _destroy = "bxmi_spans_destroy"

    def __init__(self, starts, ends, values):
        _ffi.require_gpu()
        s, e = as_i32(starts), as_i32(ends)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if not (s.shape == e.shape == v.shape) or s.ndim != 1:
            raise ValueError("starts, ends and values must be 1-d arrays of equal length")
        self._create("bxmi_spans_create", ptr(s), ptr(e), ptr(v), len(s))
        n, ordered = self._info("bxmi_spans_info", C.c_int64, C.c_int)
        self.n, self.ordered = n, bool(ordered)

    @classmethod
    def from_bigwig(cls, path):
        """{chrom: SpanTrack} of a bigWig file, chromosomes without data included."""
        return {chrom: cls(*spans) for chrom, spans in bigwig.read_spans_file(path).items()}


def summarize(tracks, track_of, starts, ends, size):
    """summarize_from_full of regions [starts[i], ends[i]) of tracks[track_of[i]], `size` bins each -> Summary of [n, size] float64
    numpy arrays.  track_of[i] < 0 (unknown chromosome) or starts[i] >= ends[i] -- where the reference returns None -- gives an
    empty row: 0, +inf, -inf, 0, 0.  A negative coordinate or size < 1 raises BxmiError (EINVAL)."""
    return _summarize("bxmi_spans_summarize", tracks, track_of, starts, ends, size)


def summarize_dev(tracks, track_of, starts, ends, size, stream=None):
    """`summarize` on device arrays: int32 torch tensors on the GPU in, a Summary of [n, size] float64 torch tensors out, queued on
    torch's current stream (or `stream`); nothing is waited for.  An entry of track_of outside [0, len(tracks)) or a negative
    coordinate gives an empty row (the device form cannot report it).  The table of tracks the kernel reads belongs to the library and
    is rewritten by every call on that call's stream: ONE summary call at a time per process may be in flight on the device.  Calls
    on one stream follow each other; before a call on another stream, or with other tracks from another thread, wait for the one
    before it."""
    return _summarize_dev("bxmi_spans_summarize_dev", "summarize", tracks, track_of, starts, ends, size, stream)


def arrays(tracks, track_of, starts, ends):
    """get_as_array of regions [starts[i], ends[i]) of tracks[track_of[i]] -> (values float32[total], offsets int64[n + 1]): row i
    is values[offsets[i]:offsets[i + 1]], its per-base values -- NaN (numpy's) where no item covers the base, the value of the
    LAST covering item in file order elsewhere, its bits unchanged.  A row with ends[i] <= starts[i] is empty; track_of[i] < 0
    (unknown chromosome) is a NaN row; a base below 0 or at 2^31-1 and beyond holds no data.  One device pass over the OUTPUT: rows
    of one base and rows of millions cost their bases."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    offsets = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(np.maximum(e.astype(np.int64) - s.astype(np.int64), 0), out=offsets[1:])
    values = np.empty(int(offsets[-1]), dtype=np.float32)
    call("bxmi_spans_arrays", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), 0, ptr(offsets), len(values), ptr(values))
    return values, offsets


def matrix(tracks, track_of, win_starts, width):
    """get_as_array of the windows [win_starts[i], win_starts[i] + width) of tracks[track_of[i]] -> float32 [n, width]; values as
    `arrays`.  width < 1 raises BxmiError (EINVAL)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s = _rows_i32("track_of and win_starts", track_of, win_starts)
    width = int(width)
    out = np.empty((len(t), max(width, 0)), dtype=np.float32)
    call("bxmi_spans_arrays", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), width, None, out.size, ptr(out))
    return out


def arrays_dev(tracks, track_of, starts, ends, stream=None):
    """`arrays` on device arrays: int32 torch tensors on the GPU in, (values float32[total], offsets int64[n + 1]) tensors out.  The
    offsets are computed by torch on its current stream and `total` is read back to size the output -- ONE synchronisation; the
    values are then queued on torch's current stream (or `stream`) and not waited for.  Unchecked entries as `summarize_dev`: a
    track_of outside [0, len(tracks)) is a NaN row.  One summary call of any kind at a time per process may be in flight."""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("arrays_dev", "arrays", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum((ends.to(torch.int64) - starts.to(torch.int64)).clamp_(min=0), 0, out=offsets[1:])
    total = int(offsets[-1].item()) if n else 0
    values = torch.empty(total, dtype=torch.float32, device=dev)
    call("bxmi_spans_arrays_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), n, 0, offsets.data_ptr(), total,
         values.data_ptr(), stream)
    return values, offsets


def matrix_dev(tracks, track_of, win_starts, width, stream=None, out=None):
    """`matrix` on device arrays: int32 torch tensors on the GPU in, the float32 [n, width] tensor out -- `out` if given (contiguous
    float32 [n, width] on the same device; 16-byte aligned it is written by 16-byte stores, otherwise element by element, with the
    same result), else a new one.  Queued on torch's current stream (or `stream`), nothing is waited for: the matrix stays on the
    device.  Unchecked entries and the one-call-at-a-time rule: as `arrays_dev`."""
    import torch

    tracks = list(tracks)
    (track_of, win_starts), n, dev, stream = _ffi.device_args("matrix_dev", "matrix", ("track_of", "win_starts"), (track_of, win_starts), stream)
    width = int(width)
    if out is None:
        out = torch.empty((n, max(width, 0)), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, width) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 [n, width] tensor on the device of the rows")
    call("bxmi_spans_arrays_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), win_starts.data_ptr(), n, width, None, out.numel(),
         out.data_ptr(), stream)
    return out


class BedTrack(_Track):
    """(start, end) records of one chromosome of a bigBed file on the device, in the order given (file order); no values: every
    record counts 1.  `sorted`: the starts never descend, which holds in every real bigBed whatever its ends do; other tracks are
    summarized by a slow general walk."""

    _destroy = "bxmi_beds_destroy"

    def __init__(self, starts, ends):
        _ffi.require_gpu()
        s, e = _rows_i32("starts and ends", starts, ends)
        self._create("bxmi_beds_create", ptr(s), ptr(e), len(s))
        n, is_sorted = self._info("bxmi_beds_info", C.c_int64, C.c_int)
        self.n, self.sorted = n, bool(is_sorted)

    @classmethod
    def from_bigbed(cls, path):
        """{chrom: BedTrack} of a bigBed file, chromosomes without records included."""
        return {chrom: cls(s, e) for chrom, (s, e, _) in bigbed.read_items_file(path).items()}


def summarize_beds(tracks, track_of, starts, ends, size):
    """BigBedFile.summarize_from_full of regions [starts[i], ends[i]) of the BedTrack tracks[track_of[i]], `size` bins each ->
    Summary of [n, size] float64 numpy arrays: what `summarize` gives for the same records as items of value 1.  valid_count is
    the rounded coverage chain, sum_data and sum_squares the chain itself, min_val and max_val 1 where a record overlaps the bin
    (+inf / -inf elsewhere).  Empty rows and errors as `summarize`."""
    return _summarize("bxmi_beds_summarize", tracks, track_of, starts, ends, size)


def summarize_beds_dev(tracks, track_of, starts, ends, size, stream=None):
    """`summarize_beds` on device arrays, as `summarize_dev`: int32 torch tensors on the GPU in, float64 tensors out, queued on
    torch's current stream (or `stream`).  It shares the library's track table with the other summaries: one summary call of any
    kind at a time per process may be in flight."""
    return _summarize_dev("bxmi_beds_summarize_dev", "summarize_beds", tracks, track_of, starts, ends, size, stream)


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


class ZoomTrack(_Track):
    """One chromosome's part of one zoom level on the device: `arrays` is a bxmi.bigwig.ZoomArrays (records in load order and the
    leaf entries that decide what a region loads).  Only an ORDERED level is accepted (bxmi.bigwig.ordered_level): anything else
    raises BxmiError (EINVAL) naming the condition."""

    _destroy = "bxmi_zoom_destroy"

    def __init__(self, arrays):
        _ffi.require_gpu()
        a = arrays
        rec = [as_i32(a.start), as_i32(a.end), np.ascontiguousarray(a.valid, dtype=np.uint32)]
        rec += [np.ascontiguousarray(x, dtype=np.float32) for x in (a.min, a.max, a.sum, a.sumsq)]
        leaf = [as_i32(a.leaf_lo), as_i32(a.leaf_hi)]
        first = np.ascontiguousarray(a.leaf_first, dtype=np.int64)
        if any(x.ndim != 1 or x.shape != rec[0].shape for x in rec) or leaf[0].shape != leaf[1].shape or first.shape != (len(leaf[0]) + 1,):
            raise ValueError("seven record arrays of one length, leaf_lo and leaf_hi of one length, leaf_first one longer")
        self._create("bxmi_zoom_create", *[ptr(x) for x in rec], len(rec[0]), ptr(leaf[0]), ptr(leaf[1]), ptr(first), len(leaf[0]))
        self.n, self.n_leaves = self._info("bxmi_zoom_info", C.c_int64, C.c_int64)

    @classmethod
    def from_bigwig(cls, path):
        """{chrom: [ZoomTrack per level, in file order]} of a bigWig file; every level must be ordered."""
        levels = bigwig.read_zoom_file(path)
        return {chrom: [cls(per[chrom]) for _, per in levels] for chrom in (levels[0][1] if levels else bigwig.chroms(path))}


def summarize_zoom(tracks, track_of, starts, ends, size):
    """ZoomLevel._summarize of regions [starts[i], ends[i]) from the ZoomTrack tracks[track_of[i]], `size` bins each -> Summary of
    [n, size] float64 numpy arrays; valid_count is not a whole number here.  A bin without a record left is 0, NaN, NaN, 0, 0.
    track_of[i] < 0 or starts[i] >= ends[i] -- where the reference returns None -- gives the empty row of `summarize`: 0, +inf,
    -inf, 0, 0.  A negative coordinate or size < 1 raises BxmiError (EINVAL)."""
    return _summarize("bxmi_zoom_summarize", tracks, track_of, starts, ends, size)


def summarize_zoom_dev(tracks, track_of, starts, ends, size, stream=None):
    """`summarize_zoom` on device arrays, as `summarize_dev`: int32 torch tensors on the GPU in, float64 tensors out, queued on
    torch's current stream (or `stream`).  It shares the library's track table with `summarize_dev`: one summary call of either kind
    at a time per process may be in flight."""
    return _summarize_dev("bxmi_zoom_summarize_dev", "summarize_zoom", tracks, track_of, starts, ends, size, stream)


def pick_levels(reductions, starts, ends, size):
    """The zoom level BBIFile.summarize takes for `size` bins over each [starts[i], ends[i]) (bbi_file.pyx:205-215, 281-294): int32
    [n] of indices into `reductions` (the levels' reduction_level in file order, sorted or not), -1 for full data.  desired =
    ((end - start) // size) // 2; no level when desired <= 1; else the level with the smallest desired - reduction >= 0, the
    first in file order among equals."""
    desired = ((np.asarray(ends, dtype=np.int64) - np.asarray(starts, dtype=np.int64)) // int(size)) // 2
    level, best = np.full(len(desired), -1, dtype=np.int32), np.full(len(desired), np.iinfo(np.int64).max)
    for k, r in enumerate(reductions):
        diff = desired - int(r)
        take = (desired > 1) & (diff >= 0) & (diff < best)
        level[take], best[take] = k, diff[take]
    return level


def pick_level(reductions, start, end, size):
    """`pick_levels` for one region: an index into `reductions`, or None for full data."""
    k = int(pick_levels(reductions, [start], [end], size)[0])
    return None if k < 0 else k


NOT_ORDERED = ("the reference answers this region from a zoom level that is not ordered (%s), which is not implemented: "
               "call summarize_from_full for the answer from full data")


class _FileSet:
    """What TrackSet and BedSet share: every chromosome's full data as one track (`self.full`: {chrom: track}, summarized by
    `_summarize_full`) and its part of every zoom level (ZoomTrack; None in place of a part that is not ordered), and `summarize`,
    which answers a batch as the reference's BBIFile.summarize would, row by row."""

    _summarize_full = None  # summarize or summarize_beds

    def _set_levels(self, levels):
        self.reductions = [r for r, _ in levels]
        self.not_ordered = {}
        self.zoom = []  # one track per (chromosome, level), chromosome-major: track_of = chromosome * levels + level
        for chrom in self.chroms:
            for k, (_, per) in enumerate(levels):
                why = bigwig.ordered_level(per[chrom])
                if why:
                    self.not_ordered[len(self.zoom)] = why
                self.zoom.append(None if why else ZoomTrack(per[chrom]))

    def close(self):
        _ffi.close_all(list(self.full.values()) + [t for t in self.zoom if t is not None])

    def _track_of(self, chroms):
        """int32 positions in self.chroms of `chroms` (names, or an int array of such positions already), -1 for an unknown one"""
        chroms = np.asarray(chroms)
        if chroms.dtype.kind in "iu":
            track_of = as_i32(chroms)
        else:
            index = {chrom: k for k, chrom in enumerate(self.chroms)}
            track_of = np.array([index.get(c, -1) for c in chroms.tolist()], dtype=np.int32)
        if track_of.ndim != 1:
            raise ValueError("chroms, starts and ends must be 1-d arrays of equal length")
        if len(track_of) and track_of.max() >= len(self.chroms):
            raise ValueError("a chromosome position beyond the file's %d chromosomes" % len(self.chroms))
        return track_of

    def summarize(self, chroms, starts, ends, size, zoom=True):
        """BBIFile.summarize for a batch: `size` bins over chroms[i]:starts[i]-ends[i] -> Summary of [n, size] float64 arrays.
        `chroms`: names, or an int array of positions in self.chroms (-1: unknown).  With `zoom`, a row for which the reference's
        rule picks a level is answered from that level and the others from full data: ONE call of each kind, the zoom call's table
        listing every (chromosome, level) track.  Without it every row comes from full data.  An unknown chromosome or start >= end
        gives the empty row 0, +inf, -inf, 0, 0.  A row that needs a level which is not ordered raises NotImplementedError."""
        summarize_full = type(self)._summarize_full
        track_of = self._track_of(chroms)
        s, e = as_i32(starts), as_i32(ends)
        if not (track_of.shape == s.shape == e.shape) or s.ndim != 1:
            raise ValueError("chroms, starts and ends must be 1-d arrays of equal length")
        size = int(size)
        if size < 1 or not zoom or not self.reductions:
            return summarize_full(self.full.values(), track_of, s, e, size)
        level = pick_levels(self.reductions, s, e, size)
        from_zoom = (level >= 0) & (track_of >= 0)  # (a row without a chromosome is the reference's None: the full call's empty row)
        if not from_zoom.any():
            return summarize_full(self.full.values(), track_of, s, e, size)
        rows = np.nonzero(from_zoom)[0]
        zoom_track = track_of[rows] * len(self.reductions) + level[rows]
        for t in np.unique(zoom_track):
            if int(t) in self.not_ordered:
                raise NotImplementedError(NOT_ORDERED % self.not_ordered[int(t)])
        # (a handle array has no holes: the tracks that exist, renumbered)
        kept = [k for k, t in enumerate(self.zoom) if t is not None]
        renumber = np.full(len(self.zoom), -1, dtype=np.int32)
        renumber[kept] = np.arange(len(kept), dtype=np.int32)
        part = summarize_zoom([self.zoom[k] for k in kept], renumber[zoom_track], s[rows], e[rows], size)
        if from_zoom.all():
            return part
        rest = np.nonzero(~from_zoom)[0]
        full = summarize_full(self.full.values(), track_of[rest], s[rest], e[rest], size)
        out = [np.empty((len(s), size), dtype=np.float64) for _ in range(5)]
        for o, a, b in zip(out, part, full):
            o[rows], o[rest] = a, b
        return Summary(*out)


class TrackSet(_FileSet):
    """A whole bigWig file on the device: every chromosome's items (SpanTrack) and its part of every zoom level (ZoomTrack; None in
    place of a part that is not ordered).  `summarize` answers a batch as the reference's BigWigFile.summarize would, row by row."""

    _summarize_full = staticmethod(summarize)

    def __init__(self, spans, levels):
        """spans: bigwig.read_spans_file's result; levels: bigwig.read_zoom_file's"""
        self.chroms = list(spans)
        self.spans = self.full = {chrom: SpanTrack(*spans[chrom]) for chrom in self.chroms}
        self._set_levels(levels)

    @classmethod
    def from_bigwig(cls, path=None, data=None):
        return cls(bigwig.read_spans_file(path, data=data), bigwig.read_zoom_file(path, data=data))

    def arrays(self, chroms, starts, ends):
        """BigWigFile.get_as_array for a mixed-chromosome batch in ONE call: (values float32[total], offsets int64[n + 1]) as
        `arrays`.  `chroms` as in `summarize`; an unknown chromosome gives a NaN row (the reference answers None), start >= end an
        empty one.  Always from full data: zoom levels hold no per-base values."""
        return arrays(self.spans.values(), self._track_of(chroms), starts, ends)

    def matrix(self, chroms, win_starts, width):
        """The site x base matrix float32 [n, width] of the windows chroms[i]:win_starts[i]-(win_starts[i] + width) in ONE call, as
        `matrix`; an unknown chromosome gives a NaN row."""
        return matrix(self.spans.values(), self._track_of(chroms), win_starts, width)


class BedSet(_FileSet):
    """A whole bigBed file on the device, the counterpart of TrackSet: every chromosome's records (BedTrack) and its part of every
    zoom level.  `summarize` answers a batch as the reference's BigBedFile.summarize would, row by row: from the level its rule picks
    (`summarize_zoom`) or from the records (`summarize_beds`), one call of each kind."""

    _summarize_full = staticmethod(summarize_beds)

    def __init__(self, items, levels):
        """items: bigbed.read_items_file's result; levels: bigbed.read_zoom_file's"""
        self.chroms = list(items)
        self.beds = self.full = {chrom: BedTrack(items[chrom][0], items[chrom][1]) for chrom in self.chroms}
        self._set_levels(levels)

    @classmethod
    def from_bigbed(cls, path=None, data=None):
        return cls(bigbed.read_items_file(path, data=data), bigbed.read_zoom_file(path, data=data))
