"""
BigWig file: ``BigWigFile`` of the reference's lib/bx/bbi/bigwig_file.pyx (over bbi_file.pyx), with the summaries computed on the
MI355X (bxmi.summary).

``summarize_from_full`` is the reference's bit for bit.  ``summarize`` and ``query`` are served from full data exactly when the
reference's own rule picks no zoom level (bbi_file.pyx:205-215, 281-294: ``((end - start) // size) // 2`` is at most 1, or no
level's ``reduction_level`` is at most that value); otherwise, BY DEFAULT, they raise NotImplementedError and
``summarize_from_full`` is the call to make.  ``BigWigFile(file, use_zoom=True)`` answers those regions as the reference does, from
the zoom level its rule picks (bbi_file.pyx:296-432; bxmi.summary.ZoomTrack), bit for bit; only a level whose records are not in
order still raises the same NotImplementedError.  The default is kept for compatibility with tests that pin the earlier
behaviour and is meant to flip later.
``get`` and ``get_as_array`` are host code over the file's spans; ``get_as_arrays`` answers a whole list of regions, each as
``get_as_array`` would, in ONE device call (bxmi.summary.arrays).  The file is read once, when the object is made; its items go
to the device on the first summary.  `chrom` may be str or bytes everywhere.
"""
import numpy as np

from bxmi import bigwig


class SummarizedData:
    """The five arrays of one region (bbi_file.pyx:66-79), `size` float64 values each."""

    def __init__(self, start, end, size, planes):
        self.start, self.end, self.size = start, end, size
        self.valid_count, self.min_val, self.max_val, self.sum_data, self.sum_squares = planes


def _bits32(value):
    value = int(value)
    if value < 0:
        raise OverflowError("can't convert negative value to bits32")
    if value > 0xFFFFFFFF:
        raise OverflowError("value too large to convert to bits32")
    return value


class BigWigFile:
    """A "big binary indexed" file whose raw data is in wiggle format.  `file`: a file object opened in binary mode."""

    def __init__(self, file=None, use_zoom=False):
        self._tracks = None
        self._zoom_tracks = {}
        self.use_zoom = bool(use_zoom)
        if file is not None:
            self.open(file)

    def open(self, file):
        try:
            file.seek(0)
        except (AttributeError, OSError):
            pass
        data = file.read()
        self.file = file
        self._sizes = bigwig.chroms(data=data)
        self._spans = bigwig.read_spans_file(data=data)
        self._reductions = bigwig.zoom_reductions(data=data)
        self.zoom_levels = len(self._reductions)
        self._levels = bigwig.read_zoom_file(data=data) if self.use_zoom else None

    def close(self):
        """Free the device copies of the items (they are made again on the next summary)."""
        for t in list((self._tracks or {}).values()) + list(self._zoom_tracks.values()):
            t.close()
        self._tracks = None
        self._zoom_tracks = {}

    @staticmethod
    def _name(chrom):
        return chrom.decode() if isinstance(chrom, (bytes, bytearray)) else chrom

    def _track(self, chrom):
        from bxmi.summary import SpanTrack

        if self._tracks is None:
            self._tracks = {}
        if chrom not in self._tracks:
            self._tracks[chrom] = SpanTrack(*self._spans[chrom])
        return self._tracks[chrom]

    def _picks_zoom(self, start, end, summary_size):
        desired = ((end - start) // summary_size) // 2
        return desired > 1 and any(r <= desired for r in self._reductions)

    def summarize_from_full(self, chrom, start, end, summary_size):
        """`summary_size` data points over `chrom`:`start`-`end`, always from the raw data points.  None for start >= end or an
        unknown chromosome."""
        from bxmi.summary import summarize

        start, end, summary_size = _bits32(start), _bits32(end), int(summary_size)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        if end > 2147483647:
            raise ValueError("regions beyond 2^31 - 1 are not supported")
        res = summarize([self._track(chrom)], [0], [start], [end], summary_size)
        return SummarizedData(start, end, summary_size, [plane[0] for plane in res])

    def summarize(self, chrom, start, end, summary_size):
        """`summary_size` data points over `chrom`:`start`-`end`: from full data where the reference would take them from
        there; where it would take a zoom level, from that level with `use_zoom`, else NotImplementedError."""
        start, end, summary_size = _bits32(start), _bits32(end), int(summary_size)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        if self._picks_zoom(start, end, summary_size):
            if not self.use_zoom:
                raise NotImplementedError("the reference answers this region from a zoom level, which is not implemented: "
                                          "call summarize_from_full for the answer from full data")
            return self._summarize_from_zoom(chrom, start, end, summary_size)
        return self.summarize_from_full(chrom, start, end, summary_size)

    def _summarize_from_zoom(self, chrom, start, end, summary_size):
        from bxmi.summary import NOT_ORDERED, ZoomTrack, pick_level, summarize_zoom

        if end > 2147483647:
            raise ValueError("regions beyond 2^31 - 1 are not supported")
        level = pick_level(self._reductions, start, end, summary_size)
        if (chrom, level) not in self._zoom_tracks:
            arrays = self._levels[level][1][chrom]
            why = bigwig.ordered_level(arrays)
            if why:
                raise NotImplementedError(NOT_ORDERED % why)
            self._zoom_tracks[chrom, level] = ZoomTrack(arrays)
        res = summarize_zoom([self._zoom_tracks[chrom, level]], [0], [start], [end], summary_size)
        return SummarizedData(start, end, summary_size, [plane[0] for plane in res])

    def query(self, chrom, start, end, summary_size):
        """A list of `summary_size` dicts with the keys mean, max, min, coverage, std_dev (bbi_file.pyx:231-260)."""
        from bxmi.summary import Summary, stats

        if end > 2147483647 or start < 0:
            raise ValueError
        results = self.summarize(chrom, start, end, summary_size)
        if not results:
            return None
        planes = Summary(*[np.asarray(p)[None, :] for p in (results.valid_count, results.min_val, results.max_val, results.sum_data,
                                                              results.sum_squares)])
        mean, coverage, std_dev = (a[0] for a in stats(planes, [results.start], [results.end], summary_size))
        return [{"mean": mean[i], "max": results.max_val[i], "min": results.min_val[i], "coverage": coverage[i], "std_dev": std_dev[i]}
                for i in range(summary_size)]

    def _clipped(self, chrom, start, end):
        """the items of bigwig_file.pyx:63-88: clipped to [start, end), empty ones dropped, in file order"""
        s, e, v = self._spans[chrom]
        keep = np.nonzero((e > start) & (s < end))[0]
        cs, ce = np.maximum(s[keep].astype(np.int64), start), np.minimum(e[keep].astype(np.int64), end)
        ok = cs < ce
        return cs[ok], ce[ok], v[keep][ok]

    def get(self, chrom, start, end):
        """All data points over `chrom`:`start`-`end` as a list of (start, end, value)."""
        start, end = _bits32(start), _bits32(end)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        cs, ce, v = self._clipped(chrom, start, end)
        return [(int(a), int(b), float(x)) for a, b, x in zip(cs, ce, v)]

    def get_as_array(self, chrom, start, end):
        """The data points over `chrom`:`start`-`end` as a float32 array, NaN where there is none; a later item overwrites."""
        start, end = _bits32(start), _bits32(end)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        out = np.full(end - start, np.nan, dtype=np.float32)
        for a, b, x in zip(*self._clipped(chrom, start, end)):
            out[a - start:b - start] = x
        return out

    def get_as_arrays(self, chroms, starts, ends):
        """`get_as_array` for every region `chroms[i]`:`starts[i]`-`ends[i]` in ONE device call: a list with one float32 array per
        region, None where `get_as_array` answers None (start >= end, an unknown chromosome)."""
        from bxmi.summary import arrays

        names = [self._name(c) for c in chroms]
        starts, ends = [_bits32(s) for s in starts], [_bits32(e) for e in ends]
        if not len(names) == len(starts) == len(ends):
            raise ValueError("chroms, starts and ends must have one length")
        answered = [s < e and c in self._sizes for c, s, e in zip(names, starts, ends)]
        if any(e > 2147483647 for e, ok in zip(ends, answered) if ok):
            raise ValueError("regions beyond 2^31 - 1 are not supported")
        order = sorted({c for c, ok in zip(names, answered) if ok})
        track_of = [order.index(c) if ok else -1 for c, ok in zip(names, answered)]
        # (a region that is not answered travels as an empty row)
        values, offsets = arrays([self._track(c) for c in order], track_of, [s if ok else 0 for s, ok in zip(starts, answered)],
                                 [e if ok else 0 for e, ok in zip(ends, answered)])
        # (a copy per region, as get_as_array returns: no row keeps the batch alive or shares its memory)
        return [values[offsets[i]:offsets[i + 1]].copy() if ok else None for i, ok in enumerate(answered)]
