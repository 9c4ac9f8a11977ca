"""
BigBed file: ``BigBedFile`` of the reference's lib/bx/bbi/bigbed_file.pyx (over bbi_file.pyx), with the summaries computed on the
MI355X (bxmi.summary).

``summarize_from_full`` is the reference's bit for bit: the coverage of every bin by the file's records, each weighted as a
bigWig item of value 1 (bxmi.summary.BedTrack).  ``summarize`` and ``query`` answer as the reference does: from the zoom level its
rule picks (bbi_file.pyx:205-215, 281-294; bxmi.summary.ZoomTrack), from the records where it picks none.  Only a level whose
records are not in order raises NotImplementedError.  ``get`` is host code over the file's records.  The file is read once, when
the object is made; its records go to the device on the first summary.  `chrom` may be str or bytes everywhere (the reference
takes bytes in ``summarize_from_full`` and ``get``, str in ``summarize`` and ``query``).
"""
import numpy as np

from bx.bbi.bigwig_file import SummarizedData, _bits32
from bx.intervals.io import GenomicInterval
from bxmi import bigbed, bigwig


class BigBedFile:
    """A "big binary indexed" file whose raw data is in BED format.  `file`: a file object opened in binary mode."""

    def __init__(self, file=None):
        self._tracks = {}
        self._zoom_tracks = {}
        if file is not None:
            self.open(file)

    def open(self, file):
        try:
            file.seek(0)
        except (AttributeError, OSError):
            pass
        data = file.read()
        self.file = file
        self._sizes = bigbed.chroms(data=data)
        self._items = bigbed.read_items_file(data=data)
        self._levels = bigbed.read_zoom_file(data=data)
        self._reductions = [r for r, _ in self._levels]
        self.zoom_levels = len(self._reductions)

    def close(self):
        """Free the device copies of the records (they are made again on the next summary)."""
        for t in list(self._tracks.values()) + list(self._zoom_tracks.values()):
            t.close()
        self._tracks = {}
        self._zoom_tracks = {}

    @staticmethod
    def _name(chrom):
        return chrom.decode() if isinstance(chrom, (bytes, bytearray)) else chrom

    def _track(self, chrom):
        from bxmi.summary import BedTrack

        if chrom not in self._tracks:
            s, e, _ = self._items[chrom]
            self._tracks[chrom] = BedTrack(s, e)
        return self._tracks[chrom]

    def summarize_from_full(self, chrom, start, end, summary_size):
        """`summary_size` data points over `chrom`:`start`-`end`, always from the file's records.  None for start >= end or an
        unknown chromosome."""
        from bxmi.summary import summarize_beds

        start, end, summary_size = _bits32(start), _bits32(end), int(summary_size)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        if end > 2147483647:
            raise ValueError("regions beyond 2^31 - 1 are not supported")
        res = summarize_beds([self._track(chrom)], [0], [start], [end], summary_size)
        return SummarizedData(start, end, summary_size, [plane[0] for plane in res])

    def summarize(self, chrom, start, end, summary_size):
        """`summary_size` data points over `chrom`:`start`-`end`, from the zoom level the reference's rule picks, or from the
        records where it picks none."""
        from bxmi.summary import NOT_ORDERED, ZoomTrack, pick_level, summarize_zoom

        start, end, summary_size = _bits32(start), _bits32(end), int(summary_size)
        chrom = self._name(chrom)
        if start >= end or chrom not in self._sizes:
            return None
        level = pick_level(self._reductions, start, end, summary_size) if summary_size >= 1 else None
        if level is None:
            return self.summarize_from_full(chrom, start, end, summary_size)
        if end > 2147483647:
            raise ValueError("regions beyond 2^31 - 1 are not supported")
        if (chrom, level) not in self._zoom_tracks:
            arrays = self._levels[level][1][chrom]
            why = bigwig.ordered_level(arrays)
            if why:
                raise NotImplementedError(NOT_ORDERED % why)
            self._zoom_tracks[chrom, level] = ZoomTrack(arrays)
        res = summarize_zoom([self._zoom_tracks[chrom, level]], [0], [start], [end], summary_size)
        return SummarizedData(start, end, summary_size, [plane[0] for plane in res])

    def query(self, chrom, start, end, summary_size):
        """A list of `summary_size` dicts with the keys mean, max, min, coverage, std_dev (bbi_file.pyx:231-260); std_dev is a
        Python float, as the reference's."""
        from bxmi.summary import Summary, stats

        if end > 2147483647 or start < 0:
            raise ValueError
        results = self.summarize(chrom, start, end, summary_size)
        if not results:
            return None
        planes = Summary(*[np.asarray(p)[None, :] for p in (results.valid_count, results.min_val, results.max_val, results.sum_data,
                                                              results.sum_squares)])
        mean, coverage, std_dev = (a[0] for a in stats(planes, [results.start], [results.end], summary_size))
        return [{"mean": mean[i], "max": results.max_val[i], "min": results.min_val[i], "coverage": coverage[i], "std_dev": float(std_dev[i])}
                for i in range(summary_size)]

    def get(self, chrom, start, end):
        """All records over `chrom`:`start`-`end` (start < `end` and end > `start`; not clipped), in file order, as
        GenomicInterval(chrom, start, end, the record's other columns...).  As in the reference, a bytes `chrom` stays bytes in
        `.chrom` and shows as its repr in the fields."""
        start, end = _bits32(start), _bits32(end)
        name = self._name(chrom)
        if start >= end or name not in self._sizes:
            return None
        s, e, rest = self._items[name]
        out = []
        for i in np.nonzero((s.astype(np.int64) < end) & (e.astype(np.int64) > start))[0]:
            row = GenomicInterval(None, [chrom, str(int(s[i])), str(int(e[i]))] + rest[i].split("\t"), 0, 1, 2, 5, "+")
            row.fields[0] = str(chrom)  # (the reference's __setattr__ writes str(value) back into the field)
            out.append(row)
        return out
