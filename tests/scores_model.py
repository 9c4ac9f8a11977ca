"""
A NumPy restatement of what the reference's scripts/aggregate_scores_in_intervals.py computes (:107-134, over
lib/bx/binned_array.py:72-100 and lib/bx/wiggle.py:16-85) -- the model the device path is compared with, itself pinned to the
reference's recorded output by tests/test_scores_model_golden.py.

  * scores are float32, NaN where nothing was stored, filled span by span in file order (later lines overwrite);
  * a base counts when its score is truthy (not +-0), not masked and not NaN;
  * total is a float32 accumulator fed in position order: numpy.cumsum(dtype=float32) adds sequentially, as `total += score`
    on numpy.float32 does; avg = total / count in float32;
  * min / max start as the ints 100000000 / -100000000 and give way to a score only through min(score, m) / max(score, m).
"""
import gzip

import numpy as np

MAX = 512 * 1024 * 1024


def open_text(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def wiggle_rows(lines):
    """(chrom, start, end, float value) per data line, the tuples of lib/bx/wiggle.py:31-69 without the strand"""
    chrom = pos = step = None
    span, mode = 1, "bed"
    for line in lines:
        if line.isspace() or line.startswith("track") or line.startswith("#") or line.startswith("browser"):
            continue
        if line.startswith("variableStep") or line.startswith("fixedStep"):
            header = dict(f.split("=") for f in line.split()[1:])
            chrom = header["chrom"]
            span = int(header.get("span", 1))
            mode = line.split()[0]
            if mode == "fixedStep":
                pos, step = int(header["start"]) - 1, int(header["step"])
        elif mode == "bed":
            f = line.split()
            if len(f) > 3:
                yield f[0], int(f[1]), int(f[2]), float(f[3])
        elif mode == "variableStep":
            f = line.split()
            yield chrom, int(f[0]) - 1, int(f[0]) - 1 + span, float(f[1])
        else:
            yield chrom, pos, pos + span, float(line.split()[0])
            pos += step


def fill(size, starts, ends, values):
    """float32[size], NaN, then track[s:e] = v in order (clipped to the track)"""
    track = np.full(size, np.nan, dtype=np.float32)
    for s, e, v in zip(starts, ends, values):
        s, e = max(int(s), 0), min(int(e), size)
        if s < e:
            track[s:e] = np.float32(v)
    return track


def load_wiggle(lines):
    """{chrom: float32 track sized to its largest span end}"""
    rows = {}
    for chrom, s, e, v in wiggle_rows(lines):
        rows.setdefault(chrom, []).append((s, e, v))
    return {c: fill(max([e for _, e, _ in r] + [0]), [s for s, _, _ in r], [e for _, e, _ in r], [v for _, _, v in r]) for c, r in rows.items()}


def load_mask(lines):
    """{chrom: bool array sized to its largest end} of a BED mask (bitset_builders.py:33-46)"""
    rows = {}
    for line in lines:
        if line.startswith("#") or line.isspace():
            continue
        f = line.split()
        rows.setdefault(f[0], []).append((int(f[1]), int(f[2])))
    out = {}
    for c, r in rows.items():
        m = out[c] = np.zeros(max(e for _, e in r), dtype=bool)
        for s, e in r:
            m[s:e] = True
    return out


def valid_scores(track, s, e, mask=None):
    """the scores of [s, e) that count, in position order"""
    s, e = max(int(s), 0), min(int(e), len(track))
    if s >= e:
        return np.zeros(0, dtype=np.float32)
    v = track[s:e]
    ok = ~np.isnan(v) & (v != 0)
    if mask is not None:
        m = np.zeros(e - s, dtype=bool)
        hi = min(e, len(mask))
        if s < hi:
            m[:hi - s] = mask[s:hi]
        ok &= ~m
    return v[ok]


def aggregate(track, starts, ends, mask=None):
    """count int32, total / minimum / maximum float32 per interval (+0.0, +inf, -inf where nothing counts)"""
    n = len(starts)
    count, total = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    mn, mx = np.full(n, np.inf, dtype=np.float32), np.full(n, -np.inf, dtype=np.float32)
    for i, (s, e) in enumerate(zip(starts, ends)):
        v = valid_scores(track, s, e, mask)
        if len(v):
            count[i], total[i], mn[i], mx[i] = len(v), np.cumsum(v, dtype=np.float32)[-1], v.min(), v.max()
    return count, total, mn, mx


def format_row(chrom, start, stop, count, total, mn, mx):
    if count > 0:
        avg = np.float32(total) / int(count)
        mn = np.float32(mn) if not 100000000 < np.float32(mn) else 100000000
        mx = np.float32(mx) if not -100000000 > np.float32(mx) else -100000000
    else:
        avg = mn = mx = "nan"
    return "\t".join(map(str, [chrom, start, stop, avg, mn, mx]))


def run(score_lines, interval_lines, mask_lines=None):
    """the script's standard output"""
    tracks = load_wiggle(score_lines)
    masks = load_mask(mask_lines) if mask_lines is not None else None
    out = []
    for line in interval_lines:
        f = line.split()
        chrom, s, e = f[0], int(f[1]), int(f[2])
        if chrom in tracks:
            c, t, a, b = aggregate(tracks[chrom], [s], [e], masks.get(chrom) if masks else None)
            out.append(format_row(chrom, s, e, c[0], t[0], a[0], b[0]))
        else:
            out.append(format_row(chrom, s, e, 0, 0, 0, 0))
    return "".join(x + "\n" for x in out)


def fraction_order_sensitive(track, starts, ends):
    """Of the intervals with something to add: the fraction whose ordered float32 sum differs from BOTH the rounded float64 sum
    and numpy's pairwise float32 sum -- what lets a fixture tell an ordered chain from a reduction tree."""
    differ = seen = 0
    for s, e in zip(starts, ends):
        v = valid_scores(track, s, e)
        if len(v) == 0:
            continue
        seen += 1
        ordered = np.cumsum(v, dtype=np.float32)[-1]
        wide, pairwise = np.float32(np.sum(v, dtype=np.float64)), np.sum(v, dtype=np.float32)
        differ += (ordered.tobytes() != wide.tobytes()) and (ordered.tobytes() != pairwise.tobytes())
    return differ / max(seen, 1)
