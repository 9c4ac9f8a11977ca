"""
Wiggle text -> per-chromosome span arrays, what lib/bx/wiggle.py:16-69 (IntervalReader) yields line by line, collected for
``ScoreTrack.set_spans``: {chrom: (starts, ends, values)} with int64 starts / ends (zero-based, half-open) and float32 values,
in file order per chromosome (later spans overwrite earlier ones, as load_scores_wiggle's per-position assignment does).

Covered: bed-style lines (four fields or more: chrom start end value), ``variableStep`` and ``fixedStep`` with ``span``;
``track`` / ``browser`` / ``#`` / blank lines are skipped.  A value is ``float(text)`` stored as float32 -- two roundings, as
in the reference, where the double goes into a float32 BinnedArray.
"""
import gzip

import numpy as np


def parse_header(line):
    return dict(field.split("=") for field in line.split()[1:])


def read_spans(lines):
    """{chrom: (starts int64, ends int64, values float32)} from an iterable of wiggle lines."""
    per = {}
    chrom = pos = step = None
    span = 1
    mode = "bed"

    def rows_of(name):
        r = per.get(name)
        if r is None:
            r = per[name] = ([], [], [])
        return r

    for line in lines:
        if line.isspace() or line.startswith(("track", "#", "browser")):
            continue
        if line.startswith("variableStep"):
            header = parse_header(line)
            chrom, pos, step = header["chrom"], None, None
            span = int(header["span"]) if "span" in header else 1
            mode = "variableStep"
        elif line.startswith("fixedStep"):
            header = parse_header(line)
            chrom, pos, step = header["chrom"], int(header["start"]) - 1, int(header["step"])
            span = int(header["span"]) if "span" in header else 1
            mode = "fixedStep"
        elif mode == "bed":
            fields = line.split()
            if len(fields) > 3:
                s, e, v = rows_of(fields[0])
                s.append(int(fields[1])), e.append(int(fields[2])), v.append(float(fields[3]))
        elif mode == "variableStep":
            fields = line.split()
            s, e, v = rows_of(chrom)
            at = int(fields[0]) - 1
            s.append(at), e.append(at + span), v.append(float(fields[1]))
        else:
            s, e, v = rows_of(chrom)
            s.append(pos), e.append(pos + span), v.append(float(line.split()[0]))
            pos += step
    return {name: (np.array(s, dtype=np.int64), np.array(e, dtype=np.int64), np.array(v, dtype=np.float64).astype(np.float32))
            for name, (s, e, v) in per.items()}


def read_spans_file(path):
    """read_spans of a file; one named *.gz is read through gzip."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return read_spans(f)
