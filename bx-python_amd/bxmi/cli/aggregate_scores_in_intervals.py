#!/usr/bin/env python
"""
Given a list of intervals in BED format (`interval_file`) and a set of scores in wiggle format (`score_file`), print each
interval plus the average, minimum and maximum of the scores that fall in that interval, one device call per chromosome.

usage: %prog score_file interval_file [out_file] [-m MASK]
"""
# The command-line counterpart of the reference's scripts/aggregate_scores_in_intervals.py: same arguments, same lines
# (:107-134).  On purpose: -b / --binned (a directory of .ba files) is not supported, and an interval that reaches outside
# [0, 512 Mi) on a chromosome that has scores raises IndexError where the reference raises for most such rows.
import argparse
import sys

import numpy as np

from bxmi import _ffi, scores, wiggle

MAX = 512 * 1024 * 1024  # BinnedArray's default max_size (lib/bx/binned_array.py) and the size of a default bitset


def load_tracks(path):
    """{chrom: ScoreTrack} of a wiggle file, each sized to its largest span end."""
    tracks = {}
    for chrom, (s, e, v) in wiggle.read_spans_file(path).items():
        keep = e > s
        s, e, v = s[keep], e[keep], v[keep]
        if len(s) and (s.min() < 0 or e.max() > MAX):
            raise IndexError("%s: a score position outside [0, %d)" % (chrom, MAX))
        t = tracks[chrom] = scores.ScoreTrack(int(e.max()) if len(e) else 0)
        t.set_spans(s, e, v)
    return tracks


def aggregate_file(interval_path, out, tracks, masks):
    rows = []
    with open(interval_path) as f:
        for line in f:
            fields = line.split()
            rows.append((fields[0], int(fields[1]), int(fields[2])))
    by_chrom = {}
    for i, (chrom, _, _) in enumerate(rows):
        by_chrom.setdefault(chrom, []).append(i)
    lines = [None] * len(rows)
    for chrom, idx in by_chrom.items():
        track = tracks.get(chrom)
        if track is None:
            for i in idx:
                lines[i] = scores.format_row(rows[i][0], rows[i][1], rows[i][2], 0, 0.0, 0.0, 0.0)
            continue
        s = np.array([rows[i][1] for i in idx], dtype=np.int64)
        e = np.array([rows[i][2] for i in idx], dtype=np.int64)
        bad = (s < e) & ((s < 0) | (e > MAX))
        if bad.any():
            k = idx[int(np.argmax(bad))]
            raise IndexError("%s\t%d\t%d reaches outside [0, %d)" % (rows[k] + (MAX,)))
        s, e = np.where(s < e, s, 0), np.where(s < e, e, 0)  # (an empty row has no bases whatever its coordinates)
        res = track.aggregate(s, e, mask=masks.get(chrom) if masks else None)
        for j, i in enumerate(idx):
            lines[i] = scores.format_row(rows[i][0], rows[i][1], rows[i][2], int(res.count[j]), res.total[j], res.minimum[j], res.maximum[j])
    for line in lines:
        out.write(line + "\n")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("score_file", help="wiggle file (bed-style, variableStep or fixedStep lines; .gz is read through gzip)")
    p.add_argument("interval_file", help="BED file: chromosome, start, end in the first three columns")
    p.add_argument("out_file", nargs="?", help="where to write (default: standard output)")
    p.add_argument("-b", "--binned", action="store_true", help="not supported: score_file as a directory of binned array files")
    p.add_argument("-m", "--mask", metavar="FILE", help="bed file containing regions not to consider valid")
    return p


def main(argv=None, out=None):
    parser = build_parser()
    opt = parser.parse_args(argv)
    if opt.binned:
        parser.exit(2, "aggregate_scores_in_intervals: -b / --binned (a directory of .ba files) is not supported; give a wiggle file\n")
    tracks = load_tracks(opt.score_file)
    masks = None
    if opt.mask:
        from bxmi.builders import binned_bitsets_from_file

        with open(opt.mask) as f:
            masks = binned_bitsets_from_file(f)
    try:
        if out is not None or not opt.out_file:
            fd = out if out is not None else sys.stdout
            aggregate_file(opt.interval_file, fd, tracks, masks)
            fd.flush()
        else:
            with open(opt.out_file, "w") as fd:
                aggregate_file(opt.interval_file, fd, tracks, masks)
    finally:
        _ffi.close_all(tracks.values())


if __name__ == "__main__":
    main()
