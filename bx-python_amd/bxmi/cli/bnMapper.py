#!/usr/bin/env python
"""
Lift features (BED or narrowPeak rows) from the target assembly of a .chain alignment onto its query assembly,
a whole source chromosome per device call.

usage: %prog [-f BED4|BED12|narrowPeak] [-i BED|narrowPeak] [-g N] [-t X] [-k] [-o OUT] [-v LEVEL] input [input ...] alignment
"""
# The command-line counterpart of the reference's scripts/bnMapper.py: same option letters, choices, defaults and output
# formats (:146-148,198-269); the mapping itself is ChainMap.map, once per source chromosome.  On purpose: source
# chromosomes come out in order of first appearance (the reference iterates a set, :288), no .pkl is read or written next
# to the alignment, there is no -s/--screen, and nothing is logged per feature.
import argparse
import logging
import os
import sys

import numpy as np

from bxmi import liftover

VERBOSITY = {"silent": logging.ERROR, "info": logging.INFO, "debug": logging.DEBUG}
log = logging.getLogger("bxmi.bnMapper")

# the three record layouts, byte for byte what the reference writes
BED4_FRM = "%s\t%d\t%d\t%s\n"
BED12_FRM = "%s\t%d\t%d\t%s\t1000\t+\t%d\t%d\t0,0,0\t%d\t%s\t%s\n"
NPEAK_FRM = "%s\t%d\t%d\t%s\t%d\t%s\t%f\t%f\t%f\t%d\n"


def read_features(path, narrow_peak):
    """Rows of a BED (first four columns) or narrowPeak file, grouped by chromosome in order of first appearance:
    {chrom: [row, ...]}, row = [start, end, name] + [score, strand, signal, p, q, absolute summit] for narrowPeak.
    Field widths follow the reference's record types (chrom 30, name 100, strand 1 characters; bnMapper.py:30-44)."""
    groups = {}
    with open(path) as fd:
        for line in fd:
            c = line.split()
            row = [int(c[1]), int(c[2]), c[3][:100]]
            if narrow_peak:
                row += [int(c[4]), c[5][:1], float(c[6]), float(c[7]), float(c[8]), int(c[1]) + int(c[-1])]
            groups.setdefault(c[0][:30], []).append(row)
    return groups


def write_bed4(out, dest, name, starts, ends, row, summit):
    for x, y in zip(starts, ends):
        out.write(BED4_FRM % (dest, x, y, name))


def write_bed12(out, dest, name, starts, ends, row, summit):
    lo, hi = int(starts[0]), int(ends[-1])
    sizes = ",".join(str(int(y - x)) for x, y in zip(starts, ends))
    offsets = ",".join(str(int(x) - lo) for x in starts)
    out.write(BED12_FRM % (dest, lo, hi, name, lo, hi, len(starts), sizes, offsets))


def write_narrow_peak(out, dest, name, starts, ends, row, summit):
    lo, hi = int(starts[0]), int(ends[-1])
    # the summit column is relative to the start; the lifted summit where it falls inside the record, else the midpoint (:218,241)
    rel = summit - lo if summit is not None and lo <= summit <= hi else int((lo + hi) / 2) - lo
    out.write(NPEAK_FRM % (dest, lo, hi, name, row[3], row[4], row[5], row[6], row[7], rel))


WRITERS = {"BED4": write_bed4, "BED12": write_bed12, "narrowPeak": write_narrow_peak}


def lift_file(path, out, cmap, opt):
    """Map one input file and write its records to `out`."""
    narrow = opt.in_format == "narrowPeak"
    write = WRITERS[opt.format]
    for chrom, rows in read_features(path, narrow).items():
        starts = np.array([r[0] for r in rows], dtype=np.int64)
        ends = np.array([r[1] for r in rows], dtype=np.int64)
        res = cmap.map(chrom, starts, ends, gap=opt.gap, threshold=opt.threshold, keep_split=opt.keep_split)
        summits = None
        if narrow and opt.format == "narrowPeak":
            # each summit as the empty feature [p, p): first chain that yields something, its first slice's start (:222-242)
            at = np.array([r[8] for r in rows], dtype=np.int64)
            summits = cmap.map(chrom, at, at, gap=opt.gap, select=liftover.FIRST)
        dest = cmap.q_names(chrom, res.chain)
        done = 0
        for i, row in enumerate(rows):
            if res.status[i] != liftover.MAPPED:
                continue
            a, b = int(res.offsets[i]), int(res.offsets[i + 1])
            summit = None
            if summits is not None and summits.status[i] == liftover.MAPPED:
                summit = int(summits.out_start[summits.offsets[i]])
            write(out, dest[i], row[2], res.out_start[a:b], res.out_end[a:b], row, summit)
            done += 1
        log.info("%s, %s: %d features in, %d lifted", os.path.basename(path), chrom, len(rows), done)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("input", nargs="+", help="feature file(s); with more than one, -o names an existing directory that receives one output per input")
    p.add_argument("alignment", help="the alignment, .chain or .chain.gz")
    p.add_argument("-f", "--format", choices=("BED4", "BED12", "narrowPeak"), default="BED4",
                   help="BED4: one record per lifted block; BED12: one record per feature, its blocks in the block columns; "
                        "narrowPeak: one record per feature, the other columns of the input carried over (default %(default)s)")
    p.add_argument("-o", "--output", metavar="FILE", default="stdout", help="where to write; 'stdout' or '-' for standard output (default)")
    p.add_argument("-t", "--threshold", metavar="FLOAT", type=float, default=0.0,
                   help="drop a feature when fewer than this fraction of its bases is lifted (default %(default)s)")
    p.add_argument("-g", "--gap", type=int, default=-1, help="drop a feature that spans an alignment gap longer than this; -1 = no limit (default)")
    p.add_argument("-v", "--verbose", choices=list(VERBOSITY), default="info", help="how much to report on standard error (default %(default)s)")
    p.add_argument("-k", "--keep_split", action="store_true", default=False,
                   help="a feature that lifts through several chains is given to the chain with the longest result; without -k it is dropped")
    p.add_argument("-i", "--in_format", choices=["BED", "narrowPeak"], default="BED", help="format of the input (default %(default)s)")
    return p


def main(argv=None, out=None):
    parser = build_parser()
    opt = parser.parse_args(argv)
    logging.basicConfig()
    log.setLevel(VERBOSITY[opt.verbose])
    if opt.format == "narrowPeak" and opt.in_format != "narrowPeak":
        parser.error("-f narrowPeak carries the columns of narrowPeak input over: it needs -i narrowPeak")
    many = len(opt.input) > 1
    if many and not os.path.isdir(opt.output):
        parser.error("several inputs: -o must name an existing directory")
    cmap = liftover.ChainMap.from_file(opt.alignment)
    log.info("%s: %d chains on %d source chromosomes", opt.alignment, sum(len(t) for t in cmap.tables.values()), len(cmap.tables))
    try:
        if many:
            for path in opt.input:
                if os.path.isfile(path):
                    with open(os.path.join(opt.output, os.path.basename(path)), "w") as fd:
                        lift_file(path, fd, cmap, opt)
                else:
                    log.warning("%s is not a file: left out", path)
        elif out is not None or opt.output in ("stdout", "-"):
            fd = out if out is not None else sys.stdout
            lift_file(opt.input[0], fd, cmap, opt)
            fd.flush()
        else:
            with open(opt.output, "w") as fd:
                lift_file(opt.input[0], fd, cmap, opt)
    finally:
        cmap.close()


if __name__ == "__main__":
    main()
