"""
Reader of UCSC ``.chain`` / ``.chain.gz`` alignments into the SoA tables of ``bxmi_chainmap_create``.

What the reference does on loading (scripts/bnMapper.py:293-308, lib/bx/align/_epo.pyx:96-122,168-184,
lib/bx/align/epo.py:19-43), restated over arrays: a chain is a header line

    chain score tName tSize tStrand tStart tEnd qName qSize qStrand qStart qEnd id

followed by lines ``size dt dq``, a last line ``size`` and a blank line.  The block tables are cumulative and relative
to the chain's start (T[0] = (0, size0), T[j+1].start = T[j].end + dt[j]; Q likewise with dq); a '-' strand side is
turned into forward coordinates in the header (start, end = size - end, size - start), after which the target strand
must be '+'.  Chains are kept per tName in file order; a chain whose id was seen before REPLACES the earlier one in the
earlier one's place (bnMapper.py:412 keys a dict by id).

This module neither reads nor writes pickle files (the reference drops a ``.pkl`` next to its input and prefers it on
the next run).
"""
import gzip

import numpy as np


class ChainTable:
    """The chains of one source chromosome (tName), in file order, as arrays."""

    __slots__ = ("t_name", "t_start", "t_end", "q_name", "q_start", "q_span", "q_minus", "ids", "block_off", "blk_t_start",
                 "blk_t_end", "blk_q_start")

    def __len__(self):
        return len(self.t_start)

    def block_table(self, c):
        """(T, Q) of chain c as int64 [n, 2] arrays, the CT / CQ of bnMapper.py:88."""
        a, b = int(self.block_off[c]), int(self.block_off[c + 1])
        ts, te, qs = (x[a:b].astype(np.int64) for x in (self.blk_t_start, self.blk_t_end, self.blk_q_start))
        return np.stack([ts, te], 1), np.stack([qs, qs + te - ts], 1)


def _open(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def _to_i32(values, what):
    a = np.asarray(values, dtype=np.int64)
    if a.size and (a.min() < -(1 << 31) or a.max() > (1 << 31) - 1):
        raise ValueError("%s does not fit 32 bits" % what)
    return a.astype(np.int32)


def parse_chains(lines):
    """[(header fields as a tuple, sizes, dt, dq)] of an iterable of lines, in file order."""
    out, head, body = [], None, []

    def close():
        if head is None:
            return
        tok = np.array(" ".join(body).split(), dtype=np.int64)
        if len(tok) % 3 != 1:
            raise ValueError("chain %s: the block lines do not end in a single size" % head[-1])
        n = len(tok) // 3
        trip = tok[: 3 * n].reshape(n, 3)
        out.append((head, np.append(trip[:, 0], tok[-1]), trip[:, 1].copy(), trip[:, 2].copy()))

    for line in lines:
        if line.startswith("chain"):
            close()
            f = line.split()
            if len(f) != 13:
                raise ValueError("not a chain header: %r" % line)
            head = (int(f[1]), f[2], int(f[3]), f[4], int(f[5]), int(f[6]), f[7], int(f[8]), f[9], int(f[10]), int(f[11]), f[12])
            body = []
        elif head is not None and line.strip():
            body.append(line)
    close()
    return out


def load_chains(path):
    """{tName: ChainTable} of a .chain or .chain.gz file, source chromosomes in order of first appearance."""
    with _open(path) as fd:
        parsed = parse_chains(fd)
    by_id = {}
    for rec in parsed:  # a repeated id replaces the earlier chain where that one stood (bnMapper.py:412)
        by_id[rec[0][11]] = rec
    groups = {}
    for rec in by_id.values():
        groups.setdefault(rec[0][1], []).append(rec)
    tables = {}
    for t_name, recs in groups.items():
        t = ChainTable()
        t.t_name = t_name
        t_start, t_end, q_start, q_span, q_minus, off = [], [], [], [], [], [0]
        bts, bte, bqs = [], [], []
        for head, size, dt, dq in recs:
            _score, _tn, t_size, t_strand, ts, te, _qn, q_size, q_strand, qs, qe, cid = head
            if t_strand == "-":  # bnMapper.py:301-304
                ts, te = t_size - te, t_size - ts
            if q_strand == "-":
                qs, qe = q_size - qe, q_size - qs
            if t_strand not in "+-" or q_strand not in "+-":
                raise ValueError("chain %s: strand must be + or -" % cid)
            if t_strand != "+":
                raise ValueError("chain %s: all target strands should be +" % cid)  # bnMapper.py:307
            if (size < 0).any() or (dt < 0).any() or (dq < 0).any():  # (empty blocks are legal: chains made from EPO alignments have them)
                raise ValueError("chain %s: a block or a gap of negative length" % cid)
            # cumulative intervals (epo.py cummulative_intervals, _epo.pyx:168-184)
            cs = np.cumsum(size)
            starts_t = np.concatenate([[0], cs[:-1] + np.cumsum(dt)])
            starts_q = np.concatenate([[0], cs[:-1] + np.cumsum(dq)])
            bts.append(starts_t)
            bte.append(starts_t + size)
            bqs.append(starts_q)
            t_start.append(ts), t_end.append(te), q_start.append(qs), q_span.append(qe - qs), q_minus.append(q_strand == "-")
            off.append(off[-1] + len(size))
        t.t_start, t.t_end = _to_i32(t_start, "tStart"), _to_i32(t_end, "tEnd")
        t.q_start, t.q_span = _to_i32(q_start, "qStart"), _to_i32(q_span, "qEnd - qStart")
        t.q_minus = np.array(q_minus, dtype=np.uint8)
        t.q_name = [r[0][6] for r in recs]
        t.ids = [r[0][11] for r in recs]
        t.block_off = np.array(off, dtype=np.int64)
        t.blk_t_start = _to_i32(np.concatenate(bts), "a block's target start")
        t.blk_t_end = _to_i32(np.concatenate(bte), "a block's target end")
        t.blk_q_start = _to_i32(np.concatenate(bqs), "a block's query start")
        tables[t_name] = t
    return tables
