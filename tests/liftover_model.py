"""
A plain, per-row restatement of what the reference's scripts/bnMapper.py computes (a test helper like bitset_replay.py;
the product does not import it).  Line numbers are the reference's.

load_chains           bnMapper.py:293-308,412-420; lib/bx/align/_epo.pyx:96-122,168-184; lib/bx/align/epo.py:19-43
find                  IntervalTree.find over the chain spans, in its result order (in-order: by start, then insertion)
transform             bnMapper.py:83-123 (np.where scans over the whole block table, as there)
union                 bnMapper.py:126-142 with elem_u = bed_union, _epo.pyx:128-164 (starts and ends sorted independently)
map_feature           bnMapper.py:153-193
bed4 / bed12 / npeak  bnMapper.py:146-148,196-269
"""
import gzip

MAPPED, NOCHAIN, SPLIT, BELOW, EMPTY = 0, 1, 2, 3, 4
UNIQUE, LONGEST, FIRST = 0, 1, 2


def read_lines(path):
    """the lines of a text file, gzipped or not"""
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rt") as fd:
        return fd.readlines()


def load_chains(path):
    """{tName: [chain, ...]} in file order; chain = dict(tS, tE, qName, qS, Sz, minus, T, Q, id) in forward coordinates."""
    lines = [line.rstrip("\n") for line in read_lines(path)] + [""]
    by_id = {}
    i = 0
    while i < len(lines):
        if not lines[i].startswith("chain"):
            i += 1
            continue
        h = lines[i].split()
        i += 1
        t_name, t_size, t_strand, ts, te = h[2], int(h[3]), h[4], int(h[5]), int(h[6])
        q_name, q_size, q_strand, qs, qe = h[7], int(h[8]), h[9], int(h[10]), int(h[11])
        sizes, dts, dqs = [], [], []
        while True:
            f = lines[i].split()
            i += 1
            sizes.append(int(f[0]))
            if len(f) == 1:
                break
            dts.append(int(f[1]))
            dqs.append(int(f[2]))
        if t_strand == "-":
            ts, te = t_size - te, t_size - ts
        if q_strand == "-":
            qs, qe = q_size - qe, q_size - qs
        assert t_strand == "+", "all target strands should be +"
        T, Q, t, q = [], [], 0, 0
        for j, s in enumerate(sizes):
            T.append((t, t + s))
            Q.append((q, q + s))
            if j < len(dts):
                t += s + dts[j]
                q += s + dqs[j]
        by_id[h[12]] = dict(tName=t_name, tS=ts, tE=te, qName=q_name, qS=qs, Sz=qe - qs, minus=q_strand == "-", T=T, Q=Q, id=h[12])
    chains = {}
    for c in by_id.values():
        chains.setdefault(c["tName"], []).append(c)
    return chains


def find(chains, fs, fe):
    hit = [k for k, c in enumerate(chains) if c["tE"] > fs and c["tS"] < fe]
    return sorted(hit, key=lambda k: (chains[k]["tS"], k))


def transform(c, fs, fe, gap):
    a, b = max(fs, c["tS"]) - c["tS"], min(fe, c["tE"]) - c["tS"]
    T, Q = c["T"], c["Q"]
    si = [j for j in range(len(T)) if T[j][1] > a][0]
    ei = [j for j in range(len(T)) if T[j][0] < b][-1]
    if si > ei:
        return []
    if gap >= 0 and si < ei - 1:
        if max(T[j + 1][0] - T[j][1] for j in range(si, ei - 1)) > gap or max(Q[j + 1][0] - Q[j][1] for j in range(si, ei - 1)) > gap:
            return []
    to_start = Q[si][0] + max(0, a - T[si][0])
    to_end = Q[ei][1] - max(0, T[ei][1] - b)
    if si == ei:
        slices = [(to_start, to_end)]
    else:
        slices = [(to_start, Q[si][1])] + [Q[j] for j in range(si + 1, ei)] + [(Q[ei][0], to_end)]
    if c["minus"]:
        slices = [(c["Sz"] - y, c["Sz"] - x) for x, y in slices]
    return [(c["qS"] + x, c["qS"] + y) for x, y in slices]


def union(slices):
    if len(slices) < 2:
        return list(slices)
    starts, ends = sorted(x for x, _ in slices), sorted(y for _, y in slices)
    out, cs, ce = [], starts[0], ends[0]
    for x, y in zip(starts[1:], ends[1:]):
        if x <= ce:
            ce = max(ce, y)
        else:
            out.append((cs, ce))
            cs, ce = x, y
    out.append((cs, ce))
    return [(x, y) for x, y in out if x < y]


def map_feature(chains, fs, fe, gap=-1, threshold=0.0, select=UNIQUE, hits=None):
    """(status, chain index or -1, rows) of one feature over the chains of its chromosome (hits: find(chains, fs, fe) where the
    caller has it already)."""
    yielded = [(k, t) for k, t in ((k, transform(chains[k], fs, fe, gap)) for k in (find(chains, fs, fe) if hits is None else hits)) if t]
    if not yielded:
        return NOCHAIN, -1, []
    pick = 0
    if len(yielded) > 1:
        if select == UNIQUE:
            return SPLIT, -1, []
        if select == LONGEST:
            best = 0
            for i, (_, t) in enumerate(yielded):
                m = t[-1][1] - t[0][1]
                if m > best:
                    best, pick = m, i
    k, slices = yielded[pick]
    if (fe - fs) * threshold > sum(y - x for x, y in slices):
        return BELOW, -1, []
    rows = sorted(union(slices))
    if not rows:
        return EMPTY, -1, []
    return MAPPED, k, rows


def bed4(q_name, rows, name):
    return ["%s\t%d\t%d\t%s\n" % (q_name, x, y, name) for x, y in rows]


def bed12(q_name, rows, name):
    start, end = rows[0][0], rows[-1][1]
    return ["%s\t%d\t%d\t%s\t1000\t+\t%d\t%d\t0,0,0\t%d\t%s\t%s\n" % (
        q_name, start, end, name, start, end, len(rows), ",".join("%d" % (y - x) for x, y in rows), ",".join("%d" % (x - start) for x, _ in rows))]


def npeak(chains, q_name, rows, rec, gap):
    """rec = (name, score, strand, signalValue, pValue, qValue, absolute summit)"""
    start, end = rows[0][0], rows[-1][1]
    peak = int((start + end) / 2) - start
    status, _, prow = map_feature(chains, rec[6], rec[6], gap=gap, select=FIRST)
    if status == MAPPED and start <= prow[0][0] <= end:
        peak = prow[0][0] - start
    return ["%s\t%d\t%d\t%s\t%d\t%s\t%f\t%f\t%f\t%d\n" % (q_name, start, end, rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], peak)]


def run(bed_path, chain_path, gap=-1, threshold=0.0, keep_split=False, fmt="BED4", in_format="BED"):
    """{row number of the input: its output lines} -- per feature, since the reference writes chromosomes in set order."""
    chains = load_chains(chain_path)
    out = {}
    for n, line in enumerate(read_lines(bed_path)):
        f = line.split()
        cs = chains.get(f[0], [])
        status, k, rows = map_feature(cs, int(f[1]), int(f[2]), gap, threshold, LONGEST if keep_split else UNIQUE)
        if status != MAPPED:
            continue
        if fmt == "BED4":
            out[n] = bed4(cs[k]["qName"], rows, f[3])
        elif fmt == "BED12":
            out[n] = bed12(cs[k]["qName"], rows, f[3])
        else:
            rec = (f[3], int(f[4]), f[5][:1], float(f[6]), float(f[7]), float(f[8]), int(f[-1]) + int(f[1]))
            out[n] = npeak(cs, cs[k]["qName"], rows, rec, gap)
    return out
