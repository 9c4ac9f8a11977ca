#!/usr/bin/env python
"""
The seeded synthetic liftover case of tests/golden/bnmapper: syn.chain (60 chains on 2 source chromosomes, 1-399 blocks
each, gaps 0-39 on either side and never both 0, either query strand, overlapping spans) and syn.bed (3000 features, every
second one placed near a chain, lengths 0-2999, every seventh 0-2).  PCG64 seed 701.

usage: gen_liftover_case.py OUTDIR        (the golden directory keeps them as `gzip -9n`; tools/record_liftover_golden.py then
                                           records what the reference answers)
"""
import os
import sys

import numpy as np


def generate(outdir, seed=701):
    rng = np.random.default_rng(seed)
    tsz = {"chrA": 5_000_000, "chrB": 3_000_000}
    qsz = {"chrX": 6_000_000, "chrY": 4_000_000}
    out, cid = [], 0
    for tname, T in tsz.items():
        for _ in range(30):
            nb = int(rng.integers(1, 400))
            S = rng.integers(1, 300, nb)
            dt, dq = rng.integers(0, 40, nb - 1), rng.integers(0, 40, nb - 1)
            dt[(dt == 0) & (dq == 0)] = 1  # a chain never has both gaps zero
            tspan, qspan = int(S.sum() + dt.sum()), int(S.sum() + dq.sum())
            ts = int(rng.integers(0, T - tspan))
            qname = list(qsz)[int(rng.integers(0, 2))]
            Q = qsz[qname]
            qs = int(rng.integers(0, Q - qspan))
            qstrand = "+-"[int(rng.integers(0, 2))]
            cid += 1
            out.append("chain %d %s %d + %d %d %s %d %s %d %d %d" % (int(rng.integers(1, 10**6)), tname, T, ts, ts + tspan, qname, Q, qstrand, qs, qs + qspan, cid))
            out += ["%d\t%d\t%d" % (S[i], dt[i], dq[i]) for i in range(nb - 1)]
            out += ["%d" % S[-1], ""]
    with open(os.path.join(outdir, "syn.chain"), "w") as f:
        f.write("\n".join(out) + "\n")
    heads = [line.split() for line in out if line.startswith("chain")]
    with open(os.path.join(outdir, "syn.bed"), "w") as f:
        for i in range(3000):
            if i % 2:
                h = heads[int(rng.integers(0, len(heads)))]
                a = max(int(rng.integers(int(h[5]) - 200, int(h[6]) + 200)), 0)
                tn = h[2]
            else:
                tn = list(tsz)[int(rng.integers(0, 2))]
                a = int(rng.integers(0, tsz[tn] - 5000))
            L = int(rng.integers(0, 3000)) if i % 7 else int(rng.integers(0, 3))
            f.write("%s\t%d\t%d\tf%d\n" % (tn, a, a + L, i))


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else ".")
