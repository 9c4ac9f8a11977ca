"""
The liftover case at scale that tests/test_gpu_liftover.py checks and tools/bench_liftover.py times (a helper: no tests here).
"""
import numpy as np

from bxmi.chain import ChainTable


def scale_case(n_chains=5000, n_feat=5_000_000, seed=99):
    """>= 2 M blocks in n_chains overlapping chains of one chromosome (arrays, as bxmi.chain would deliver them) and n_feat features"""
    rng = np.random.default_rng(seed)
    nb = rng.integers(300, 600, n_chains)
    off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    total = int(off[-1])
    size = rng.integers(0, 200, total)
    gt, gq = rng.integers(0, 30, total), rng.integers(0, 30, total)
    gt[(gt == 0) & (gq == 0)] = 1
    first = np.zeros(total, dtype=bool)
    first[off[:-1]] = True
    owner = np.repeat(np.arange(n_chains), nb)

    def starts(gap):
        step = np.concatenate([[0], (size + gap)[:-1]])  # distance from the block before
        step[first] = 0
        run = np.cumsum(step)
        return run - run[off[:-1]][owner]

    bts, bqs = starts(gt), starts(gq)
    t = ChainTable()
    t.t_name = "chrT"
    span_t = (bts + size)[off[1:] - 1]
    span_q = (bqs + size)[off[1:] - 1]
    t.t_start = rng.integers(0, 400_000_000, n_chains).astype(np.int32)
    t.t_end = (t.t_start + span_t).astype(np.int32)
    t.q_start = rng.integers(0, 1_000_000_000, n_chains).astype(np.int32)
    t.q_span = span_q.astype(np.int32)
    t.q_minus = rng.integers(0, 2, n_chains).astype(np.uint8)
    t.q_name, t.ids = ["chrQ"] * n_chains, [str(i) for i in range(n_chains)]
    t.block_off, t.blk_t_start, t.blk_t_end, t.blk_q_start = off, bts.astype(np.int32), (bts + size).astype(np.int32), bqs.astype(np.int32)
    near = rng.integers(0, n_chains, n_feat)
    fs = t.t_start[near].astype(np.int64) + rng.integers(-200, span_t[near] + 200)
    fs[::5] = rng.integers(0, 420_000_000, len(fs[::5]))
    fs = np.maximum(fs, 0)
    ln = rng.integers(0, 2000, n_feat)
    ln[::11] = rng.integers(0, 3, len(ln[::11]))
    ln[::1000] = rng.integers(20000, 90000, len(ln[::1000]))  # long features: more than LO_BIG runs
    return t, fs.astype(np.int32), (fs + ln).astype(np.int32)
