#!/usr/bin/env python3
"""Batched before()/after() against the per-call path: 10 M targets, 10 M positions, k = 1 and 8, max_dist 2500.

Batch: bxmi_ivl_neighbors_batch_dev on device arrays (host clock around the call and a device synchronisation, best
of --reps after one warm-up), and the host-array form (uploads and downloads included).  Per call: a Python loop of
bxmi_ivl_neighbors + the "sort, keep n" rule (IntervalTree.before/after's own path) over a 10 k subsample.
Prints one JSON line; --out also writes it to a file.
usage: python tools/bench_neighbors.py [--targets 10000000] [--queries 10000000] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bx-python_amd"))

from bxmi import _ffi  # noqa: E402
from bxmi.intervals import IntervalIndex  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--span", type=int, default=3_000_000_000 // 2)
    ap.add_argument("--max-dist", type=int, default=2500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=10_000)
    ap.add_argument("--out")
    a = ap.parse_args()
    _ffi.require_gpu()
    rng = np.random.default_rng(7)
    s = rng.integers(0, a.span, size=a.targets).astype(np.int32)
    e = (s + rng.integers(0, 5000, size=a.targets)).astype(np.int32)
    pos = rng.integers(0, a.span, size=a.queries).astype(np.int32)
    ix = IntervalIndex()
    ix.append(s, e)
    ix.seal()
    _ffi.call("bxmi_synchronize", None)
    dpos = _ffi.DeviceArray.from_numpy(pos)
    res = dict(targets=a.targets, queries=a.queries, span=a.span, max_dist=a.max_dist, runs=[])
    for d, name in ((-1, "before"), (+1, "after")):
        for k in (1, 8):
            dhits = _ffi.DeviceArray(a.queries * k * 4)
            dn = _ffi.DeviceArray(a.queries * 4)
            times = []
            for r in range(a.reps + 1):
                t0 = time.perf_counter()
                ix.neighbors_batch_dev(dpos.ptr, a.queries, k, a.max_dist, d, dhits.ptr, dn.ptr, None, None)
                _ffi.call("bxmi_synchronize", None)
                if r:
                    times.append(time.perf_counter() - t0)
            dev_s = min(times)
            t0 = time.perf_counter()
            hits, n = ix._neighbors_batch(pos, k, a.max_dist, d)
            host_s = time.perf_counter() - t0
            assert np.array_equal(dhits.to_numpy(np.int32).reshape(a.queries, k), hits) and np.array_equal(dn.to_numpy(np.int32), n)
            sub = np.arange(0, a.queries, max(1, a.queries // a.loop))[: a.loop]
            key = e if d < 0 else s
            t0 = time.perf_counter()
            for i in sub.tolist():
                c = ix.neighbors(int(pos[i]), a.max_dist, d).tolist()
                if len(c) != k:
                    c = sorted(c, key=key.__getitem__, reverse=d < 0)[:k]
            loop_s = time.perf_counter() - t0
            run = dict(op=name, k=k, batch_dev_ms=round(dev_s * 1e3, 3), batch_dev_ns_per_query=round(dev_s / a.queries * 1e9, 2),
                       batch_host_ms=round(host_s * 1e3, 3), per_call_us=round(loop_s / len(sub) * 1e6, 2),
                       speedup_dev=round((loop_s / len(sub)) / (dev_s / a.queries), 1), mean_hits=round(float(n.mean()), 3))
            res["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
            dhits.free()
            dn.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
