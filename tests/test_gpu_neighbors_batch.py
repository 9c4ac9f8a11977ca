"""Batched before()/after() (bxmi_ivl_neighbors_batch[_dev], IntervalIndex.before_batch / after_batch,
IntervalTree.before_many / after_many): the reference's golden vectors, differential runs at scale against the per-call
path plus the host rule of intersection.pyx:232-260 and against the oracle treap, and the edges."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the _dev entry point this file drives (through IntervalIndex.neighbors_batch_dev; tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_ivl_neighbors_batch_dev",)

I32_MIN, I32_MAX = -(2**31), 2**31 - 1


@pytest.fixture(scope="module")
def IntervalIndex():
    from bxmi.intervals import IntervalIndex

    return IntervalIndex


def make_index(IntervalIndex, starts, ends):
    ix = IntervalIndex()
    ix.append(starts, ends)
    ix.seal()
    return ix


def host_rule(cand, key, k, before):
    """intersection.pyx:242-245 / :257-260 on a candidate list of insertion indices (key = ends or starts by index)."""
    cand = np.asarray(cand, dtype=np.int64)
    if len(cand) == k:
        return cand.tolist()
    if before:  # stable sort by end descending: equal ends keep their (reverse in-order) order
        o = np.argsort(-key[cand].astype(np.int64), kind="stable")
    else:
        o = np.argsort(key[cand], kind="stable")
    return cand[o[:k]].tolist()


def rows(hits, n):
    return [r[:c] for r, c in zip(hits.tolist(), n.tolist())]


# ------------------------------------------------------------------ golden --
def test_batch_matches_reference_vectors(golden_trees, IntervalIndex):
    calls = 0
    for case in golden_trees:
        if not case["neighbours"]:
            continue
        ix = make_index(IntervalIndex, case["starts"], case["ends"])
        groups = collections.defaultdict(list)
        for kind, pos, k, md, want in case["neighbours"]:
            groups[(kind, k, md)].append((pos, want))
        for (kind, k, md), items in groups.items():
            pos = np.array([p for p, _ in items], dtype=np.int64)
            fn = ix.before_batch if kind == "before" else ix.after_batch
            hits, n = fn(pos, k, md)
            assert hits.shape == (len(pos), k)
            assert rows(hits, n) == [w for _, w in items], (case["mode"], kind, k, md)
            assert all((r[c:] == -1).all() for r, c in zip(hits, n))
            calls += len(items)
    assert calls > 300


# ------------------------------------------------------------ differential --
def _layout(kind, rng, n=1_000_000, span=100_000_000):
    s = rng.integers(0, span, size=n)
    e = s + rng.integers(0, 2000, size=n)
    if kind == "clustered":  # duplicate starts and ends: the tie rules
        centers = rng.integers(0, span, size=4000)
        s = rng.choice(centers, size=n) + rng.integers(0, 40, size=n)
        e = s + rng.choice(np.array([0, 1, 10, 100, 1000]), size=n)
    if kind == "pile":  # long targets under everything: every before() window spans much of the index
        s[:20_000] = rng.integers(0, span // 10, size=20_000)
        e[:20_000] = s[:20_000] + rng.integers(span // 2, span, size=20_000)
    return s.astype(np.int32), e.astype(np.int32)


def _positions(rng, s, e, nq, span=100_000_000):
    p = rng.integers(-5000, span + 5000, size=nq)
    # positions right next to targets: end + 1 (before) and start - 1 (after) put the nearest at distance 0
    m = nq // 4
    p[:m] = e[rng.integers(0, len(e), size=m)].astype(np.int64) + rng.integers(1, 3, size=m)
    p[m:2 * m] = s[rng.integers(0, len(s), size=m)].astype(np.int64) - rng.integers(1, 3, size=m)
    return p.astype(np.int32)


@pytest.mark.parametrize("layout", ["uniform", "clustered", "pile"])
def test_batch_differential_at_scale(IntervalIndex, layout):
    from oracle import oracle as O

    rng = np.random.default_rng({"uniform": 11, "clustered": 12, "pile": 13}[layout])
    s, e = _layout(layout, rng)
    ix = make_index(IntervalIndex, s, e)
    nq = 200_000 if layout == "pile" else 2_000_000
    pos = _positions(rng, s, e, nq)
    t = O.OracleIntervalTree()
    t.insert_many(s, e)  # (left/right sort by the Python lists this keeps)
    ks = [1, 3, 17, 64]
    seen_exact_k = 0
    for md in (1, 2500, 10**6):
        sub = np.arange(0, nq, nq // (2_000 if md == 10**6 else 20_000))
        osub = sub[:: max(1, len(sub) // 300)]
        for d in (-1, +1):
            before = d < 0
            fn = ix.before_batch if before else ix.after_batch
            # the per-call candidate lists do not depend on k: one call per position, the host rule for every k
            cands = {int(i): ix.neighbors(int(pos[i]), md, d, cap=1 << 16) for i in sub}
            for k in ks:
                hits, n = fn(pos, k, md)
                assert hits.shape == (nq, k) and (n <= k).all()
                got = dict(zip(sub.tolist(), rows(hits[sub], n[sub])))
                for i in sub.tolist():
                    c = cands[i]
                    seen_exact_k += len(c) == k and k > 1
                    want = host_rule(c, e if before else s, k, before)
                    assert got[i] == want, (layout, md, d, k, int(pos[i]), len(c))
                for i in osub.tolist():
                    o = t.left(int(pos[i]), k, md) if before else t.right(int(pos[i]), k, md)
                    assert got[i] == o, ("oracle", layout, md, d, k, int(pos[i]))
    assert seen_exact_k > 0  # the unsorted `len(results) == n` answer is pinned


def test_exact_k_keeps_reverse_in_order(IntervalIndex):
    """Exactly k candidates: before() returns them in reverse in-order, NOT sorted by end (intersection.pyx:242-245)."""
    s = np.array([0, 10, 20], dtype=np.int32)
    e = np.array([95, 30, 40], dtype=np.int32)  # in-order by start: ends 95, 30, 40
    ix = make_index(IntervalIndex, s, e)
    hits, n = ix.before_batch([100, 100], 3, 1000)
    assert rows(hits, n) == [[2, 1, 0], [2, 1, 0]]
    hits, n = ix.before_batch([100], 2, 1000)  # three candidates: sorted by end, desc
    assert rows(hits, n) == [[0, 2]]
    hits, n = ix.before_batch([100], 4, 1000)
    assert rows(hits, n) == [[0, 2, 1]]


# ------------------------------------------------------------------- edges --
def test_edges(IntervalIndex):
    from bxmi import _ffi

    rng = np.random.default_rng(5)
    s = rng.integers(-1000, 1000, size=3000)
    s[:10] = I32_MIN
    s[10:20] = I32_MAX - 5
    e = s + rng.integers(0, 5, size=3000)
    s, e = s.astype(np.int32), e.astype(np.int32)
    ix = make_index(IntervalIndex, s, e)
    pos = np.array([I32_MIN, I32_MIN + 1, I32_MIN + 7, -3, 0, 5, I32_MAX - 10, I32_MAX - 1, I32_MAX], dtype=np.int32)
    for md in (-5, 0, 1, 3, 2500, I32_MAX):
        for d in (-1, 1):
            for k in (1, 2, 64):
                hits, n = ix._neighbors_batch(pos, k, md, d)
                for i, p in enumerate(pos.tolist()):
                    want = host_rule(ix.neighbors(p, md, d), e if d < 0 else s, k, d < 0)
                    assert hits[i, : n[i]].tolist() == want, (md, d, k, p)
                if md <= 0:
                    assert (n == 0).all()
    # nq = 0
    hits, n = ix.before_batch(np.empty(0, dtype=np.int32), 3)
    assert hits.shape == (0, 3) and n.shape == (0,)
    # k outside 1..64
    for k in (0, -1, 65):
        with pytest.raises(_ffi.BxmiError) as ei:
            ix.after_batch(pos, k)
        assert ei.value.code == _ffi.EINVAL
    # an empty index
    empty = make_index(IntervalIndex, np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32))
    hits, n = empty.before_batch(pos, 4)
    assert (n == 0).all() and (hits == -1).all()


def test_reversed_targets_equal_the_per_call_path(IntervalIndex):
    rng = np.random.default_rng(9)
    s = rng.integers(0, 200_000, size=20_000)
    e = s + rng.integers(0, 300, size=20_000)
    rev = rng.choice(20_000, size=500, replace=False)
    e[rev] = s[rev] - rng.integers(1, 5000, size=500)
    s, e = s.astype(np.int32), e.astype(np.int32)
    ix = make_index(IntervalIndex, s, e)
    assert ix.has_reversed
    pos = rng.integers(-100, 200_300, size=3000).astype(np.int32)
    for md in (50, 2500, 100_000):
        for d in (-1, 1):
            cands = [ix.neighbors(int(p), md, d, cap=1 << 16) for p in pos]
            for k in (1, 3, 64):
                hits, n = ix._neighbors_batch(pos, k, md, d)
                got = rows(hits, n)
                for i in range(len(pos)):
                    assert got[i] == host_rule(cands[i], e if d < 0 else s, k, d < 0), (md, d, k, int(pos[i]))


def test_dev_variant_matches_host(IntervalIndex):
    """bxmi_ivl_neighbors_batch_dev on device arrays, stream-ordered on the caller's stream: the host variant's answer, and
    n_cand = the candidate count before the cut."""
    from bxmi import _ffi

    rng = np.random.default_rng(21)
    s, e = _layout("pile", rng, n=200_000, span=20_000_000)
    ix = make_index(IntervalIndex, s, e)
    pos = _positions(rng, s, e, 300_000, span=20_000_000)
    dpos = _ffi.DeviceArray.from_numpy(pos)
    for d in (-1, 1):
        for k in (1, 8):
            hits_h, n_h = ix._neighbors_batch(pos, k, 2500, d)
            hits = _ffi.DeviceArray(len(pos) * k * 4)
            n = _ffi.DeviceArray(len(pos) * 4)
            cand = _ffi.DeviceArray(len(pos) * 8)
            ix.neighbors_batch_dev(dpos.ptr, len(pos), k, 2500, d, hits.ptr, n.ptr, cand.ptr, None)
            _ffi.call("bxmi_synchronize", None)
            assert np.array_equal(hits.to_numpy(np.int32).reshape(len(pos), k), hits_h)
            assert np.array_equal(n.to_numpy(np.int32), n_h)
            c = cand.to_numpy(np.int64)
            assert (n_h == np.minimum(c, k)).all() and (c > k).any()
            sub = np.arange(0, len(pos), 997)
            want = [len(ix.neighbors(int(pos[i]), 2500, d, cap=1 << 16)) for i in sub]
            assert c[sub].tolist() == want


# ------------------------------------------------------------ drop-in tree --
def test_tree_before_after_many_equal_per_call_loop():
    from bx.intervals.intersection import Interval, IntervalTree

    rng = np.random.default_rng(3)
    tree = IntervalTree()
    for a, b in zip(rng.integers(0, 100_000, size=5000).tolist(), rng.integers(0, 400, size=5000).tolist()):
        tree.insert_interval(Interval(a, a + b, strand=rng.choice(["+", "-"])))
    pos = rng.integers(-500, 100_500, size=2000).tolist()
    for k, md in ((1, 2500), (3, 500), (8, 100_000), (70, 2500)):
        assert tree.before_many(pos, k, md) == [tree.before(p, k, md) for p in pos], (k, md)
        assert tree.after_many(pos, k, md) == [tree.after(p, k, md) for p in pos], (k, md)
    ivs = [Interval(p, p + 10, strand=("-" if i % 3 == 0 else "+")) for i, p in enumerate(pos) if p >= 0]
    assert tree.upstream_many(ivs, 2) == [tree.upstream_of_interval(iv, 2) for iv in ivs]
    assert tree.downstream_many(ivs, 2) == [tree.downstream_of_interval(iv, 2) for iv in ivs]
    assert IntervalTree().before_many(pos[:5]) == [[]] * 5
    with pytest.raises(OverflowError):
        tree.before_many([I32_MIN])
    with pytest.raises(OverflowError):
        tree.after_many([I32_MAX])
