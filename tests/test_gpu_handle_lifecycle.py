"""
Long-lived interval handles on the MI355X (run with -m gpu): everything a large batch leaves on a handle -- bucket geometry,
the five kinds of images, the (end, id) pairs, the feedback of the 8-bit counts, the order-check streak, the grow-only query
scratch -- must be forgotten or rebuilt by bxmi_ivl_seal after more appends, and must not depend on the knobs turned or the
batch sizes seen in between.

The checker is the CPU oracle treap (oracle/ivtree.c), which grows incrementally too; every comparison is bit-exact.  A
resealed handle L is also compared with a fresh handle F built from the concatenated arrays: same answers, same introspection
(bxmi_ivl_*_state).  What keeps a stale image from passing unnoticed is asserted on the oracle's answers alone
(_phase_plan): from one phase to the next at least a quarter of the counts change, and some hit list changes before its end.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def IntervalIndex():
    from bxmi.intervals import IntervalIndex

    return IntervalIndex


def set_opt(key, value):
    from bxmi import _ffi

    _ffi.call("bxmi_set_option", key.encode(), int(value))


def _library_defaults():
    """every knob's value as the library starts with (bxmi_option_at): read at import, before any test turns one"""
    from bxmi import _ffi

    return _ffi.options()


DEFAULT_OPTS = _library_defaults()


def reset_opts():
    for k, v in DEFAULT_OPTS.items():
        set_opt(k, v)


def _erange_contract(ix, qs, qe, want_off):
    """bxmi_ivl_find with a hit buffer that is too small: BXMI_ERANGE, the offsets and the total valid, the buffer untouched."""
    from bxmi import _ffi

    qs, qe = np.ascontiguousarray(qs, dtype=np.int32), np.ascontiguousarray(qe, dtype=np.int32)
    cap = max(1, int(want_off[-1]) // 3)
    offsets = np.full(len(qs) + 1, -7, dtype=np.int64)
    hits = np.full(cap, -5, dtype=np.int32)
    total = C.c_int64(0)
    rc = _ffi.call("bxmi_ivl_find", ix._h, _ffi.ptr(qs), _ffi.ptr(qe), len(qs), _ffi.ptr(offsets), _ffi.ptr(hits), cap, C.byref(total), allow=(_ffi.ERANGE,))
    assert rc == _ffi.ERANGE and total.value == int(want_off[-1])
    assert np.array_equal(offsets, want_off), np.nonzero(offsets != want_off)[0][:8]
    assert (hits == -5).all()


def make_index(IntervalIndex, starts, ends):
    ix = IntervalIndex()
    ix.append(starts, ends)
    ix.seal()
    return ix


def _i32(*arrays):
    return tuple(np.ascontiguousarray(np.clip(a, -(2**31), 2**31 - 1), dtype=np.int32) for a in arrays)


def _same(got, want, *what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0] if len(got) == len(want) else None
    assert bad is not None and len(bad) == 0, (what, len(got), len(want), None if bad is None else (bad[:6], np.asarray(got)[bad[:6]], np.asarray(want)[bad[:6]]))


def _messy_queries(rng, nq, span, long_share, long_max):
    """a shuffled batch over [0, span + 2000): mostly windows of 1..3000, and a messy share as in test_bitmap_pass_differential --
    zero-length, reversed, longer than a record holds, left and right of the grid, the int32 extremes"""
    qs = rng.integers(0, span + 2000, size=nq)
    qe = qs + rng.integers(1, 3000, size=nq)
    k, kl = nq // 50, max(1, int(nq * long_share))
    qe[:k] = qs[:k]
    qe[k:2 * k] = qs[k:2 * k] - rng.integers(1, 50, size=k)
    qs[2 * k:3 * k] = rng.integers(-(2**31), 1000, size=k)
    qe[2 * k:3 * k] = qs[2 * k:3 * k] + rng.integers(1, 2000, size=k)
    qs[3 * k:4 * k] = rng.integers(span + 2000, 2**31 - 5000, size=k)
    qe[3 * k:4 * k] = qs[3 * k:4 * k] + rng.integers(1, 2000, size=k)
    qe[4 * k:4 * k + kl] = qs[4 * k:4 * k + kl] + rng.integers(32766, long_max, size=kl)
    qs[4 * k + kl:4 * k + kl + 4] = [-(2**31), 2**31 - 1, 900, 999]
    qe[4 * k + kl:4 * k + kl + 4] = [2**31 - 1, 2**31 - 1, 1001, 1000]
    p = rng.permutation(nq)
    return _i32(qs[p], qe[p])


def _host_rule(cand, key, k, before):
    """intersection.pyx:242-245 / :257-260 on a candidate list of insertion indices (key = ends or starts by index)"""
    cand = np.asarray(cand, dtype=np.int64)
    if len(cand) == k:
        return cand.tolist()
    o = np.argsort(-key[cand].astype(np.int64), kind="stable") if before else np.argsort(key[cand], kind="stable")
    return cand[o[:k]].tolist()


def _rows(hits, n):
    return [r[:c] for r, c in zip(hits.tolist(), n.tolist())]


def _check_neighbors(ix, pos, s, e, k, md, oracle_rows=None, n_oracle=0, oracle_before=True):
    """before_batch / after_batch against the per-call candidate lists + the host's rule for every position, and against the
    oracle's left() / right() for the first n_oracle of them"""
    for before in (True, False):
        hits, cnt = (ix.before_batch if before else ix.after_batch)(pos, k, md)
        assert hits.shape == (len(pos), k)
        got = _rows(hits, cnt)
        for i, p in enumerate(pos.tolist()):
            cand = ix.neighbors(p, md, -1 if before else +1, cap=1 << 14)
            assert got[i] == _host_rule(cand, e if before else s, k, before), ("before" if before else "after", i, p, len(cand))
        if oracle_rows is not None and (oracle_before or not before):
            want = oracle_rows[0 if before else 1]
            assert got[:n_oracle] == want[:n_oracle], ("oracle", "before" if before else "after", [i for i in range(n_oracle) if got[i] != want[i]][:5])


# ------------------------------------------------- 1. one handle grown through every regime --
SPAN = 40_000_000  # bucket width 2^15 until phase 4 moves both ends of the grid
NQ_COUNT = 200_000  # (offset cells take a batch that brings 4096 queries per unit image: 39 units at phases 1)
NQ_FIND = 70_000
N_ONE = 36
N_POS = 240
N_POS_ORACLE = 60
PHASES = ["P0 small", "P1 sparse", "P2 dense", "P3 clumped", "P4 wide", "P5 reversed"]


def _phase_chunks():
    """What each phase appends.  Each crosses one predicate of bm_choose_stage / the *_prepare_index functions:
    P0  3000 intervals                                              n < 4096: no image stage
    P1  + 120 000 uniform (one per 325 coordinates)                 offset cells of 256 coordinates, 8-bit counts
    P2  + 650 000 uniform (span / n = 52 < 64, 1.2 keys per 64)     too dense for offset cells: flat walk on bitmap cells
    P3  + 10 000 windows of four coordinates, eight targets each    20 000 cells with several duplicated coordinates (8000 per
                                                                    million > ivl.bm_hard_ppm): bitmap cells refuse
    P4  + one target from -3e8 into the middle, one at 1.7e9        cmin moves, bucket width 2^20 > 2^BD_MAX_SHIFT
    P5  + 30 000 uniform, one of them reversed                      has_reversed: the general path
    (P4's long target is under half of the queries and P5 brings ordinary targets along, so that the answers change enough for
    a stale index to be noticed.)"""
    rng = np.random.default_rng(20240)
    chunks = []
    for n in (3000, 120_000, 650_000):
        s = rng.integers(1000, SPAN, size=n)
        chunks.append((s, s + rng.integers(0, 1500, size=n)))
    hot = rng.integers(1000, SPAN - 2000, size=10_000)
    s = np.repeat(hot, 8) + rng.integers(0, 4, size=80_000)
    chunks.append((s, s + 1200))
    chunks.append((np.array([-300_000_000, 1_700_000_000]), np.array([20_000_000, 1_700_000_100])))
    s = rng.integers(1000, SPAN, size=30_000)
    e = s + rng.integers(0, 1500, size=30_000)
    s[17], e[17] = 10_000_500, 10_000_000
    chunks.append((s, e))
    return [_i32(s, e) for s, e in chunks]


class _Phase:
    pass


@pytest.fixture(scope="module")
def phase_plan(O):
    return _build_phase_plan(O)


def _build_phase_plan(O):
    """The chunks, the batches (the same at every phase) and the oracle's answers per phase -- computed once, on the CPU."""
    rng = np.random.default_rng(515)
    chunks = _phase_chunks()
    qs, qe = _messy_queries(rng, NQ_COUNT, SPAN, 0.005, 5_000_000)
    fqs, fqe = _messy_queries(rng, NQ_FIND, SPAN, 0.003, 300_000)
    so, fo = np.argsort(qs, kind="stable"), np.argsort(fqs, kind="stable")
    all_s, all_e = np.concatenate([c[0] for c in chunks]), np.concatenate([c[1] for c in chunks])
    pos = rng.integers(-5000, SPAN + 5000, size=N_POS)
    pos[0::3] = all_e[rng.integers(0, len(all_e), size=len(pos[0::3]))].astype(np.int64) + rng.integers(1, 3, size=len(pos[0::3]))
    pos[1::3] = all_s[rng.integers(0, len(all_s), size=len(pos[1::3]))].astype(np.int64) - rng.integers(1, 3, size=len(pos[1::3]))
    pos = _i32(pos)[0]
    t = O.OracleIntervalTree()
    phases = []
    for p, (cs, ce) in enumerate(chunks):
        t.insert_many(cs, ce)  # (left() / right() sort by the Python lists this keeps)
        ph = _Phase()
        ph.name = PHASES[p]
        ph.n = len(t)
        ph.s, ph.e = np.concatenate([c[0] for c in chunks[:p + 1]]), np.concatenate([c[1] for c in chunks[:p + 1]])
        ph.reversed = bool((ph.e < ph.s).any())
        ph.order = t.traverse()
        ph.qs, ph.qe, ph.so = qs, qe, so
        ph.want_c, ph.want_t = t.count_batch(qs, qe)
        ph.fqs, ph.fqe, ph.fo = fqs, fqe, fo
        ph.want_off, ph.want_hits = t.find_batch(fqs, fqe)
        ph.sfqs, ph.sfqe = np.ascontiguousarray(fqs[fo]), np.ascontiguousarray(fqe[fo])
        ph.swant_off, ph.swant_hits = t.find_batch(ph.sfqs, ph.sfqe)
        ph.pos = pos
        ph.want_nb = ([t.left(int(x), 3, 2500) for x in pos[:N_POS_ORACLE]], [t.right(int(x), 3, 2500) for x in pos[:N_POS_ORACLE]])
        ph.want_cl = {}
        if not ph.reversed:
            for md in (0, 300):
                regs = O.cluster_regions(ph.s, ph.e, None, md, 0)
                ph.want_cl[md] = (np.array([r[0] for r in regs]), np.array([r[1] for r in regs]),
                                  np.concatenate([[0], np.cumsum([len(r[2]) for r in regs])]), np.concatenate([r[2] for r in regs]))
        phases.append(ph)
    # The condition that keeps a stale image, rank table or (end, id) array from passing: the answers move with every phase.
    for p in range(1, len(phases)):
        a, b = phases[p - 1], phases[p]
        b.changed = float((a.want_c != b.want_c).mean())
        assert b.changed >= 0.25, (b.name, b.changed)
        ca, cb = np.diff(a.want_off), np.diff(b.want_off)
        b.mid_changes = 0
        for i in np.nonzero((ca > 0) & (cb > ca))[0][:4000].tolist():
            old = a.want_hits[a.want_off[i]:a.want_off[i + 1]]
            if not np.array_equal(b.want_hits[b.want_off[i]:b.want_off[i] + len(old)], old):
                b.mid_changes += 1  # (not merely longer: an old hit has moved)
        assert b.mid_changes > 0, b.name
    phases[0].changed, phases[0].mid_changes = 1.0, 0
    print("\nphase plan: " + "; ".join("%s n=%d counts changed %.3f lists changed inside %d" % (ph.name, ph.n, ph.changed, ph.mid_changes) for ph in phases))
    return phases


@pytest.fixture(scope="module")
def bystander(O):
    """the second index of count_multi_dev: sealed once per walk, never resealed"""
    rng = np.random.default_rng(616)
    s = rng.integers(0, 5_000_000, size=20_000)
    s, e = _i32(s, s + rng.integers(0, 2000, size=20_000))
    qs = rng.integers(-1000, 5_003_000, size=50_000)
    qs, qe = _i32(qs, qs + rng.integers(0, 4000, size=50_000))
    t = O.OracleIntervalTree()
    t.insert_many_arrays(s, e)
    return s, e, qs, qe, t.count_batch(qs, qe)


CONFIGS = {
    "defaults": {},
    "slices": {"ivl.dense": 0, "ivl.flat": 0, "ivl.slice": 1},
    "dense": {"ivl.flat": 0, "ivl.dense": 1},
    "flat": {"ivl.flat": 1, "ivl.dense": 1},
    "sparse": {"ivl.sparse": 1},
    "clumped": {"ivl.clumped": 1, "ivl.flat": 0},
}


def _states(ix):
    return {"slice": ix.slice_state(), "flat": ix.flat_state(), "dense": ix.dense_state(), "sparse": ix.sparse_state(), "bits": ix.count_width()[0]}


def _assert_stage(cfg, p, st, bits_at_seal):
    """The stage a FRESH handle reaches per phase: a property of the input and the knobs (bm_choose_stage read top to bottom;
    the chunks of P2 and P3 are sized so that their rank tables and overflow entries fit a unit image)."""
    sl, fl, dn, sp = st["slice"][0], st["flat"][0], st["dense"][0], st["sparse"][0]
    what = (cfg, PHASES[p], st)
    if p in (0, 5):  # n < 4096 / reversed targets: no stage is even asked
        assert (sl, fl, dn, sp) == (0, 0, 0, 0), what
        return
    if cfg == "defaults":
        if p == 1:
            # (8-bit counts by the density; the messy share of the batch -- one "ask again" in twelve -- then makes the feedback
            # give them up, on L and F alike)
            assert sp == 1 and st["sparse"][2] == 8 and bits_at_seal == 8 and fl == 0 and dn == 0, what
        elif p == 2:
            assert fl == 1 and sp == 0 and dn == 0, what
        elif p == 3:  # bitmap cells refuse, the clumped layout takes over
            assert fl == -1 and st["flat"][1] > 5000 and sp == 2 and dn == 0, what
        else:  # bucket width 2^20: offset cells refuse at once; bitmap cells and dense images refuse too where the slices do not fit
            assert sp == -1 and fl <= 0 and dn <= 0 and sl in (1, -1), what
    elif cfg == "slices":
        assert (fl, dn, sp) == (0, 0, 0) and sl == 1, what
    elif cfg == "dense":
        assert (fl, sp) == (0, 0) and dn == (1 if p < 4 else -1), what
    elif cfg == "flat":
        assert sp == 0 and (fl == 1 if p in (1, 2) else fl == -1), what
        assert dn == (0 if p in (1, 2) else 1 if p == 3 else -1), what
    elif cfg == "sparse":
        if p == 1:
            assert sp == 1 and st["sparse"][2] == 8 and fl == 0 and dn == 0, what
        elif p == 2:
            assert sp == 0 and fl == 1, what
        elif p == 3:
            assert fl == -1 and sp == 2 and dn == 0, what
        else:
            assert sp == -1 and fl <= 0 and dn <= 0, what
    elif cfg == "clumped":
        assert fl == 0 and sp == (2 if p < 4 else -1), what


def _exercise(IntervalIndex, ix, ph, other, by, tag):
    """Every call of the walk on one handle, in a fixed order, each against the oracle."""
    from bxmi import _ffi

    assert len(ix) == ph.n and ix.has_reversed == ph.reversed, tag
    _same(ix.order(), ph.order, tag, "order")
    got, tot = ix.count(ph.qs, ph.qe)
    _same(got, ph.want_c, tag, "count, shuffled", _states(ix))
    assert tot == ph.want_t, (tag, "total, shuffled")
    got, tot = ix.count(ph.qs[ph.so], ph.qe[ph.so])
    _same(got, ph.want_c[ph.so], tag, "count, sorted", _states(ix))
    assert tot == ph.want_t, (tag, "total, sorted")
    assert ix.count(ph.qs, ph.qe, want_counts=False) == (None, ph.want_t), (tag, "total only")
    set_opt("ivl.bitmap_min", 1)  # (find() through the exchange takes batches of ivl.bitmap_min queries and more)
    try:
        off, hits = ix.find(ph.fqs, ph.fqe)
        _same(off, ph.want_off, tag, "find offsets, shuffled")
        _same(hits, ph.want_hits, tag, "find hits, shuffled")
        off, hits = ix.find(ph.sfqs, ph.sfqe)
        _same(off, ph.swant_off, tag, "find offsets, sorted")
        _same(hits, ph.swant_hits, tag, "find hits, sorted")
        _erange_contract(ix, ph.fqs, ph.fqe, ph.want_off)
    finally:
        set_opt("ivl.bitmap_min", DEFAULT_OPTS["ivl.bitmap_min"])
    for i in range(N_ONE):
        i = i * 97 % NQ_FIND
        want = ph.want_hits[ph.want_off[i]:ph.want_off[i + 1]]
        assert ix.find_one(int(ph.fqs[i]), int(ph.fqe[i])).tolist() == want.tolist(), (tag, "find_one", i)
    # (with reversed targets before() reports the union of what the reference's pruned walk can report: documented in
    # test_gpu_intervals.py; after() is the reference's)
    _check_neighbors(ix, ph.pos, ph.s, ph.e, 3, 2500, ph.want_nb, N_POS_ORACLE, oracle_before=not ph.reversed)
    for md, (ws, we, woff, wmem) in ph.want_cl.items():
        cs, ce, off, mem = ix.clusters(md)
        _same(cs, ws, tag, "cluster starts", md)
        _same(ce, we, tag, "cluster ends", md)
        _same(off, woff, tag, "cluster offsets", md)
        _same(mem, wmem, tag, "cluster members", md)
    dq = [_ffi.DeviceArray.from_numpy(a) for a in (ph.qs, ph.qe, by[2], by[3])]
    dc = [_ffi.DeviceArray(4 * len(ph.qs)), _ffi.DeviceArray(4 * len(by[2]))]
    totals = _ffi.DeviceArray(16)
    totals.zero()
    IntervalIndex.count_multi_dev([ix, other], [dq[0].ptr, dq[2].ptr], [dq[1].ptr, dq[3].ptr], [len(ph.qs), len(by[2])], [dc[0].ptr, dc[1].ptr],
                                  [totals.ptr, totals.ptr + 8], None)
    _ffi.call("bxmi_synchronize", None)
    _same(dc[0].to_numpy(np.int32, len(ph.qs)), ph.want_c, tag, "count_multi_dev, the grown index")
    _same(dc[1].to_numpy(np.int32, len(by[2])), by[4][0], tag, "count_multi_dev, the bystander")
    assert totals.to_numpy(np.int64, 2).tolist() == [ph.want_t, by[4][1]], (tag, "count_multi_dev totals")
    for a in dq + dc + [totals]:
        a.free()
    return _states(ix)


@pytest.mark.parametrize("walk", ["every_seal", "two_appends", "seal_twice"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_handle_grown_through_every_regime(O, IntervalIndex, phase_plan, bystander, cfg, walk):
    """One handle L, a chunk appended and a seal per phase (_phase_chunks), under the default knobs and with each search stage
    forced in turn.  After each seal a fresh handle F is built from the concatenated arrays; L and F make the same calls in the
    same order (_exercise), every answer is compared with the oracle, and L's introspection with F's (wide_counts and the
    order reports arrive late by design and are left out).  F must report the stage the phase is meant to reach
    (_assert_stage).  Walks: queried after every seal; two appends with no query in between (phases 1, 3, 5 are queried);
    seal() twice in a row."""
    L = IntervalIndex()
    reset_opts()
    set_opt("ivl.partition", 1)
    for k, v in CONFIGS[cfg].items():
        set_opt(k, v)
    try:
        other = make_index(IntervalIndex, bystander[0], bystander[1])
        chunks = _phase_chunks()
        for p, ph in enumerate(phase_plan):
            L.append(*chunks[p])
            if walk == "two_appends" and p % 2 == 0:
                continue
            L.seal()
            if walk == "seal_twice":
                L.seal()
            F = make_index(IntervalIndex, ph.s, ph.e)
            bits_l, bits_f = L.count_width()[0], F.count_width()[0]  # before any pass: the density rule alone
            assert bits_l == bits_f, (cfg, walk, ph.name, bits_l, bits_f)
            st_l = _exercise(IntervalIndex, L, ph, other, bystander, (cfg, walk, ph.name, "resealed"))
            st_f = _exercise(IntervalIndex, F, ph, other, bystander, (cfg, walk, ph.name, "fresh"))
            print("stage report: %s | %s | %s | changed %.3f | %s" % (cfg, walk, ph.name, ph.changed, st_f))
            assert st_l == st_f, (cfg, walk, ph.name, "resealed", st_l, "fresh", st_f)
            _assert_stage(cfg, p, st_f, bits_f)
            F.close()
        other.close()
    finally:
        reset_opts()
        L.close()


# --------------------------------------------------- 2. per-handle feedback across a reseal --
def test_order_check_streak_is_forgotten_by_a_reseal(O, IntervalIndex):
    """The handle is driven to "the order check is no longer launched" (the recipe of test_order_check_is_dropped_and_comes_back),
    then grows and is resealed right after a shuffled batch, whose order report may still be on its way: the streak belongs to
    the index that was.  The check is back, sorted batches are exact (twice: the second has the first one's report), and so is
    the next shuffled one."""
    rng = np.random.default_rng(95)
    n, span, nq = 150_000, 40_000_000, 32768 * 10 + 1234
    s = rng.integers(1000, span, size=n + 100_000)
    s, e = _i32(s, s + rng.integers(1, 1500, size=len(s)))
    qs = rng.integers(0, span, size=nq)
    qs, qe = _i32(qs, qs + rng.integers(1, 2500, size=nq))
    o = np.argsort(qs, kind="stable")
    t = O.OracleIntervalTree()
    t.insert_many_arrays(s[:n], e[:n])
    want, want_total = t.count_batch(qs, qe)
    ix = make_index(IntervalIndex, s[:n], e[:n])
    set_opt("ivl.partition", 1)
    set_opt("ivl.flat", 1)
    set_opt("ivl.dense", 1)
    try:
        assert ix.order_state()[0] == 0
        for k in range(3):
            got, total = ix.count(qs, qe)
            assert np.array_equal(got, want) and total == want_total, ("shuffled", k)
        assert ix.order_state()[0] == 1, ix.order_state()
        got, total = ix.count(qs, qe)  # one more without the check ...
        ix.append(s[n:], e[n:])        # ... and the index grows at once
        ix.seal()
        assert np.array_equal(got, want) and total == want_total
        assert ix.order_state()[0] == 0, ix.order_state()
        t.insert_many_arrays(s[n:], e[n:])
        want2, want2_total = t.count_batch(qs, qe)
        assert (want2 != want).mean() > 0.25
        for k in range(2):
            got, total = ix.count(qs[o], qe[o])
            assert np.array_equal(got, want2[o]) and total == want2_total, ("sorted after the reseal", k)
        got, total = ix.count(qs, qe)
        assert np.array_equal(got, want2) and total == want2_total, "shuffled after the reseal"
        assert ix.flat_state()[0] == 1
    finally:
        reset_opts()


def test_count_width_feedback_is_forgotten_by_a_reseal(O, IntervalIndex):
    """The handle is driven to 16-bit counts (the recipe of test_count_width_feedback: a crowd whose counts do not fit 8 bits),
    then grows and is resealed: the feedback belongs to the index that was, and the density rule of bxmi_ivl_count_width (fewer
    than 128 targets per 2048 coordinates) says 8 bits again.  Exact counts before and after, off the crowd and inside it."""
    rng = np.random.default_rng(91)
    span = 30_000_000
    s = np.concatenate([rng.integers(1000, span, size=400_000), rng.integers(5_000_000, 5_400_000, size=150_000), rng.integers(1000, span, size=50_000)])
    s, e = _i32(s, s + rng.integers(1, 300, size=len(s)))
    n = 550_000
    nq = 32768 * 12 + 99
    calm_s = rng.integers(6_000_000, span, size=nq)
    calm_s, calm_e = _i32(calm_s, calm_s + rng.integers(1, 800, size=nq))
    crowd_s = rng.integers(5_000_000, 5_400_000, size=nq)
    crowd_s, crowd_e = _i32(crowd_s, crowd_s + rng.integers(900, 1200, size=nq))
    t = O.OracleIntervalTree()
    t.insert_many_arrays(s[:n], e[:n])
    want_calm, want_crowd = t.count_batch(calm_s, calm_e), t.count_batch(crowd_s, crowd_e)
    assert (want_crowd[0] >= 255).mean() > 0.9
    ix = make_index(IntervalIndex, s[:n], e[:n])
    set_opt("ivl.partition", 1)
    set_opt("ivl.flat", 1)
    set_opt("ivl.bm_hard_ppm", 10**6)  # (the crowd has cells with several duplicated coordinates: keep the cell images anyway)
    try:
        got = ix.count(calm_s, calm_e)
        assert ix.flat_state()[0] == 1
        assert np.array_equal(got[0], want_calm[0]) and got[1] == want_calm[1]
        assert ix.count_width() == (8, 0)
        for _ in range(10):  # (the mirror in host memory is a pass or two behind the kernels that write it)
            got = ix.count(crowd_s, crowd_e)
            assert np.array_equal(got[0], want_crowd[0]) and got[1] == want_crowd[1]
            if ix.count_width()[0] == 16:
                break
        assert ix.count_width()[0] == 16, ix.count_width()
        ix.append(s[n:], e[n:])
        ix.seal()
        assert len(s) * 2048 < (int(e.max()) - int(s.min()) + 1) * 128  # the header's rule for this index: 8 bits
        assert ix.count_width() == (8, 0), ix.count_width()
        t.insert_many_arrays(s[n:], e[n:])
        want_calm2, want_crowd2 = t.count_batch(calm_s, calm_e), t.count_batch(crowd_s, crowd_e)
        assert (want_calm2[0] != want_calm[0]).mean() > 0.25
        got = ix.count(calm_s, calm_e)
        assert ix.flat_state()[0] == 1
        assert np.array_equal(got[0], want_calm2[0]) and got[1] == want_calm2[1], "off the crowd, after the reseal"
        for k in range(3):
            got = ix.count(crowd_s, crowd_e)
            assert np.array_equal(got[0], want_crowd2[0]) and got[1] == want_crowd2[1], ("inside the crowd, after the reseal", k)
    finally:
        reset_opts()


# ------------------------------------------------------ 3. knob walk on a live handle, no reseal --
KNOBS = {  # (the values the tests of test_gpu_intervals.py set)
    "ivl.partition": [1, 1, 1, -1],
    "ivl.bitmap": [-1, -1, 0],
    "ivl.flat": [-1, 0, 1],
    "ivl.dense": [-1, 0, 1],
    "ivl.slice": [-1, 0, 1],
    "ivl.sparse": [-1, 1],
    "ivl.clumped": [-1, 0, 1],
    "ivl.sorted_path": [0, 1],
    "ivl.sorted_cells": [0, 1],
    "ivl.bm_variant": [-1, 0, 1, 2],
    "ivl.bd_chunk": [0, 1024, 4096, 8192, 20000, 65536, 1 << 20],
    "ivl.bd_w8": [-1, 0, 1],
    "ivl.find_sliced": [0, 1],
    "ivl.fx_direct": [0, 1],
    "ivl.order_skip": [-1, 0],
    "ivl.tot_walk": [0, 1],
    "ivl.sl_f": [-1, 0, 1, 2, 3, 4, 6],
    "ivl.sl_lanes": [0, 1, 16, 64],
    "ivl.sl_flat": [0, 1],
}


@pytest.mark.parametrize("kind", ["sparse", "dense", "dups"])
def test_knob_walk_on_a_live_handle(O, IntervalIndex, kind):
    """include/bxmi.h on the knobs: "Results never depend on them".  A seeded random walk of 30 steps over the knobs, on a
    handle that is never resealed -- so the stages are prepared, refused and retried (bo_state -1 / 0 / 1 / 2, the clumped
    retry) in orders no other test reaches; after every step a shuffled count, a sorted count, a total and a find() against
    the oracle's answers, which are computed once."""
    seed = ["sparse", "dense", "dups"].index(kind)
    rng = np.random.default_rng(300 + seed)
    n, span = (300_000, 6_000_000) if kind == "dense" else (120_000, 40_000_000)
    s = rng.integers(1000, span, size=n)
    if kind == "dups":  # the "dups" shape of test_bitmap_pass_differential
        s[: n // 2] = rng.choice(s[n // 2:], size=n // 2)
        s[:2000] = rng.integers(5_000_000, 5_000_064, size=2000)
    s, e = _i32(s, s + rng.integers(0, 1500, size=n))
    qs, qe = _messy_queries(rng, 70_000, span, 0.005, 5_000_000)
    fqs, fqe = _messy_queries(rng, 30_000, span, 0.003, 300_000)
    so = np.argsort(qs, kind="stable")
    t = O.OracleIntervalTree()
    t.insert_many_arrays(s, e)
    want, want_total = t.count_batch(qs, qe)
    want_off, want_hits = t.find_batch(fqs, fqe)
    ix = make_index(IntervalIndex, s, e)
    names = sorted(KNOBS)
    now = {}
    try:
        set_opt("ivl.bitmap_min", 1)  # (so that find() reaches the exchange whenever ivl.partition = 1)
        for step in range(30):
            for k in names:
                if rng.random() < 0.35:
                    now[k] = int(rng.choice(KNOBS[k]))
                    set_opt(k, now[k])
            tag = (kind, step, dict(now))
            got, total = ix.count(qs, qe)
            _same(got, want, tag, "count, shuffled", _states(ix))
            assert total == want_total, tag
            got, total = ix.count(qs[so], qe[so])
            _same(got, want[so], tag, "count, sorted", _states(ix))
            assert total == want_total, tag
            assert ix.count(qs, qe, want_counts=False)[1] == want_total, (tag, "total only", _states(ix))
            off, hits = ix.find(fqs, fqe)
            _same(off, want_off, tag, "find offsets")
            _same(hits, want_hits, tag, "find hits")
        print("knob walk: %s ends with %s" % (kind, _states(ix)))
    finally:
        reset_opts()


# ------------------------------------------- 4. scratch reuse across batch sizes, natural thresholds --
def test_scratch_reuse_across_batch_sizes(O, IntervalIndex):
    """One handle, default knobs, batches of 70 000, 17, 1, 0, 3 * 16384 + 17, 2 Mi + 5, 5, 4 Mi + 3 and 33 queries: the grow-only
    scratch shared by count, find, find_one and neighbors_batch serves small batches after large ones, and the two large sizes
    cross ivl.bitmap_min and the 4 Mi partition threshold for real.  Host-pointer count, device-pointer count, find, find_one and
    before_batch / after_batch are interleaved; the multi-million batches are checked on 300 000 sampled queries plus the total."""
    from bxmi import _ffi

    rng = np.random.default_rng(404)
    n, span = 200_000, 50_000_000
    s = rng.integers(1000, span, size=n)
    s, e = _i32(s, s + rng.integers(1, 1500, size=n))
    t = O.OracleIntervalTree()
    t.insert_many(s, e)
    ix = make_index(IntervalIndex, s, e)
    sizes = [70_000, 17, 1, 0, 3 * 16384 + 17, (2 << 20) + 5, 5, (4 << 20) + 3, 33]
    assert sizes[5] >= DEFAULT_OPTS["ivl.bitmap_min"] and DEFAULT_OPTS["ivl.partition"] == -1
    for step, nq in enumerate(sizes):
        qs = rng.integers(-2000, span + 2000, size=nq)
        qs, qe = _i32(qs, qs + rng.integers(0, 2500, size=nq))
        if nq > 40:
            qe[::31] = qs[::31] - 2               # reversed
            qe[::37] = qs[::37] + 60_000          # longer than a record holds
        big = nq > (1 << 20)
        pick = rng.integers(0, nq, size=300_000) if big else np.arange(nq)
        want, _ = t.count_batch(qs[pick], qe[pick])
        want_total = t.count_batch(qs, qe, want_counts=False)[1] if big else int(want.sum())
        tag = (step, nq)
        got, total = ix.count(qs, qe)  # host pointers
        _same(got[pick], want, tag, "host count", _states(ix))
        assert total == want_total, (tag, "host total", total, want_total)
        if nq:  # device pointers, counts and total
            dq, de, dc, dt = _ffi.DeviceArray.from_numpy(qs), _ffi.DeviceArray.from_numpy(qe), _ffi.DeviceArray(4 * max(nq, 4)), _ffi.DeviceArray(8)
            dt.zero()
            ix.count_dev(dq.ptr, de.ptr, nq, dc.ptr, dt.ptr, None)
            _ffi.call("bxmi_synchronize", None)
            _same(dc.to_numpy(np.int32, nq)[pick], want, tag, "device count")
            assert int(dt.to_numpy(np.int64, 1)[0]) == want_total, (tag, "device total")
            for a in (dq, de, dc, dt):
                a.free()
        if nq <= (2 << 20) + 5:  # find(): the whole list against the oracle's
            want_off, want_hits = t.find_batch(qs, qe)
            off, hits = ix.find(qs, qe)
            _same(off, want_off, tag, "find offsets")
            _same(hits, want_hits, tag, "find hits")
            if nq:
                assert ix.find_one(int(qs[0]), int(qe[0])).tolist() == want_hits[want_off[0]:want_off[1]].tolist(), (tag, "find_one")
        # before / after for the whole batch of positions, checked on a sample
        sub = rng.integers(0, nq, size=150) if nq > 150 else np.arange(nq)
        for before in (True, False):
            hits, cnt = (ix.before_batch if before else ix.after_batch)(qs, 2, 2500)
            assert hits.shape == (nq, 2)
            for i in sub.tolist():
                row = hits[i, :cnt[i]].tolist()
                want_row = t.left(int(qs[i]), 2, 2500) if before else t.right(int(qs[i]), 2, 2500)
                assert row == want_row, (tag, "before" if before else "after", i, int(qs[i]))
    assert ix.sparse_state()[0] == 1, _states(ix)  # (one target per 250 coordinates: the large batches ran on offset cells)


# ------------------------------------------------------------------------ 5. drop-in classes --
def _dropin_steps():
    rng = np.random.default_rng(505)
    span = 30_000_000
    s = rng.integers(1000, span, size=306_000)
    s, e = _i32(s, s + rng.integers(0, 1500, size=len(s)))
    qs, qe = _messy_queries(rng, 20_000, span, 0.003, 300_000)
    return s, e, qs, qe, (3000, 6000, 306_000)


@pytest.mark.parametrize("how", ["insert", "add_interval"])
def test_dropin_tree_keeps_growing_between_finds(O, how):
    """bx.intervals.intersection.IntervalTree.insert / Intersecter.add_interval after find(): 3000 intervals and a find batch,
    6000 and a find batch (the index passes 4096 targets), 306 000 and a find batch -- each against the oracle, with a few dozen
    per-call find()s."""
    from bx.intervals.intersection import Intersecter, Interval, IntervalTree

    s, e, qs, qe, steps = _dropin_steps()
    tree = IntervalTree() if how == "insert" else Intersecter()
    t = O.OracleIntervalTree()
    done = 0
    set_opt("ivl.partition", 1)  # (20 000 queries through the large-batch paths)
    set_opt("ivl.bitmap_min", 1)
    try:
        for upto in steps:
            if how == "insert":
                for i in range(done, upto):
                    tree.insert(int(s[i]), int(e[i]), i)
            else:
                for i in range(done, upto):
                    tree.add_interval(Interval(int(s[i]), int(e[i]), value=i))
            t.insert_many_arrays(s[done:upto], e[done:upto])
            done = upto
            want_off, want_hits = t.find_batch(qs, qe)
            off, hits = tree.find_batch(qs, qe)
            _same(off, want_off, how, upto, "find_batch offsets")
            _same(hits, want_hits, how, upto, "find_batch hits")
            got, total = tree.count_batch(qs, qe)
            _same(got, np.diff(want_off), how, upto, "count_batch")
            assert total == int(want_off[-1])
            for i in range(0, 40 * 331, 331):
                found = tree.find(int(qs[i]), int(qe[i]))
                found = found if how == "insert" else [iv.value for iv in found]
                assert found == want_hits[want_off[i]:want_off[i + 1]].tolist(), (how, upto, i)
    finally:
        reset_opts()


def test_dropin_clustertree_keeps_growing_between_getregions(O):
    """ClusterTree.getregions(), 200 000 more inserts, getregions() again: both against the oracle's cluster.c."""
    from bx.intervals.cluster import ClusterTree

    rng = np.random.default_rng(506)
    n0, n1 = 5000, 205_000
    s = rng.integers(0, 200_000_000, size=n1)
    s, e = _i32(s, s + rng.integers(0, 400, size=n1))
    ids = rng.permutation(n1).astype(np.int32)
    tree = ClusterTree(300, 2)
    done = 0
    for upto in (n0, n1):
        for i in range(done, upto):
            tree.insert(int(s[i]), int(e[i]), int(ids[i]))
        done = upto
        want = O.cluster_regions(s[:upto], e[:upto], ids[:upto], 300, 2)
        got = tree.getregions()
        assert len(got) == len(want) and got == want, (upto, len(got), len(want))
        assert tree.getlines() == [i for w in want for i in w[2]]
