"""
The device-pointer entry points of the interval index (include/bxmi.h, `_dev`) against the oracle, as a caller outside
the suite uses them: caller-owned buffers at every alignment bxmi.h declares legal, guard bytes around every output, a
caller's non-blocking stream, and accumulated totals.

The host forms stage through the library's own 16-byte-aligned, grow-only scratch, so a write past the end of an output,
a store where the contract says "accumulated", work queued on another stream than the caller's, or a path that assumes an
alignment it does not check would all pass the host-form tests.  Here every output lives in a guarded buffer: G bytes of
a sentinel before and after, plus the misalignment pad, all checked after the call.

(No torch: tests/conftest.py:has_gpu explains why it must not become the process's first HIP runtime.  The caller's
stream comes from the HIP runtime libbxmi itself links.)
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# every _dev entry point of the interval index this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_ivl_find_dev", "bxmi_ivl_count_dev", "bxmi_ivl_count_multi_dev", "bxmi_ivl_append_dev", "bxmi_ivl_order_dev")

G = 256       # guard bytes on each side of an output
SENT = 0xA5   # the guard's byte
PRESET = 10**12 + 7  # what an accumulated total holds before the call


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def _ffi():
    from bxmi import _ffi

    return _ffi


def set_opt(key, value):
    _ffi().call("bxmi_set_option", key.encode(), int(value))


def _library_defaults():
    """every knob's value as the library starts with (bxmi_option_at): read at import, before any test turns one"""
    return _ffi().options()


DEFAULT_OPTS = _library_defaults()


def reset_opts():
    for k, v in DEFAULT_OPTS.items():
        set_opt(k, v)


# ---------------------------------------------------------------- helpers --
class Hip:
    """The few HIP runtime calls a stream-ordered caller makes, from the libamdhip64 libbxmi has loaded."""

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            _ffi().load()
            path = None
            with open("/proc/self/maps") as f:
                for line in f:
                    p = line.split()[-1]
                    if os.path.basename(p).startswith("libamdhip64.so"):
                        path = p
                        break
            assert path, "libbxmi is loaded but libamdhip64 is not mapped"
            L = C.CDLL(path)
            L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            L.hipStreamSynchronize.argtypes = [C.c_void_p]
            L.hipStreamDestroy.argtypes = [C.c_void_p]
            for f in (L.hipStreamCreateWithFlags, L.hipMemcpyAsync, L.hipStreamSynchronize, L.hipStreamDestroy, L.hipDeviceSynchronize):
                f.restype = C.c_int
            cls._lib = L
        return cls._lib

    @classmethod
    def check(cls, rc, what):
        assert rc == 0, "%s: hipError %d" % (what, rc)

    @classmethod
    def device_sync(cls):
        cls.check(cls.lib().hipDeviceSynchronize(), "hipDeviceSynchronize")


H2D, D2H, D2D = 1, 2, 3


class Stream:
    """A non-blocking caller stream (hipStreamNonBlocking): ordered with nothing but itself."""

    def __init__(self):
        s = C.c_void_p()
        Hip.check(Hip.lib().hipStreamCreateWithFlags(C.byref(s), 1), "hipStreamCreateWithFlags")
        self.s = s.value

    def copy_d2d(self, dst, src, nbytes):
        if nbytes:
            Hip.check(Hip.lib().hipMemcpyAsync(dst, src, nbytes, D2D, self.s), "hipMemcpyAsync D2D")

    def read(self, src, dtype, count):
        out = np.empty(count, dtype=dtype)
        if count:
            Hip.check(Hip.lib().hipMemcpyAsync(out.ctypes.data, src, out.nbytes, D2H, self.s), "hipMemcpyAsync D2H")
        return out

    def sync(self):
        Hip.check(Hip.lib().hipStreamSynchronize(self.s), "hipStreamSynchronize")

    def close(self):
        if self.s:
            Hip.check(Hip.lib().hipStreamDestroy(self.s), "hipStreamDestroy")
            self.s = None


class Guarded:
    """A caller's output (or input) buffer: `nbytes` at ptr = base + G + mis, the sentinel everywhere around it."""

    def __init__(self, nbytes, mis=0):
        assert 0 <= mis < 16
        self.nbytes, self.mis = int(nbytes), mis
        self.total = self.nbytes + 2 * G + 16
        self.buf = _ffi().DeviceArray(self.total)
        _ffi().call("bxmi_memset", self.buf.ptr, SENT, self.total)
        _ffi().call("bxmi_synchronize", None)  # (hipMemset on the null stream: landed before any other stream uses the buffer)
        self.ptr = self.buf.ptr + G + mis

    @classmethod
    def holding(cls, arr, mis=0):
        arr = np.ascontiguousarray(arr)
        g = cls(arr.nbytes, mis)
        if arr.nbytes:
            _ffi().call("bxmi_memcpy_h2d", g.ptr, arr.ctypes.data, arr.nbytes)
        return g

    def fill(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _ffi().call("bxmi_memcpy_h2d", self.ptr, arr.ctypes.data, arr.nbytes)

    def raw(self):
        out = np.empty(self.total, dtype=np.uint8)
        _ffi().call("bxmi_memcpy_d2h", out.ctypes.data, self.buf.ptr, self.total)
        return out

    def check(self, written, what, raw=None):
        """every byte outside [ptr, ptr + written) still holds the sentinel; returns the whole raw buffer"""
        raw = self.raw() if raw is None else raw
        lo, hi = G + self.mis, G + self.mis + int(written)
        bad = np.nonzero(raw[:lo] != SENT)[0]
        assert len(bad) == 0, ("%s: %d guard bytes before the buffer written" % (what, len(bad)), bad[:8] - lo)
        bad = np.nonzero(raw[hi:] != SENT)[0]
        assert len(bad) == 0, ("%s: %d bytes past the written region changed" % (what, len(bad)), bad[:8])
        return raw

    def payload(self, raw, dtype, count):
        lo = G + self.mis
        return raw[lo:lo + count * np.dtype(dtype).itemsize].view(dtype).copy()


def dev_read(ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    if count:
        _ffi().call("bxmi_memcpy_d2h", out.ctypes.data, ptr, out.nbytes)
    return out


def make_index(s, e):
    from bxmi.intervals import IntervalIndex

    ix = IntervalIndex()
    ix.append(s, e)
    ix.seal()
    return ix


# ------------------------------------------------------------------ data --
SPAN = 40_000_000
N_TARGETS = 120_000
NQ_BIG = (1 << 20) + 3 * 32768 + 4099     # >= 1 Mi (the sorted path's probe), not a multiple of 4 nor of a 32768-query tile
NQ_MID = 300_001                          # sorted, below 1 Mi: no probe
NQ_SMALL = 50_003                         # below ivl.partition's automatic threshold: the direct kernels


def _targets(rng):
    s = rng.integers(1000, SPAN, size=N_TARGETS)
    e = s + rng.integers(0, 1500, size=N_TARGETS)
    s[:500] = rng.integers(5_000_000, 5_000_040, size=500)  # duplicated coordinates
    e[:500] = s[:500] + rng.integers(0, 1500, size=500)
    return s.astype(np.int32), e.astype(np.int32)


def _queries(rng, nq):
    """shuffled queries, one in a hundred of each escape: zero-length, reversed, over-long, left and right of the grid"""
    qs = rng.integers(0, SPAN + 2000, size=nq)
    qe = qs + rng.integers(1, 2500, size=nq)
    k = nq // 100
    qe[:k] = qs[:k]
    qe[k:2 * k] = qs[k:2 * k] - rng.integers(1, 50, size=k)
    qe[2 * k:3 * k] = qs[2 * k:3 * k] + rng.integers(32766, 100_000, size=k)
    qs[3 * k:4 * k] = rng.integers(-(2**31), 1000, size=k)
    qe[3 * k:4 * k] = qs[3 * k:4 * k] + rng.integers(1, 2000, size=k)
    qs[4 * k:5 * k] = rng.integers(SPAN + 2000, 2**31 - 5000, size=k)
    qe[4 * k:5 * k] = qs[4 * k:5 * k] + rng.integers(1, 2000, size=k)
    qs[5 * k:5 * k + 4] = [-(2**31), 2**31 - 1, 900, 999]
    qe[5 * k:5 * k + 4] = [2**31 - 1, 2**31 - 1, 1001, 1000]
    p = rng.permutation(nq)
    return (np.clip(qs[p], -(2**31), 2**31 - 1).astype(np.int32), np.clip(qe[p], -(2**31), 2**31 - 1).astype(np.int32))


def _sorted(qs, qe):
    o = np.argsort(qs, kind="stable")
    return qs[o].copy(), qe[o].copy()


class World:
    """One set of targets, its oracle, and each batch's oracle answer computed once and shared by every path and placement."""

    def __init__(self, O):
        rng = np.random.default_rng(2026)
        self.s, self.e = _targets(rng)
        self.t = O.OracleIntervalTree()
        self.t.insert_many_arrays(self.s, self.e)
        # reversed targets (has_reversed: every batch takes the direct kernels)
        rs, re = _targets(rng)
        flip = rng.random(len(rs)) < 0.05
        self.rs, self.re = np.where(flip, re, rs).astype(np.int32), np.where(flip, rs, re).astype(np.int32)
        self.rt = O.OracleIntervalTree()
        self.rt.insert_many_arrays(self.rs, self.re)
        big = _queries(rng, NQ_BIG)
        srt = _sorted(*big)
        almost = (srt[0].copy(), srt[1].copy())
        # one descent near the end: the probe (a third and two thirds in) passes, the full check finds it
        i = NQ_BIG - 1000
        while almost[0][i] == almost[0][i + 1]:
            i += 1
        almost[0][[i, i + 1]] = almost[0][[i + 1, i]]
        almost[1][[i, i + 1]] = almost[1][[i + 1, i]]
        self.batches = {"unsorted": big, "sorted": srt, "almost": almost, "sorted_mid": _sorted(*_queries(rng, NQ_MID)),
                        "small": _queries(rng, NQ_SMALL), "rev": _queries(rng, NQ_SMALL)}
        self._find, self._count = {}, {}

    def tree(self, batch):
        return self.rt if batch == "rev" else self.t

    def targets(self, batch):
        return (self.rs, self.re) if batch == "rev" else (self.s, self.e)

    def find(self, batch):
        if batch not in self._find:
            self._find[batch] = self.tree(batch).find_batch(*self.batches[batch])
        return self._find[batch]

    def count(self, batch):
        if batch not in self._count:
            if batch in self._find:
                off = self._find[batch][0]
                c = np.diff(off).astype(np.int32)
                self._count[batch] = (c, int(off[-1]))
            else:
                self._count[batch] = self.tree(batch).count_batch(*self.batches[batch])
        return self._count[batch]


@pytest.fixture(scope="module")
def W(O):
    return World(O)


def _find_dev(ix, qs_ptr, qe_ptr, nq, off_ptr, hits_ptr, cap, want_total=True, stream=None):
    total = C.c_int64(-99)
    rc = _ffi().call("bxmi_ivl_find_dev", ix._h, qs_ptr, qe_ptr, nq, off_ptr, hits_ptr, cap, C.byref(total) if want_total else None, stream,
                     allow=(_ffi().ERANGE,))
    return rc, total.value


# ---------------------------------------------------------- find_dev paths --
# (name, batch, knobs, offsets misalignment, hits misalignment, queries misalignment, takes the exchange)
# Which branch of bxmi_ivl_find_dev each row selects (csrc/intervals.hip):
#   direct         nq below ivl.partition's automatic threshold (4 Mi): the direct tree kernels + device_scan.
#   reversed       has_reversed: the direct kernels even with ivl.partition forced on.
#   sorted_gated   q_aligned, sorted starts, nq >= 1 Mi, offsets 16-byte aligned: probe, order check, the gated chain of ivl_find_local.
#   sorted_scan    the same batch with offsets at +8: ivl_find_local without gate, offsets by device_scan (no chunk scan).
#   sorted_mid     sorted, nq < 1 Mi: no probe, the order check waited for, ivl_find_local with the chunk scan.
#   almost         the probe passes, the full check finds a descent: the gated chain stands down, the exchange answers.
#   fx_direct/copy shuffled: the probe finds a descent, the exchange (ivl_find_fx) with the fill straight into the list / copy.
#   partitioned    shuffled, offsets at +8: the exchange stores offsets 16 bytes at a time, so ivl_find_partitioned.
#   q4             shuffled, qs/qe at +4: not q_aligned, the direct kernels on a batch that would take the exchange.
# A fresh index per row: the slice stage (sl_state, bxmi_ivl_slice_state) is prepared only by the exchange, so
# slice_state()[0] == 1 afterwards says the exchange ran and == 0 says it did not.
BIG = {"ivl.partition": 1, "ivl.bitmap_min": 1}
FIND_PATHS = [
    ("direct", "small", {}, 0, 4, 0, False),
    ("reversed", "rev", {"ivl.partition": 1}, 0, 8, 0, False),
    ("sorted_gated", "sorted", BIG, 0, 12, 0, False),
    ("sorted_scan", "sorted", BIG, 8, 0, 0, False),
    ("sorted_mid", "sorted_mid", BIG, 0, 4, 0, False),
    ("almost", "almost", BIG, 0, 8, 0, True),
    ("fx_direct", "unsorted", dict(BIG, **{"ivl.fx_direct": 1}), 0, 12, 0, True),
    ("fx_copy", "unsorted", dict(BIG, **{"ivl.fx_direct": 0}), 0, 4, 0, True),
    ("partitioned", "unsorted", BIG, 8, 8, 0, False),
    ("q4", "unsorted", BIG, 0, 12, 4, False),
]


@pytest.mark.parametrize("name,batch,knobs,off_mis,hits_mis,q_mis,exchange", FIND_PATHS, ids=[p[0] for p in FIND_PATHS])
def test_find_dev_paths_and_placements(W, name, batch, knobs, off_mis, hits_mis, q_mis, exchange):
    """bxmi_ivl_find_dev on every path of its dispatch, outputs in guarded caller buffers at the placements bxmi.h allows:
    exact CSR offsets and hit order, the total (also with total_host = NULL), nothing written outside [offsets[0..nq]] and
    [hits[0..total)], BXMI_ERANGE with cap = total - 1 leaving the whole hit buffer alone, cap = total exactly."""
    qs, qe = W.batches[batch]
    nq = len(qs)
    want_off, want_hits = W.find(batch)
    total = int(want_off[-1])
    assert total > 1000
    ix = make_index(*W.targets(batch))
    dq, de = Guarded.holding(qs, q_mis), Guarded.holding(qe, q_mis)
    try:
        for k, v in knobs.items():
            set_opt(k, v)
        # 1. room to spare: cap = total + 1000, every byte past hits[total) is the caller's and stays as it was
        off = Guarded((nq + 1) * 8, off_mis)
        hits = Guarded((total + 1000) * 4, hits_mis)
        rc, got_total = _find_dev(ix, dq.ptr, de.ptr, nq, off.ptr, hits.ptr, total + 1000)
        Hip.device_sync()
        assert rc == _ffi().OK and got_total == total, (name, rc, got_total, total)
        raw_off = off.check((nq + 1) * 8, name + ": offsets")
        raw_hits = hits.check(total * 4, name + ": hits")
        got_off = off.payload(raw_off, np.int64, nq + 1)
        assert np.array_equal(got_off, want_off), (name, np.nonzero(got_off != want_off)[0][:8])
        got_hits = hits.payload(raw_hits, np.int32, total)
        bad = np.nonzero(got_hits != want_hits)[0]
        assert len(bad) == 0, (name, len(bad), bad[:8], got_hits[bad[:8]], want_hits[bad[:8]])
        assert ix.slice_state()[0] == (1 if exchange else 0), (name, ix.slice_state())

        # 2. BXMI_ERANGE: cap = total - 1.  The offsets and the total are valid, not one byte of the hit buffer is touched.
        off2 = Guarded((nq + 1) * 8, off_mis)
        hits2 = Guarded((total - 1) * 4, hits_mis)
        rc, got_total = _find_dev(ix, dq.ptr, de.ptr, nq, off2.ptr, hits2.ptr, total - 1)
        Hip.device_sync()
        assert rc == _ffi().ERANGE and got_total == total, (name, rc, got_total, total)
        raw_off = off2.check((nq + 1) * 8, name + ": offsets on BXMI_ERANGE")
        got_off = off2.payload(raw_off, np.int64, nq + 1)
        assert np.array_equal(got_off, want_off), (name, "offsets on BXMI_ERANGE", np.nonzero(got_off != want_off)[0][:8])
        hits2.check(0, name + ": hit buffer on BXMI_ERANGE")

        # 3. cap = total exactly, total_host = NULL
        off3 = Guarded((nq + 1) * 8, off_mis)
        hits3 = Guarded(total * 4, hits_mis)
        rc, _ = _find_dev(ix, dq.ptr, de.ptr, nq, off3.ptr, hits3.ptr, total, want_total=False)
        Hip.device_sync()
        assert rc == _ffi().OK, (name, rc)
        raw_off = off3.check((nq + 1) * 8, name + ": offsets, cap = total")
        raw_hits = hits3.check(total * 4, name + ": hits, cap = total")
        assert np.array_equal(off3.payload(raw_off, np.int64, nq + 1), want_off), name
        assert np.array_equal(hits3.payload(raw_hits, np.int32, total), want_hits), name
        # the queries are inputs: untouched, guards included
        for g, a in ((dq, qs), (de, qe)):
            raw = g.check(nq * 4, name + ": queries")
            assert np.array_equal(g.payload(raw, np.int32, nq), a)
    finally:
        reset_opts()


def test_find_dev_empty_batch_writes_offsets0_only(W):
    """nq = 0: offsets[0] = 0, the total 0, nothing else written"""
    ix = make_index(W.s, W.e)
    for off_mis in (0, 8):
        off = Guarded(8, off_mis)
        hits = Guarded(64, 4)
        rc, total = _find_dev(ix, None, None, 0, off.ptr, hits.ptr, 16)
        Hip.device_sync()
        assert rc == _ffi().OK and total == 0
        raw = off.check(8, "offsets of an empty batch")
        assert off.payload(raw, np.int64, 1).tolist() == [0]
        hits.check(0, "hits of an empty batch")


# ------------------------------------------------------- count_dev stages --
# (name, batch, knobs, introspection: (state method, expected first field) or None)
# Which branch of bxmi_ivl_count_dev each row selects: `direct` -- ivl.partition 0: ivl_count_kernel; `bucketed` --
# ivl.bitmap 0: ivl_count_partitioned; the image stages by bm_choose_stage (forced as test_bitmap_pass_differential does and
# read back through the handle's introspection); `sorted_walk` -- a sorted batch on cell images (ivl.sorted_cells: the bs_*
# walk stretch by stretch); `sorted_bucketed` -- a sorted batch with ivl.bitmap 0: ivl_local_count_kernel in the bucketed pass.
NQ_COUNT = 70_001
COUNT_STAGES = [
    ("direct", "count", {"ivl.partition": 0}, None),
    ("bucketed", "count", {"ivl.partition": 1, "ivl.bitmap": 0}, None),
    ("flat_cells", "count", {"ivl.partition": 1, "ivl.flat": 1, "ivl.dense": 1, "ivl.bm_hard_ppm": 10**6}, ("flat_state", 1)),
    ("offset_cells", "count", {"ivl.partition": 1, "ivl.sparse": 1, "ivl.bm_hard_ppm": 10**6}, ("sparse_state", 1)),
    ("dense", "count", {"ivl.partition": 1, "ivl.flat": 0, "ivl.dense": 1}, ("dense_state", 1)),
    ("slices", "count", {"ivl.partition": 1, "ivl.flat": 0, "ivl.dense": 0, "ivl.slice": 1}, ("slice_state", 1)),
    ("sorted_walk", "count_sorted", {"ivl.partition": 1, "ivl.flat": 1, "ivl.dense": 1, "ivl.bm_hard_ppm": 10**6}, ("flat_state", 1)),
    ("sorted_bucketed", "count_sorted", {"ivl.partition": 1, "ivl.bitmap": 0}, None),
]


def _count_batches(W):
    if "count" not in W.batches:
        rng = np.random.default_rng(99)
        W.batches["count"] = _queries(rng, NQ_COUNT)
        W.batches["count_sorted"] = _sorted(*W.batches["count"])
    return W


def _count_dev(ix, qs_ptr, qe_ptr, nq, counts_ptr, total_ptr, stream=None, allow=()):
    return _ffi().call("bxmi_ivl_count_dev", ix._h, qs_ptr, qe_ptr, nq, counts_ptr, total_ptr, stream, allow=allow)


def _preset_total(value=PRESET):
    t = Guarded(8)
    t.fill(np.array([value], dtype=np.int64))
    return t


@pytest.mark.parametrize("name,batch,knobs,state", COUNT_STAGES, ids=[c[0] for c in COUNT_STAGES])
def test_count_dev_accumulates_and_stays_in_bounds(W, name, batch, knobs, state):
    """bxmi_ivl_count_dev on every stage: *total_dev is ACCUMULATED (a preset of 10^12 + 7 comes back plus the oracle's
    total), the counts equal the oracle's, nothing is written past counts[nq) (nq ragged); then total-only (counts = NULL)
    with ivl.tot_walk 0 and 1, accumulated as well."""
    _count_batches(W)
    qs, qe = W.batches[batch]
    nq = len(qs)
    want_c, want_t = W.count(batch)
    ix = make_index(W.s, W.e)
    dq, de = Guarded.holding(qs), Guarded.holding(qe)
    try:
        for k, v in knobs.items():
            set_opt(k, v)
        counts = Guarded(nq * 4)
        total = _preset_total()
        _count_dev(ix, dq.ptr, de.ptr, nq, counts.ptr, total.ptr)
        Hip.device_sync()
        raw = counts.check(nq * 4, name + ": counts")
        got = counts.payload(raw, np.int32, nq)
        bad = np.nonzero(got != want_c)[0]
        assert len(bad) == 0, (name, len(bad), bad[:8], got[bad[:8]], want_c[bad[:8]])
        raw = total.check(8, name + ": total")
        assert int(total.payload(raw, np.int64, 1)[0]) == PRESET + want_t, (name, int(total.payload(raw, np.int64, 1)[0]) - PRESET, want_t)
        if state:
            got_state = getattr(ix, state[0])()
            assert got_state[0] == state[1], (name, state[0], got_state)
        for tot_walk in (1, 0):
            set_opt("ivl.tot_walk", tot_walk)
            total = _preset_total()
            _count_dev(ix, dq.ptr, de.ptr, nq, None, total.ptr)
            _count_dev(ix, dq.ptr, de.ptr, nq, None, total.ptr)  # twice: the second call adds to the first
            Hip.device_sync()
            raw = total.check(8, name + ": total only")
            assert int(total.payload(raw, np.int64, 1)[0]) == PRESET + 2 * want_t, (name, tot_walk)
    finally:
        reset_opts()


def test_count_dev_without_outputs_writes_nothing(W):
    """counts = NULL and total_dev = NULL: BXMI_OK and nothing to compute, on every path (the entry point returns before any
    launch; without that the bucketed and direct paths would be handed two NULL outputs)."""
    _count_batches(W)
    qs, qe = W.batches["count"]
    nq = len(qs)
    ix = make_index(W.s, W.e)
    dq, de = Guarded.holding(qs), Guarded.holding(qe)
    try:
        for knobs in ({"ivl.partition": 0}, {"ivl.partition": 1, "ivl.bitmap": 0}, {"ivl.partition": 1}):
            reset_opts()
            for k, v in knobs.items():
                set_opt(k, v)
            _count_dev(ix, dq.ptr, de.ptr, nq, None, None)
            _ffi().call("bxmi_ivl_count_multi_dev", (C.c_void_p * 1)(ix._h.value), 1, (C.c_void_p * 1)(dq.ptr), (C.c_void_p * 1)(de.ptr),
                        (C.c_int64 * 1)(nq), None, None, None)
            Hip.device_sync()
            for g, a in ((dq, qs), (de, qe)):
                raw = g.check(nq * 4, "queries")
                assert np.array_equal(g.payload(raw, np.int32, nq), a)
    finally:
        reset_opts()


def test_count_multi_dev_accumulates_per_index(O, W):
    """bxmi_ivl_count_multi_dev over indexes on different stages (a sparse index, a dense one, one with reversed targets that
    takes the direct kernel), one with counts[i] = NULL, one with nq[i] = 0: each guarded counts[i] equals the oracle's,
    each preset totals_dev[i] comes back plus the oracle's total; then the same with totals_dev = NULL."""
    rng = np.random.default_rng(5)
    _count_batches(W)
    ds = rng.choice(3_000_000, size=150_000, replace=False)  # dense: one target per 20 coordinates, no start repeated
    de_ = ds + rng.integers(0, 200, size=len(ds))
    ds, de_ = ds.astype(np.int32), de_.astype(np.int32)
    dt = O.OracleIntervalTree()
    dt.insert_many_arrays(ds, de_)
    dq_s = rng.integers(-1000, 3_100_000, size=90_007)
    dense_q = (dq_s.astype(np.int32), (dq_s + rng.integers(-20, 3000, size=len(dq_s))).astype(np.int32))
    members = [
        ("sparse", make_index(W.s, W.e), W.batches["count"], W.count("count"), True),
        ("dense", make_index(ds, de_), dense_q, dt.count_batch(*dense_q), True),
        ("reversed", make_index(W.rs, W.re), W.batches["rev"], W.count("rev"), True),
        ("no_counts", make_index(W.s, W.e), W.batches["count_sorted"], W.count("count_sorted"), False),
        ("empty", make_index(W.s, W.e), (np.zeros(0, np.int32), np.zeros(0, np.int32)), (np.zeros(0, np.int32), 0), True),
    ]
    n = len(members)
    try:
        set_opt("ivl.partition", 1)
        set_opt("ivl.bm_hard_ppm", 10**6)
        for with_totals in (True, False):
            qbufs = [(Guarded.holding(q[0]), Guarded.holding(q[1])) for _, _, q, _, _ in members]
            cbufs = [Guarded(max(len(q[0]), 1) * 4) if want else None for _, _, q, _, want in members]
            tbufs = [_preset_total(PRESET + i) for i in range(n)]
            H = (C.c_void_p * n)(*[m[1]._h.value for m in members])
            Q = (C.c_void_p * n)(*[b[0].ptr for b in qbufs])
            E = (C.c_void_p * n)(*[b[1].ptr for b in qbufs])
            N = (C.c_int64 * n)(*[len(m[2][0]) for m in members])
            K = (C.c_void_p * n)(*[b.ptr if b else None for b in cbufs])
            T = (C.c_void_p * n)(*[b.ptr for b in tbufs]) if with_totals else None
            _ffi().call("bxmi_ivl_count_multi_dev", H, n, Q, E, N, K, T, None)
            Hip.device_sync()
            for i, (name, _, q, (want_c, want_t), want) in enumerate(members):
                nq = len(q[0])
                if cbufs[i] is not None:
                    raw = cbufs[i].check(nq * 4, name + ": counts")
                    got = cbufs[i].payload(raw, np.int32, nq)
                    assert np.array_equal(got, want_c), (name, with_totals, np.nonzero(got != want_c)[0][:8])
                raw = tbufs[i].check(8, name + ": total")
                got_t = int(tbufs[i].payload(raw, np.int64, 1)[0])
                assert got_t == PRESET + i + (want_t if with_totals else 0), (name, with_totals, got_t - PRESET - i, want_t)
        # (the stages that served them: cell images for the dense index, offset cells or key slices for the sparse one)
        assert members[1][1].flat_state()[0] == 1, members[1][1].flat_state()
        assert members[0][1].flat_state()[0] != 1 and (members[0][1].sparse_state()[0] == 1 or members[0][1].slice_state()[0] == 1), \
            (members[0][1].flat_state(), members[0][1].sparse_state(), members[0][1].slice_state())
        assert members[2][1].has_reversed
    finally:
        reset_opts()


@pytest.mark.parametrize("which", ["qs", "qe", "counts"])
def test_count_dev_refuses_unaligned_arrays(W, which):
    """qs, qe or counts not on a 16-byte boundary: BXMI_EINVAL from count_dev and count_multi_dev (bxmi.h), outputs untouched."""
    _count_batches(W)
    qs, qe = W.batches["count"]
    nq = len(qs)
    ix = make_index(W.s, W.e)
    dq = Guarded.holding(qs, 4 if which == "qs" else 0)
    de = Guarded.holding(qe, 4 if which == "qe" else 0)
    counts = Guarded(nq * 4, 4 if which == "counts" else 0)
    total = _preset_total()
    try:
        for knobs in ({"ivl.partition": 0}, {"ivl.partition": 1}):
            reset_opts()
            for k, v in knobs.items():
                set_opt(k, v)
            rc = _count_dev(ix, dq.ptr, de.ptr, nq, counts.ptr, total.ptr, allow=(_ffi().EINVAL,))
            assert rc == _ffi().EINVAL, (which, knobs)
            rc = _ffi().call("bxmi_ivl_count_multi_dev", (C.c_void_p * 1)(ix._h.value), 1, (C.c_void_p * 1)(dq.ptr), (C.c_void_p * 1)(de.ptr),
                             (C.c_int64 * 1)(nq), (C.c_void_p * 1)(counts.ptr), (C.c_void_p * 1)(total.ptr), None, allow=(_ffi().EINVAL,))
            assert rc == _ffi().EINVAL, (which, knobs)
            Hip.device_sync()
            counts.check(0, "counts of a refused call")
            raw = total.check(8, "total of a refused call")
            assert int(total.payload(raw, np.int64, 1)[0]) == PRESET
    finally:
        reset_opts()


# ------------------------------------------------------------ caller stream --
# (family, batch, knobs) -- find_dev and count_dev per family on a fresh handle, so the exchange family's first call is the
# handle's first large batch (unit images built, `stream` waited for once: bxmi.h)
STREAM_FAMILIES = [
    ("direct", "small", {}),
    ("exchange", "unsorted", BIG),
    ("sorted", "sorted", BIG),
]


@pytest.mark.parametrize("family,batch,knobs", STREAM_FAMILIES, ids=[f[0] for f in STREAM_FAMILIES])
def test_stream_ordered_on_a_caller_stream(W, family, batch, knobs):
    """Inputs staged into their final buffers by a copy on the caller's non-blocking stream right before the call, results
    read back on the same stream, only that stream synchronised: every kernel and copy of the call has to be on it."""
    qs, qe = W.batches[batch]
    nq = len(qs)
    want_off, want_hits = W.find(batch)
    want_c, want_t = W.count(batch)
    total_hits = int(want_off[-1])
    ix = make_index(*W.targets(batch))
    src_q, src_e = _ffi().DeviceArray.from_numpy(qs), _ffi().DeviceArray.from_numpy(qe)
    src_t = _ffi().DeviceArray.from_numpy(np.array([PRESET], dtype=np.int64))
    st = Stream()
    try:
        for k, v in knobs.items():
            set_opt(k, v)
        # count first: the handle's first large batch
        dq, de = Guarded(nq * 4), Guarded(nq * 4)
        counts, total = Guarded(nq * 4), Guarded(8)
        st.copy_d2d(dq.ptr, src_q.ptr, nq * 4)
        st.copy_d2d(de.ptr, src_e.ptr, nq * 4)
        st.copy_d2d(total.ptr, src_t.ptr, 8)
        _count_dev(ix, dq.ptr, de.ptr, nq, counts.ptr, total.ptr, stream=st.s)
        got_c = st.read(counts.ptr, np.int32, nq)
        got_t = st.read(total.ptr, np.int64, 1)
        st.sync()
        assert np.array_equal(got_c, want_c), (family, np.nonzero(got_c != want_c)[0][:8])
        assert int(got_t[0]) == PRESET + want_t, (family, int(got_t[0]) - PRESET, want_t)
        # find on fresh query buffers (still sentinel until the stream's copy lands)
        dq2, de2 = Guarded(nq * 4), Guarded(nq * 4)
        off, hits = Guarded((nq + 1) * 8), Guarded(total_hits * 4)
        st.copy_d2d(dq2.ptr, src_q.ptr, nq * 4)
        st.copy_d2d(de2.ptr, src_e.ptr, nq * 4)
        rc, got_total = _find_dev(ix, dq2.ptr, de2.ptr, nq, off.ptr, hits.ptr, total_hits, stream=st.s)
        got_off = st.read(off.ptr, np.int64, nq + 1)
        got_hits = st.read(hits.ptr, np.int32, total_hits)
        st.sync()
        assert rc == _ffi().OK and got_total == total_hits, (family, rc, got_total)
        assert np.array_equal(got_off, want_off), (family, np.nonzero(got_off != want_off)[0][:8])
        bad = np.nonzero(got_hits != want_hits)[0]
        assert len(bad) == 0, (family, len(bad), bad[:8])
        Hip.device_sync()
        off.check((nq + 1) * 8, family + ": offsets")
        hits.check(total_hits * 4, family + ": hits")
        counts.check(nq * 4, family + ": counts")
        if family == "exchange":
            assert ix.slice_state()[0] == 1
    finally:
        st.close()
        reset_opts()


# ------------------------------------------------- append_dev / seal / order_dev --
def _host_find(ix, qs, qe, cap):
    nq = len(qs)
    offsets = np.zeros(nq + 1, dtype=np.int64)
    hits = np.empty(cap, dtype=np.int32)
    total = C.c_int64(0)
    _ffi().call("bxmi_ivl_find", ix._h, qs.ctypes.data, qe.ctypes.data, nq, offsets.ctypes.data, hits.ctypes.data, cap, C.byref(total))
    return offsets, hits[:total.value].copy()


def test_append_dev_seal_and_order_dev(O):
    """One index built four ways -- host append; append_dev from device arrays; host -> device -> host appends re-sealed between
    rounds; append_dev + seal on a non-blocking stream -- gives the same order(), has_reversed, counts and finds, equal to the
    oracle's; the bxmi_ivl_order_dev views satisfy idx == order(), start_dev[i] == starts[idx[i]], end_dev[i] == ends[idx[i]]."""
    from bxmi.intervals import IntervalIndex

    rng = np.random.default_rng(31)
    n = 30_011
    s = rng.integers(-50_000, 2_000_000, size=n)
    e = s + rng.integers(0, 900, size=n)
    flip = rng.random(n) < 0.02
    s, e = np.where(flip, e, s).astype(np.int32), np.where(flip, s, e).astype(np.int32)
    e[:50] = s[:50]  # zero-length
    t = O.OracleIntervalTree()
    t.insert_many_arrays(s, e)
    qs = rng.integers(-60_000, 2_100_000, size=20_001).astype(np.int32)
    qe = (qs + rng.integers(-10, 3000, size=len(qs))).astype(np.int32)
    want_order = t.traverse()
    want_off, want_hits = t.find_batch(qs, qe)
    want_c, want_t = t.count_batch(qs, qe)
    ds, de = _ffi().DeviceArray.from_numpy(s), _ffi().DeviceArray.from_numpy(e)
    cuts = (0, 7_000, 19_000, n)
    builds = {}

    ix = IntervalIndex()
    ix.append(s, e)
    ix.seal()
    builds["host"] = ix

    ix = IntervalIndex()
    ix.append_dev(ds.ptr, de.ptr, n)
    ix.seal()
    builds["device"] = ix

    ix = IntervalIndex()
    for r in range(3):
        a, b = cuts[r], cuts[r + 1]
        if r == 1:
            ix.append_dev(ds.ptr + 4 * a, de.ptr + 4 * a, b - a)
        else:
            ix.append(s[a:b], e[a:b])
        ix.seal()
        t_part = O.OracleIntervalTree()
        t_part.insert_many_arrays(s[:b], e[:b])
        assert np.array_equal(ix.order(), t_part.traverse()), ("interleaved", r)
    builds["interleaved"] = ix

    st = Stream()
    try:
        ix = IntervalIndex()
        sb, eb = Guarded(n * 4), Guarded(n * 4)
        st.copy_d2d(sb.ptr, ds.ptr, n * 4)
        st.copy_d2d(eb.ptr, de.ptr, n * 4)
        ix.append_dev(sb.ptr, eb.ptr, n, stream=st.s)
        ix.seal(stream=st.s)
        builds["stream"] = ix
    finally:
        st.close()

    for name, ix in builds.items():
        assert ix.has_reversed, name  # (2 % of the targets are reversed)
        order = ix.order()
        assert np.array_equal(order, want_order), name
        p_idx, p_s, p_e = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _ffi().call("bxmi_ivl_order_dev", ix._h, C.byref(p_idx), C.byref(p_s), C.byref(p_e))
        idx = dev_read(p_idx.value, np.int32, n)
        assert np.array_equal(idx, order), name
        assert np.array_equal(dev_read(p_s.value, np.int32, n), s[idx]), name
        assert np.array_equal(dev_read(p_e.value, np.int32, n), e[idx]), name
        c, tot = ix.count(qs, qe)
        assert np.array_equal(c, want_c) and tot == want_t, name
        off, hits = _host_find(ix, qs, qe, len(want_hits) + 16)
        assert np.array_equal(off, want_off) and np.array_equal(hits, want_hits), name
