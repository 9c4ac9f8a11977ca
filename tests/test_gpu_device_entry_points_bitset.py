"""
The device-pointer entry points of the binned bitset (include/bxmi.h, `_dev`) against the oracle (oracle/binbits.c):
ranges from device arrays, a guarded result array, ACCUMULATED counts, lazily allocated operands of different capacity, and
a chain of calls on a caller's non-blocking stream.

The host forms stage through the set's own scratch, synchronise its own stream and zero the accumulator first, so a count
that is stored instead of added, a result written past out[n) or a kernel queued on another stream than the caller's would
pass them.  (No torch: see tests/conftest.py:has_gpu.)
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# every _dev entry point of the bitset this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_bits_set_ranges_dev", "bxmi_bits_count_ranges_dev", "bxmi_bits_words_dev", "bxmi_bits_and_dev", "bxmi_bits_or_dev",
                    "bxmi_bits_and_count_dev", "bxmi_bits_popcount_dev", "bxmi_bits_group_and_dev", "bxmi_bits_group_or_dev",
                    "bxmi_bits_group_popcount_dev")

G = 256
SENT = 0xA5
PRESET = 10**12 + 7
BITS_WIDE_BELOW_BITS = (1 << 21) * 128  # csrc/bitset.hip BITS_WIDE_BELOW (16-byte pairs) in bits: above it the counting kernels run 256 threads


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def _ffi():
    from bxmi import _ffi

    return _ffi


def set_opt(key, value):
    _ffi().call("bxmi_set_option", key.encode(), int(value))


DEFAULT_OPTS = _ffi().options()


def reset_opts():
    for k, v in DEFAULT_OPTS.items():
        set_opt(k, v)


# ---------------------------------------------------------------- helpers --
# (the same small helpers as tests/test_gpu_device_entry_points.py; test modules do not import each other)
class Hip:
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


class Stream:
    def __init__(self):
        s = C.c_void_p()
        Hip.check(Hip.lib().hipStreamCreateWithFlags(C.byref(s), 1), "hipStreamCreateWithFlags")
        self.s = s.value

    def copy_d2d(self, dst, src, nbytes):
        if nbytes:
            Hip.check(Hip.lib().hipMemcpyAsync(dst, src, nbytes, 3, self.s), "hipMemcpyAsync D2D")

    def read(self, src, dtype, count):
        out = np.empty(count, dtype=dtype)
        if count:
            Hip.check(Hip.lib().hipMemcpyAsync(out.ctypes.data, src, out.nbytes, 2, self.s), "hipMemcpyAsync D2H")
        return out

    def sync(self):
        Hip.check(Hip.lib().hipStreamSynchronize(self.s), "hipStreamSynchronize")

    def close(self):
        if self.s:
            Hip.check(Hip.lib().hipStreamDestroy(self.s), "hipStreamDestroy")
            self.s = None


class Guarded:
    def __init__(self, nbytes, mis=0):
        self.nbytes, self.mis = int(nbytes), mis
        self.total = self.nbytes + 2 * G + 16
        self.buf = _ffi().DeviceArray(self.total)
        _ffi().call("bxmi_memset", self.buf.ptr, SENT, self.total)
        _ffi().call("bxmi_synchronize", None)
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
        _ffi().call("bxmi_memcpy_h2d", self.ptr, arr.ctypes.data, arr.nbytes)

    def read(self, written, dtype, what):
        """the payload [ptr, ptr + written) as dtype, after checking that every byte around it holds the sentinel"""
        raw = np.empty(self.total, dtype=np.uint8)
        _ffi().call("bxmi_memcpy_d2h", raw.ctypes.data, self.buf.ptr, self.total)
        lo, hi = G + self.mis, G + self.mis + int(written)
        bad = np.nonzero(raw[:lo] != SENT)[0]
        assert len(bad) == 0, ("%s: %d guard bytes before the buffer written" % (what, len(bad)), bad[:8] - lo)
        bad = np.nonzero(raw[hi:] != SENT)[0]
        assert len(bad) == 0, ("%s: %d bytes past the written region changed" % (what, len(bad)), bad[:8])
        return raw[lo:hi].view(dtype).copy()


def preset(values):
    g = Guarded(8 * len(values))
    g.fill(np.asarray(values, dtype=np.int64))
    return g


def new_pair(O, size, gran):
    from bxmi.bitset import DeviceBitSet

    return DeviceBitSet(size, gran), O.OracleBinnedBitSet(size, gran)


def random_ranges(rng, size, m, lo=0, hi=None, maxlen=None):
    hi = size if hi is None else hi
    s = rng.integers(lo, hi, size=m)
    n = rng.integers(0, maxlen or max(2, (hi - lo) // 20), size=m)
    n = np.minimum(n, size - s)
    s[:3] = [lo, hi - 1, max(lo, hi - 70)]  # the edges of the stretch
    n[:3] = [min(65, size - lo), 1, min(70, size - max(lo, hi - 70))]
    return s.astype(np.int32), n.astype(np.int32)


def raw_bits(d):
    """the raw view of bxmi_bits_words_dev: bit p at word p >> 6, bit p & 63"""
    p, nw = C.c_void_p(), C.c_int64(0)
    _ffi().call("bxmi_bits_words_dev", d._h, C.byref(p), C.byref(nw))
    w = np.empty(nw.value, dtype=np.uint64)
    _ffi().call("bxmi_memcpy_d2h", w.ctypes.data, p.value, nw.value * 8)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[: d.size]


def set_ranges_dev(d, s, n, stream=None):
    ds, dn = Guarded.holding(s), Guarded.holding(n)
    _ffi().call("bxmi_bits_set_ranges_dev", d._h, ds.ptr, dn.ptr, len(s), stream)
    return ds, dn  # (alive until the caller has synchronised)


def count_ranges_dev(d, s, n, what):
    ds, dn = Guarded.holding(s), Guarded.holding(n)
    out = Guarded(len(s) * 4)
    _ffi().call("bxmi_bits_count_ranges_dev", d._h, ds.ptr, dn.ptr, len(s), out.ptr, None)
    Hip.device_sync()
    return out.read(len(s) * 4, np.int32, what)


# ------------------------------------------------------ ranges from device --
@pytest.mark.parametrize("gran", [1, 7, 1024])
@pytest.mark.parametrize("size", [1_000_003, 77_777])
def test_set_and_count_ranges_dev(O, size, gran):
    """bxmi_bits_set_ranges_dev + bxmi_bits_count_ranges_dev on a fresh set (no words yet: the whole array is grown for ranges
    whose extent the host does not know), on a set grown part way by the host form, and after invert (ALL_ONE tags: the
    reference's start % bin_size arithmetic); results in a guarded array at a ragged n."""
    rng = np.random.default_rng(size + gran)
    try:
        for grid in (3, 0):  # (3: a grid-stride loop over the ranges; 0: the default grid)
            set_opt("bits.grid", grid)
            # fresh: the first bits arrive through the device form
            d, o = new_pair(O, size, gran)
            s, n = random_ranges(rng, size, 2001)
            keep = set_ranges_dev(d, s, n)
            Hip.device_sync()
            o.set_ranges(s, n)
            cs, cn = random_ranges(rng, size, 3003, maxlen=size // 3)
            assert np.array_equal(count_ranges_dev(d, cs, cn, "fresh"), o.count_ranges(cs, cn)), (size, gran, grid, "fresh")
            # grown part way: the host form allocates words up to its ranges only, then device ranges reach the rest
            d, o = new_pair(O, size, gran)
            s, n = random_ranges(rng, size, 500, hi=size // 5, maxlen=3000)
            d.set_ranges(s, n), o.set_ranges(s, n)
            s, n = random_ranges(rng, size, 1001, lo=size // 2)
            keep = set_ranges_dev(d, s, n)
            Hip.device_sync()
            o.set_ranges(s, n)
            assert np.array_equal(count_ranges_dev(d, cs, cn, "grown"), o.count_ranges(cs, cn)), (size, gran, grid, "grown")
            # inverted: ALL_ONE bins, then more ranges on top of them
            d.invert(), o.invert()
            s, n = random_ranges(rng, size, 301)
            keep = set_ranges_dev(d, s, n)
            Hip.device_sync()
            o.set_ranges(s, n)
            del keep
            got = count_ranges_dev(d, cs, cn, "inverted")
            want = o.count_ranges(cs, cn)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (size, gran, grid, "inverted", bad[:8], cs[bad[:8]], cn[bad[:8]], got[bad[:8]], want[bad[:8]])
            assert d.bin_states().tolist() == o.states().tolist()
            assert np.array_equal(raw_bits(d), o.unpack())
    finally:
        reset_opts()


# ------------------------------------------------------- accumulated counts --
def _fill(rng, d, o, hi, m=300, maxlen=5000):
    s, n = random_ranges(rng, d.size, m, hi=hi, maxlen=maxlen)
    d.set_ranges(s, n), o.set_ranges(s, n)


def test_popcount_and_and_count_dev_accumulate(O):
    """bxmi_bits_popcount_dev / bxmi_bits_and_count_dev add to a preset count; operands lazily allocated to different
    capacities in both orders (AND on the larger one: the memset branch of bits_binary; OR on the smaller one: the grow
    branch); afterwards bits, bin states and the raw word view equal the oracle's."""
    rng = np.random.default_rng(8)
    size, gran = 5_000_011, 1024
    a, oa = new_pair(O, size, gran)
    b, ob = new_pair(O, size, gran)
    c, oc = new_pair(O, size, gran)
    e, oe = new_pair(O, size, gran)
    _fill(rng, a, oa, size)             # a: words up to the end
    _fill(rng, b, ob, size // 7)        # b: a seventh of them
    _fill(rng, c, oc, size // 9)        # c: fewer still
    _fill(rng, e, oe, size)
    cnt = preset([PRESET, PRESET + 1, PRESET + 2])
    _ffi().call("bxmi_bits_popcount_dev", a._h, cnt.ptr, None)
    _ffi().call("bxmi_bits_popcount_dev", b._h, cnt.ptr + 8, None)
    _ffi().call("bxmi_bits_popcount_dev", b._h, cnt.ptr + 8, None)  # twice: adds twice
    Hip.device_sync()
    got = cnt.read(24, np.int64, "popcount_dev")
    assert got.tolist() == [PRESET + int(oa.unpack().sum()), PRESET + 1 + 2 * int(ob.unpack().sum()), PRESET + 2]
    # AND on the larger operand (a) with the smaller (b): a's words past b's are zeroed
    cnt = preset([PRESET])
    _ffi().call("bxmi_bits_and_count_dev", a._h, b._h, cnt.ptr, None)
    Hip.device_sync()
    oa.iand(ob)
    assert int(cnt.read(8, np.int64, "and_count_dev")[0]) == PRESET + int(oa.unpack().sum())
    # AND on the smaller operand (c) with the larger (e)
    cnt = preset([PRESET])
    _ffi().call("bxmi_bits_and_count_dev", c._h, e._h, cnt.ptr, None)
    Hip.device_sync()
    oc.iand(oe)
    assert int(cnt.read(8, np.int64, "and_count_dev, smaller first")[0]) == PRESET + int(oc.unpack().sum())
    # OR on the smaller operand (b) with the larger (e): b grows first; and_dev / or_dev without counts
    f, of = new_pair(O, size, gran)
    _fill(rng, f, of, size // 3)
    _ffi().call("bxmi_bits_or_dev", b._h, e._h, None)
    _ffi().call("bxmi_bits_and_dev", f._h, e._h, None)
    Hip.device_sync()
    ob.ior(oe), of.iand(oe)
    for name, d, o in (("a", a, oa), ("b", b, ob), ("c", c, oc), ("f", f, of)):
        assert d.bin_states().tolist() == o.states().tolist(), name
        assert np.array_equal(raw_bits(d), o.unpack()), name


def test_group_dev_forms_accumulate(O):
    """bxmi_bits_group_popcount_dev / bxmi_bits_group_and_dev add to preset per-member counts; one member above BITS_WIDE_BELOW
    pairs (the 256-thread kernels) and the others below it, an inverted member (ALL_ONE tags), sizes off every word boundary;
    group_or_dev afterwards; bits and bin states equal the oracle's."""
    from bxmi.bitset import BitSetGroup

    rng = np.random.default_rng(12)
    sizes = [(BITS_WIDE_BELOW_BITS + 4_000_037, 1024), (3_000_001, 7), (100_003, 1), (65, 1024)]
    A = [new_pair(O, s, g) for s, g in sizes]
    B = [new_pair(O, s, g) for s, g in sizes]
    for pairs in (A, B):
        for d, o in pairs:
            hi = d.size if d.size < 10**7 else 20_000_000  # (the wide member: bits in its first 20 M only, no unpack needed)
            s, n = random_ranges(rng, d.size, 200, hi=hi, maxlen=max(2, min(hi // 10, 50_000)))
            d.set_ranges(s, n), o.set_ranges(s, n)
    B[1][0].invert(), B[1][1].invert()
    k = len(sizes)

    def popcounts(pairs):
        return [o.count_range(0, o.size) if o.size > 10**7 else int(o.unpack().sum()) for _, o in pairs]

    # the single-set counting kernels on the wide member (256 threads) before the groups take over
    wide, owide = new_pair(O, sizes[0][0], 1024)
    s, n = random_ranges(rng, wide.size, 200, hi=30_000_000, maxlen=50_000)
    wide.set_ranges(s, n), owide.set_ranges(s, n)
    cnt = preset([PRESET, PRESET])
    _ffi().call("bxmi_bits_popcount_dev", A[0][0]._h, cnt.ptr, None)
    _ffi().call("bxmi_bits_and_count_dev", wide._h, A[0][0]._h, cnt.ptr + 8, None)
    Hip.device_sync()
    owide.iand(A[0][1])
    assert cnt.read(16, np.int64, "wide popcount_dev / and_count_dev").tolist() == [PRESET + A[0][1].count_range(0, sizes[0][0]),
                                                                                    PRESET + owide.count_range(0, sizes[0][0])]
    del wide, owide
    ga, gb = BitSetGroup([d for d, _ in A]), BitSetGroup([d for d, _ in B])
    cnt = preset([PRESET + i for i in range(k)])
    _ffi().call("bxmi_bits_group_popcount_dev", ga._g, cnt.ptr, None)
    Hip.device_sync()
    want = popcounts(A)
    assert cnt.read(8 * k, np.int64, "group_popcount_dev").tolist() == [PRESET + i + w for i, w in enumerate(want)]
    cnt = preset([PRESET + 10 * i for i in range(k)])
    _ffi().call("bxmi_bits_group_and_dev", ga._g, gb._g, cnt.ptr, None)
    Hip.device_sync()
    for (_, oa), (_, ob) in zip(A, B):
        oa.iand(ob)
    want = popcounts(A)
    assert cnt.read(8 * k, np.int64, "group_and_dev").tolist() == [PRESET + 10 * i + w for i, w in enumerate(want)]
    _ffi().call("bxmi_bits_group_or_dev", ga._g, gb._g, None)
    Hip.device_sync()
    for (_, oa), (_, ob) in zip(A, B):
        oa.ior(ob)
    for i, (d, o) in enumerate(A):
        assert d.bin_states().tolist() == o.states().tolist(), i
        if d.size < 10**7:
            assert np.array_equal(raw_bits(d), o.unpack()), i
        else:
            assert d.count_range(0, d.size) == o.count_range(0, o.size), i
    ga.close(), gb.close()


# ------------------------------------------------------------ caller stream --
def test_chain_on_a_caller_stream(O):
    """set_ranges_dev -> count_ranges_dev -> and_count_dev on one non-blocking stream, the ranges staged into their final
    buffers by copies on that stream, the results read back on it, one synchronisation at the end."""
    rng = np.random.default_rng(41)
    size, gran = 2_000_003, 7
    a, oa = new_pair(O, size, gran)
    b, ob = new_pair(O, size, gran)
    _fill(rng, b, ob, size)
    s, n = random_ranges(rng, size, 4001)
    cs, cn = random_ranges(rng, size, 2003, maxlen=size // 4)
    src = [_ffi().DeviceArray.from_numpy(x) for x in (s, n, cs, cn, np.array([PRESET], dtype=np.int64))]
    dst = [Guarded(x.nbytes) for x in src]
    out = Guarded(len(cs) * 4)
    oa.set_ranges(s, n)
    want_counts = oa.count_ranges(cs, cn)
    oa.iand(ob)
    want_and = int(oa.unpack().sum())
    st = Stream()
    try:
        for d_, s_ in zip(dst, src):
            st.copy_d2d(d_.ptr, s_.ptr, s_.nbytes)
        _ffi().call("bxmi_bits_set_ranges_dev", a._h, dst[0].ptr, dst[1].ptr, len(s), st.s)
        _ffi().call("bxmi_bits_count_ranges_dev", a._h, dst[2].ptr, dst[3].ptr, len(cs), out.ptr, st.s)
        _ffi().call("bxmi_bits_and_count_dev", a._h, b._h, dst[4].ptr, st.s)
        got_counts = st.read(out.ptr, np.int32, len(cs))
        got_and = st.read(dst[4].ptr, np.int64, 1)
        st.sync()
    finally:
        st.close()
    bad = np.nonzero(got_counts != want_counts)[0]
    assert len(bad) == 0, (bad[:8], got_counts[bad[:8]], want_counts[bad[:8]])
    assert int(got_and[0]) == PRESET + want_and
    Hip.device_sync()
    out.read(len(cs) * 4, np.int32, "count_ranges_dev on a stream")
    assert np.array_equal(raw_bits(a), oa.unpack())
