"""
Seeded 2bit sequences and rows, and two models that scale, for tests/test_twobit_kernel_host.py and tests/test_gpu_twobit.py (a
helper: no tests here, no GPU).  tests/test_twobit_cases.py pins both models to the whole-sequence ones of tests/twobit_model.py
and checks the conditions that keep the tests on these cases from passing vacuously.

  random_sequence   random packed bytes (the padding bits of the last byte stay random) under sorted, disjoint N and mask blocks
                    that carry every edge the kernels treat differently (edges_of); asserted on what was generated
  window            the letters of [a, b) from the packed bytes of [a, b) alone and the blocks np.searchsorted finds: nothing of
                    the size of the sequence is built, so it answers a window of a sequence of 2^31 - 1 bases
  composition       the base counts of rows from running counts (np.cumsum, int64) of the six indicator arrays of the whole
                    sequence's letters: no checkpoints, no block tables
"""
import numpy as np

import twobit_model as M
from twobit_model import CHUNK, CKPT, TILE

EDGE_SIZE = 4 * TILE  # a random sequence of at least this many bases carries every edge of edges_of
SCAN_TILE = 2048      # of csrc/primitives.hpp: entries of a running table per workgroup of the device scan
TB_SLAB = 1 << 26     # of csrc/sequence.hip: output bytes per slab of bxmi_twobit_bases
TB_COMP_SLAB = 1 << 22  # rows per slab of bxmi_twobit_composition


def sequence_of(size, n_starts, n_sizes, m_starts, m_sizes, packed):
    from bxmi import twobit

    i64 = [np.asarray(a, dtype=np.int64) for a in (n_starts, n_sizes, m_starts, m_sizes)]
    return twobit.Sequence(int(size), *i64, np.asarray(packed, dtype=np.uint8))


# ---- the sequence generator ----
def log_uniform(rng, lo, hi, n):
    """n integers in [lo, hi], their logarithms uniform"""
    return np.clip(np.exp(rng.uniform(np.log(lo), np.log(hi + 1), n)).astype(np.int64), lo, hi)


def random_blocks(rng, size, blocks, longest):
    """(starts, sizes) int64 of at most `blocks` sorted, disjoint, non-empty blocks inside [0, size): a fifth of them of one base,
    the others log-uniform up to `longest` (a few of them `longest`), four gaps in ten empty (runs of adjacent blocks), the first
    block at 0, the last one ending at `size`, and, where the list has room between its first and last block, blocks that start
    and blocks that end on multiples of 16, 1024 and 4096"""
    n = int(min(blocks, (size + 1) // 2))
    if n <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    longest = int(max(1, min(longest, size // 4)))
    sizes = log_uniform(rng, 1, longest, n)
    sizes[rng.random(n) < 0.2] = 1
    pinned = np.zeros(n, dtype=bool)
    pinned[rng.integers(0, n, max(n // 50, 2))] = True
    if pinned.sum() * longest > size // 2:
        pinned[np.flatnonzero(pinned)[2:]] = False  # (at most half the sequence: `longest` is at most a quarter of it)
    sizes[pinned] = longest
    budget = max(n, size * 6 // 10)
    while sizes.sum() > budget and (sizes[~pinned] > 1).any():
        sizes[~pinned] = np.maximum(sizes[~pinned] // 2, 1)
    while sizes.sum() > size:  # (more blocks asked for than longest ones fit)
        sizes = np.maximum(sizes // 2, 1)
    slack = int(size - sizes.sum())
    open_gap = rng.random(n + 1) >= 0.4
    open_gap[0] = open_gap[n] = False
    if n == 1:
        open_gap[1] = True  # (one block: it starts at 0)
    elif not open_gap.any():
        open_gap[n // 2] = True
    gaps = np.zeros(n + 1, dtype=np.int64)
    gaps[open_gap] = rng.multinomial(slack, np.full(int(open_gap.sum()), 1.0 / open_gap.sum()))
    starts = np.cumsum(gaps[:n] + np.concatenate([[0], sizes[:-1]]))
    ends = starts + sizes
    # blocks that start / end on multiples: a multiple m between the first block's end and the last one's start becomes the end
    # of the block it lies in (cut there) or of the block before it (moved there), another the start of the block it lies in or
    # of the block after it.  No block grows, the first one's start and the last one's end stay, and so does the order.
    for unit in (16, 1024, 4096):
        lo, hi = int(ends[0]) // unit + 1, (int(starts[-1]) - 1) // unit
        if n < 4 or hi < lo:
            continue
        for kind in ("end", "start") * 4:
            m = int(rng.integers(lo, hi + 1)) * unit
            i = int(np.searchsorted(ends, m, side="right"))  # the first block that ends after m: 1 <= i <= n - 1, starts[i] != m or i < n - 1
            if starts[i] < m:  # m inside block i, which is neither the first nor the last
                if pinned[i]:
                    continue  # (the longest blocks stay whole)
                if kind == "end":
                    ends[i] = m
                else:
                    starts[i] = m
            elif kind == "end" and i - 1 > 0:
                starts[i - 1] += m - ends[i - 1]
                ends[i - 1] = m
            elif kind == "start" and i < n - 1:
                ends[i] -= starts[i] - m
                starts[i] = m
    sizes = ends - starts
    assert (sizes >= 1).all() and starts[0] >= 0 and ends[-1] <= size and (starts[1:] >= ends[:-1]).all()
    return starts, sizes


def edges_of(seq):
    """{edge: whether the blocks of `seq` have it}: what random_sequence guarantees from EDGE_SIZE bases on"""
    out = {}
    lists = {"N": (seq.n_starts, seq.n_sizes), "mask": (seq.m_starts, seq.m_sizes)}
    for name, (starts, sizes) in lists.items():
        starts, sizes = np.asarray(starts, dtype=np.int64), np.asarray(sizes, dtype=np.int64)
        ends = starts + sizes
        adjacent = starts[1:] == ends[:-1]
        out[name + ": one-base blocks"] = bool((sizes == 1).any())
        out[name + ": a run of three adjacent blocks"] = bool((adjacent[1:] & adjacent[:-1]).any())
        out[name + ": adjacent one-base blocks"] = bool((adjacent & (sizes[1:] == 1) & (sizes[:-1] == 1)).any())
        for unit in (16, 1024, 4096):
            out["%s: a block starts on a multiple of %d" % (name, unit)] = bool(((starts % unit == 0) & (starts > 0)).any())
            out["%s: a block ends on a multiple of %d" % (name, unit)] = bool(((ends % unit == 0) & (ends < seq.size)).any())
        out[name + ": a block ends at size"] = bool(len(ends) and ends[-1] == seq.size)
        out[name + ": a block starts at 0"] = bool(len(starts) and starts[0] == 0)
        out[name + ": a block longer than two checkpoint blocks"] = bool((sizes > 2 * CKPT).any())
    out["an N and a mask block partly overlap"] = partly_overlapping(seq)
    return out


def partly_overlapping(seq):
    """an N block begins inside a mask block and ends outside it, and a mask block does so in an N block"""
    n0, m0 = np.asarray(seq.n_starts, dtype=np.int64), np.asarray(seq.m_starts, dtype=np.int64)
    n1, m1 = n0 + np.asarray(seq.n_sizes, dtype=np.int64), m0 + np.asarray(seq.m_sizes, dtype=np.int64)
    if not len(n0) or not len(m0):
        return False

    def begins_inside(a0, a1, b0, b1):  # some [a0, a1) begins strictly inside a [b0, b1) and ends beyond it
        j = np.searchsorted(b0, a0, side="left") - 1  # the last b that starts before a
        ok = j >= 0
        j = np.maximum(j, 0)
        return bool((ok & (b0[j] < a0) & (a0 < b1[j]) & (b1[j] < a1)).any())

    return begins_inside(n0, n1, m0, m1) and begins_inside(m0, m1, n0, n1)


def random_sequence(rng, size, n_blocks, m_blocks, n_longest=3000, m_longest=3000):
    """a bxmi.twobit.Sequence of `size` bases: random packed bytes, at most n_blocks N blocks of up to n_longest bases and m_blocks
    mask blocks of up to m_longest (random_blocks).  From EDGE_SIZE bases on -- with at least 16 blocks per list and blocks of
    more than two checkpoint blocks where the list's longest allows them -- every edge of edges_of is there, or this raises."""
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    longest = {"N": n_longest, "mask": m_longest}
    for _ in range(20):
        n = random_blocks(rng, size, n_blocks, n_longest)
        m = random_blocks(rng, size, m_blocks, m_longest)
        seq = sequence_of(size, n[0], n[1], m[0], m[1], packed)
        missing = [k for k, v in edges_of(seq).items() if not v and not (k.endswith("checkpoint blocks") and longest[k.split(":")[0]] <= 2 * CKPT)]
        if size < EDGE_SIZE or not missing:
            break
    assert size < EDGE_SIZE or not missing, missing
    return seq


# ---- the letters of a window ----
_blocks_of = {}


def blocks_of(seq):
    """(n_starts, n_ends, m_starts, m_ends) int64 of a sequence, made once"""
    key = id(seq)
    if key not in _blocks_of or _blocks_of[key][0] is not seq:
        n0, m0 = np.asarray(seq.n_starts, dtype=np.int64), np.asarray(seq.m_starts, dtype=np.int64)
        _blocks_of[key] = (seq, (n0, n0 + np.asarray(seq.n_sizes, dtype=np.int64), m0, m0 + np.asarray(seq.m_sizes, dtype=np.int64)))
    return _blocks_of[key][1]


def covered_window(starts, ends, a, b):
    """bool[b - a]: the positions of [a, b) inside a block of a sorted disjoint list"""
    i0, i1 = np.searchsorted(ends, a, side="right"), np.searchsorted(starts, b, side="left")  # the blocks that meet [a, b)
    step = np.zeros(b - a + 1, dtype=np.int64)
    np.add.at(step, np.maximum(starts[i0:i1], a) - a, 1)
    np.add.at(step, np.minimum(ends[i0:i1], b) - a, -1)
    return np.cumsum(step)[:-1] > 0


def window(seq, a, b, do_mask=True):
    """uint8[b - a]: the letters of [a, b), 0 <= a <= b <= size"""
    assert 0 <= a <= b <= seq.size
    if a == b:
        return np.zeros(0, dtype=np.uint8)
    first = a // 4
    p = np.asarray(seq.packed[first:(b + 3) // 4], dtype=np.uint8)
    codes = np.stack([(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3], axis=1).reshape(-1)[a - 4 * first:b - 4 * first]
    n0, n1, m0, m1 = blocks_of(seq)
    out = M.LETTERS[codes]
    out[covered_window(n0, n1, a, b)] = ord("N")
    if do_mask:
        out[covered_window(m0, m1, a, b)] |= 0x20
    return out


def window_row(seqs, t, start, length, do_mask=True, pad=ord("N")):
    """M.Letters.row from windows: positions [start, start + length) of sequence t, `pad` outside it or when t names none"""
    out = np.full(length, pad, dtype=np.uint8)
    if 0 <= t < len(seqs):
        lo, hi = max(start, 0), min(start + length, seqs[t].size)
        if lo < hi:
            out[lo - start:hi - start] = window(seqs[t], lo, hi, do_mask)
    return out


def window_bases(seqs, track_of, starts, lengths, do_mask=True, pad=ord("N")):
    """the contract of bxmi_twobit_bases from windows: uint8[sum of lengths]"""
    rows = [window_row(seqs, int(t), int(s), int(n), do_mask, pad) for t, s, n in zip(track_of, starts, lengths)]
    return np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint8)


# ---- base counts from running counts ----
def composition(whole, starts, ends):
    """int32 [n, 6] = A, C, G, T, N, lower case of rows [starts[i], ends[i]) clipped to the sequence whose letters are `whole`
    (twobit_model.letters): differences of np.cumsum over each of the six indicator arrays, in int64, one array at a time"""
    size = len(whole)
    s = np.clip(np.asarray(starts, dtype=np.int64), 0, size)
    e = np.clip(np.asarray(ends, dtype=np.int64), 0, size)
    e = np.maximum(e, s)  # (a reversed row is empty)
    out = np.zeros((len(s), 6), dtype=np.int32)
    upper = whole & ~np.uint8(0x20)
    running = np.zeros(size + 1, dtype=np.int64)
    for k, indicator in enumerate([upper == ord(c) for c in "ACGTN"] + [whole >= ord("a")]):
        np.cumsum(indicator.view(np.int8), dtype=np.int64, out=running[1:])  # (the view: numpy sums int8 far faster than bool)
        out[:, k] = running[e] - running[s]
    return out


def composition_of(seqs, track_of, starts, ends, do_mask=True):
    """the contract of bxmi_twobit_composition over several sequences; a row that names none is zeros"""
    track_of, starts, ends = (np.asarray(a, dtype=np.int64) for a in (track_of, starts, ends))
    out = np.zeros((len(track_of), 6), dtype=np.int32)
    for t, seq in enumerate(seqs):
        rows = np.flatnonzero(track_of == t)
        if len(rows):
            out[rows] = composition(M.letters(seq, do_mask), starts[rows], ends[rows])
    return out


def counts_of_letters(text):
    """A, C, G, T, N, lower case of a uint8 array of letters, by counting"""
    upper = [np.count_nonzero(text == ord(c)) for c in "ACGTN"]
    lower = [np.count_nonzero(text == ord(c)) for c in "acgtn"]
    assert sum(upper) + sum(lower) == len(text)  # (no other byte)
    return [a + b for a, b in zip(upper, lower)] + [sum(lower)]


# ---- seeded cases of the kernel-on-host program and of the device ----
RANDOM_SEEDS = (301, 302, 303)
RANDOM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4096, 4099, 16385)
RANDOM_WIDTHS = (1, 37, TILE + 1)
_cases = {}


def random_case(seed):
    """Four random sequences -- three sizes of RANDOM_SIZES and one of EDGE_SIZE .. 40 000 bases, which has every edge of edges_of --
    and, made once per seed and never changed:
      track_of, starts, lengths   ragged rows of 0 .. 3 TILE bases (log-uniform: the host program walks every byte with a
                                  workgroup of threads), a fifth of them of 0 .. 2, from -50 to size + 50, track -1 among them,
                                  one row of 3 TILE bases
      matrix[width]               (track_of, starts): the first rows of the same as windows of RANDOM_WIDTHS, fewer the wider
      comp                        (track_of, starts, ends): the ragged rows and 200 arbitrary pairs, reversed and empty among them
    """
    if seed in _cases:
        return _cases[seed]
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.choice(RANDOM_SIZES, 3, replace=False)] + [int(rng.integers(EDGE_SIZE, 40001))]
    seqs = [random_sequence(rng, size, max(size // 400, 3), max(size // 150, 3), n_longest=2600, m_longest=2600) for size in sizes]
    assert all(edges_of(seqs[3]).values())
    n = 240
    track_of = rng.integers(0, 4, n)
    track_of[rng.random(n) < 0.5] = 3  # (half the rows on the sequence that has room for them)
    track_of[rng.integers(0, n, 6)] = -1
    track_of[7] = 3
    size_of = np.array(sizes + [0])[track_of]
    starts = rng.integers(-50, size_of + 51)
    lengths = log_uniform(rng, 1, 3 * TILE + 1, n) - 1
    short = rng.random(n) < 0.2
    lengths[short] = rng.integers(0, 3, int(short.sum()))
    starts[7], lengths[7] = sizes[3] // 3, 3 * TILE
    lengths[11] = 0
    assert lengths.min() == 0 and lengths.max() == 3 * TILE and (lengths <= 2).sum() >= n // 8 and starts.min() < 0
    assert ((starts + lengths > size_of) & (track_of >= 0)).any() and (track_of == -1).any()
    matrix = {1: (track_of, starts), 37: (track_of[:120], starts[:120]), TILE + 1: (track_of[:24], starts[:24])}
    assert set(matrix) == set(RANDOM_WIDTHS)
    more = 200
    t2 = rng.integers(-1, 4, more)
    size2 = np.array(sizes + [0])[t2]
    s2, e2 = rng.integers(-50, size2 + 51), rng.integers(-50, size2 + 51)
    e2[:40] = s2[:40]
    assert (s2 > e2).any() and (s2 == e2).any() and (s2 < e2).any()
    comp = (np.concatenate([track_of, t2]), np.concatenate([starts, s2]), np.concatenate([starts + lengths, e2]))
    case = dict(seqs=seqs, track_of=track_of, starts=starts, lengths=lengths, matrix=matrix, comp=comp)
    for a in (track_of, starts, lengths) + comp:
        a.setflags(write=False)
    _cases[seed] = case
    return case


def check_random_case(seed, bases, counts):
    """random_case(seed) through `bases(seqs, track_of, starts, do_mask, pad, width=0, lengths=None)` -> uint8[total] and
    `counts(seqs, track_of, starts, ends, do_mask)` -> int32 [n, 6], against the whole-sequence model: the ragged rows, their base
    counts and every width, each with do_mask on and with it off"""
    case = random_case(seed)
    seqs, model = case["seqs"], M.Letters(case["seqs"])
    track_of, starts, lengths = case["track_of"], case["starts"], case["lengths"]
    for do_mask, pad in ((True, ord("N")), (False, ord("."))):
        want, _ = model.bases(track_of, starts, lengths, do_mask, pad)
        assert np.array_equal(bases(seqs, track_of, starts, do_mask, pad, lengths=lengths), want), (seed, do_mask, "ragged")
        t, s, e = case["comp"]
        want = model.composition(t, s, e, do_mask)
        assert want[:, :5].any(axis=0).all() and want[:, 5].any() == do_mask
        assert np.array_equal(counts(seqs, t, s, e, do_mask), want), (seed, do_mask, "composition")
        for width in RANDOM_WIDTHS:
            t, s = case["matrix"][width]
            want = model.matrix(t, s, width, do_mask, ord("-"))
            got = bases(seqs, t, s, do_mask, ord("-"), width=width)
            assert np.array_equal(got.reshape(-1, width), want), (seed, do_mask, width)


STRETCH_N = (2003, 1500)   # one-base N blocks at 2003, 2005, ...: through a tile boundary and two checkpoints
STRETCH_M = (7601, 1200)   # adjacent one-base mask blocks [7601, 8801): through a tile boundary


def segments_of(offsets):
    """(row, first byte, past byte) of every row segment of every tile of a ragged output, as tb_bases_kernel walks them"""
    out = []
    for r in range(len(offsets) - 1):
        a, b = int(offsets[r]), int(offsets[r + 1])
        while a < b:
            cut = min(b, (a // TILE + 1) * TILE)
            out.append((r, a, cut))
            a = cut
    return out


def many_blocks_case():
    """One sequence of 3 TILE bases: STRETCH_N[1] one-base N blocks at every second position from STRETCH_N[0] (six chunks of a
    block list in one segment), STRETCH_M[1] adjacent one-base mask blocks from STRETCH_M[0] (a thread's 16 positions are 16
    blocks), a mask block over the head of the N stretch and an N block over part of the mask stretch.
      track_of, starts, lengths   rows whose lengths are multiples of 16, so that every row begins on a thread's first byte: the
                                  start of each stretch at every offset 0 .. 15 of a thread's 16 bytes, the whole stretch in
                                  the first of them; rows that begin inside the stretches
      comp                        rows cut at each of the first 40 and of the last 40 positions of each stretch, on either side
    -> dict(seqs, track_of, starts, lengths, comp, most): `most` the largest number of blocks of one list that one segment meets"""
    if "many" in _cases:
        return _cases["many"]
    rng = np.random.default_rng(304)
    size = 3 * TILE
    (n0, n_count), (m0, m_count) = STRETCH_N, STRETCH_M
    n_starts = np.concatenate([[40], n0 + 2 * np.arange(n_count), [8000, 12000]])
    n_sizes = np.concatenate([[7], np.ones(n_count, dtype=np.int64), [300, size - 12000]])
    m_starts = np.concatenate([[0, 1990], m0 + np.arange(m_count), [m0 + m_count + 3]])
    m_sizes = np.concatenate([[19, 610], np.ones(m_count, dtype=np.int64), [2000]])
    seq = sequence_of(size, n_starts, n_sizes, m_starts, m_sizes, rng.integers(0, 256, size // 4, dtype=np.uint8))
    n_end, m_end = n0 + 2 * n_count - 1, m0 + m_count
    rows = []
    for k in range(16):  # (the first two rows hold the whole stretches, the others their first bases)
        rows.append((n0 - 16 - k, 2 * n_count + 40 if k == 0 else 64))   # the N stretch begins at byte k of a thread's 16
        rows.append((m0 - 16 - k, m_count + 48 if k == 0 else 64))       # the mask stretch at byte k
    rows += [(n0 + 7, 496), (n0 + 1000, 2096), (n0 + 2 * n_count - 40, 64), (m0 + 5, 96), (m0 + 600, 704), (m0 + m_count - 9, 16)]
    starts, lengths = (np.array(x, dtype=np.int64) for x in zip(*rows))
    assert (lengths % 16 == 0).all()
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for k in range(16):  # where the stretches begin in the output
        assert (offsets[2 * k] + n0 - starts[2 * k]) % 16 == k and (offsets[2 * k + 1] + m0 - starts[2 * k + 1]) % 16 == k
    b = blocks_of(seq)
    most = 0
    for r, a, cut in segments_of(offsets):
        p0, p1 = int(starts[r]) + a - int(offsets[r]), int(starts[r]) + cut - int(offsets[r])
        p0, p1 = max(p0, 0), min(p1, size)
        for st, en in ((b[0], b[1]), (b[2], b[3])):
            most = max(most, int(np.searchsorted(st, p1, side="left") - np.searchsorted(en, p0, side="right")))
    comp = []
    for first, past in ((n0, n_end), (m0, m_end)):
        for d in range(40):
            comp += [(first + d, past + 5), (first - 5, first + d + 1), (past - 40 + d, past + 5), (first - 5, past - 40 + d + 1), (first + d, past - d)]
    cs, ce = (np.array(x, dtype=np.int64) for x in zip(*comp))
    case = dict(seqs=[seq], track_of=np.zeros(len(rows), dtype=np.int64), starts=starts, lengths=lengths,
                comp=(np.zeros(len(comp), dtype=np.int64), cs, ce), most=most)
    _cases["many"] = case
    return case


def check_many_blocks_case(bases, counts):
    """many_blocks_case through `bases` and `counts` (check_random_case), against the whole-sequence model"""
    case = many_blocks_case()
    assert case["most"] >= 5 * CHUNK  # one segment meets at least five chunks of a block list
    seqs, model = case["seqs"], M.Letters(case["seqs"])
    track_of, starts, lengths = case["track_of"], case["starts"], case["lengths"]
    for do_mask in (True, False):
        want, _ = model.bases(track_of, starts, lengths, do_mask, ord("N"))
        text = want.tobytes()
        assert b"N" in text and (b"n" in text and b"a" in text) == do_mask
        assert np.array_equal(bases(seqs, track_of, starts, do_mask, ord("N"), lengths=lengths), want), do_mask
    t, s, e = case["comp"]
    want = model.composition(t, s, e, True)
    assert (want[:, 3:] > 0).any(axis=0).all()
    assert np.array_equal(counts(seqs, t, s, e, True), want), "composition"


# ---- the large sequences of the device tests ----
BIG_SIZES = (5 * SCAN_TILE * CKPT + 777, 6143 * CKPT - 5)
BIG_N_BLOCKS, BIG_M_BLOCKS = 7000, 60000


def big_sequence(which):
    """BIG_SIZES[which] bases under exactly BIG_N_BLOCKS N blocks of 1 .. 3000 bases and BIG_M_BLOCKS mask blocks of 1 .. 300: the
    running tables of its checkpoints (10 242 and 6 144 entries a plane) and of its N blocks (7 001) go through several tiles of
    the device scan.  Made once, never changed."""
    key = ("big", which)
    if key not in _cases:
        rng = np.random.default_rng(310 + which)
        seq = random_sequence(rng, BIG_SIZES[which], BIG_N_BLOCKS, BIG_M_BLOCKS, n_longest=3000, m_longest=300)
        assert len(seq.n_starts) == BIG_N_BLOCKS and len(seq.m_starts) == BIG_M_BLOCKS
        assert seq.n_sizes.min() == 1 and seq.n_sizes.max() == 3000
        n0 = seq.n_starts
        n1 = n0 + seq.n_sizes
        inside_one = (n0 // CKPT == (n1 - 1) // CKPT)
        assert inside_one.any() and ((n1 - 1) // CKPT - n0 // CKPT >= 2).any()
        _cases[key] = seq
    return _cases[key]


def big_letters(which):
    """twobit_model.letters of big_sequence(which) with do_mask on, made once (without do_mask: these & ~0x20)"""
    key = ("big letters", which)
    if key not in _cases:
        _cases[key] = M.letters(big_sequence(which), True)
        _cases[key].setflags(write=False)
    return _cases[key]


def contained_blocks(seq, s, e):
    """(j0, j1): the N blocks wholly inside the clipped rows [s, e) are j0 .. j1 - 1 (j0 >= j1: none)"""
    n0, n1, _, _ = blocks_of(seq)
    return np.searchsorted(n0, s, side="left"), np.searchsorted(n1, e, side="right")


def big_composition_rows(which, n_random=40_000):
    """(starts, ends) int64 for big_sequence(which): n_random rows of log-uniform lengths 1 .. size; rows that begin or end at
    1024 k + d for k around the scan tiles' edges and the last checkpoint, d in -1, 0, 1; rows whose first or last wholly
    contained N block is block 2046 .. 2049; rows clipped on both sides"""
    key = ("big rows", which, n_random)
    if key in _cases:
        return _cases[key]
    seq = big_sequence(which)
    size = seq.size
    rng = np.random.default_rng(320 + which)
    ln = log_uniform(rng, 1, size, n_random)
    s = (rng.random(n_random) * (size - ln + 1)).astype(np.int64)
    rows = [(s, s + ln)]
    last = (size + CKPT - 1) // CKPT - 1
    ks = [k for k in (2047, 2048, 2049, 4095, 4096, 4097, last) if k * CKPT - 1 <= size]
    cuts = np.array(sorted({min(max(CKPT * k + d, 0), size) for k in ks for d in (-1, 0, 1)}), dtype=np.int64)
    far = rng.integers(0, size + 1, (len(cuts), 6))
    near = rng.integers(1, 3 * CKPT, (len(cuts), 6))
    for other in (far, np.clip(cuts[:, None] - near, 0, size), np.clip(cuts[:, None] + near, 0, size)):
        a, b = np.minimum(cuts[:, None], other).reshape(-1), np.maximum(cuts[:, None], other).reshape(-1)
        rows.append((a, b))
    rows.append((cuts[:-1], cuts[1:]))
    n0, n1, _, _ = blocks_of(seq)
    ds, de = [], []
    for j in (2046, 2047, 2048, 2049):
        for other in (0, 1, 2, 5, 700, 4000, len(n0) - 1):
            for lead, tail in ((0, 0), (1, 0), (0, 1), (3, 2)):
                lo, hi = min(j, other), max(j, other)
                # the row begins `lead` bases before block lo (0: on its start; past the block before: that one is cut) and
                # ends `tail` bases after block hi
                ds.append(max(int(n0[lo]) - lead, 0))
                de.append(min(int(n1[hi]) + tail, size))
    rows.append((np.array(ds, dtype=np.int64), np.array(de, dtype=np.int64)))
    rows.append((np.array([-5, -1, -(1 << 30), 0, size - 3], dtype=np.int64), np.array([size + 9, size + 1, (1 << 31) - 1, size, size + 100], dtype=np.int64)))
    rows.append((np.array([0], dtype=np.int64), n1[2048:2049]))  # the last row: from 0 to the end of N block 2048
    _cases[key] = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    for a in _cases[key]:
        a.setflags(write=False)
    return _cases[key]


def big_composition_want(which):
    """`composition` of big_composition_rows(which) with do_mask on: int32 [n, 6], made once and never changed"""
    key = ("big counts", which)
    if key not in _cases:
        _cases[key] = composition(big_letters(which), *big_composition_rows(which))
        _cases[key].setflags(write=False)
    return _cases[key]


def big_conditions(which):
    """(big_sequence(which), facts) -- facts, from the blocks and the rows alone: `stride`, the entries of a plane of the checkpoint
    table; how many rows of big_composition_rows have wholly contained N blocks on both sides of block 2048 (the kernel's j0 < 2048
    < j1: the difference of n_codes entries from two tiles of the device scan) and how many have checkpoints on both sides of
    checkpoint 2048 (k0 < 2048 < k1)"""
    seq = big_sequence(which)
    s, e = big_composition_rows(which)
    s, e = np.clip(s, 0, seq.size), np.clip(e, 0, seq.size)
    j0, j1 = contained_blocks(seq, s, e)
    k0, k1 = (s + CKPT - 1) // CKPT, e // CKPT
    facts = {"stride": (seq.size + CKPT - 1) // CKPT + 1, "rows over N block 2048": int(((j0 < SCAN_TILE) & (SCAN_TILE < j1)).sum()),
             "rows over checkpoint 2048": int(((k0 < SCAN_TILE) & (SCAN_TILE < k1)).sum())}
    for j in (2046, 2047, 2048, 2049):
        assert (j0 == j).any() and (j1 == j + 1).any(), j  # the first, the last wholly contained block
    return seq, facts


# ---- a sequence at the top of int32 ----
TOP_SIZE = (1 << 31) - 1
TOP_WINDOWS = ((0, 4096), ((1 << 30) - 2048, (1 << 30) + 2048), (TOP_SIZE - 8192, TOP_SIZE))
TOP_N = (1 << 29, (1 << 29) + (1 << 28))     # the large N block
TOP_MASK = (5000, TOP_SIZE - 9000)           # the large mask block


def overlap(a0, a1, b0, b1):
    return max(min(a1, b1) - max(a0, b0), 0)


class TopSequence:
    """TOP_SIZE bases: the packed bytes zero (T) except random ones under TOP_WINDOWS, one N block TOP_N, one mask block TOP_MASK,
    small N and mask blocks inside the windows, the last mask block ending at the size.  The model of it keeps the letters of the
    three windows and knows the rest by rule -- outside the windows a base is T, N inside TOP_N, lower case inside TOP_MASK -- so
    nothing of 2^31 entries is built but the packed bytes themselves (zeros the system hands out untouched)."""

    def __init__(self):
        size = TOP_SIZE
        rng = np.random.default_rng(330)
        packed = np.zeros((size + 3) // 4, dtype=np.uint8)
        for a, b in TOP_WINDOWS:
            packed[a // 4:(b + 3) // 4] = rng.integers(0, 256, (b + 3) // 4 - a // 4, dtype=np.uint8)
            packed[a // 4] &= 0xFF >> (2 * (a % 4))  # (the bases of that byte before the window stay T)
        half = 1 << 30
        n = [(0, 3), (50, 10), (1020, 10), (4090, 3), (TOP_N[0], TOP_N[1] - TOP_N[0]), (half - 5, 12), (half + 1000, 1), (half + 1001, 1), (size - 8190, 90), (size - 20, 10)]
        m = [(10, 10), (100, 1), (101, 1), (4000, 90), (TOP_MASK[0], TOP_MASK[1] - TOP_MASK[0]), (size - 8000, 10), (size - 4097, 2), (size - 5, 5)]
        self.seq = sequence_of(size, [s for s, _ in n], [z for _, z in n], [s for s, _ in m], [z for _, z in m], packed)
        self.size = size
        for a, b in TOP_WINDOWS:  # the large N block lies outside the windows; the large mask block covers the second one only
            assert overlap(a, b, *TOP_N) == 0
        assert [overlap(a, b, *TOP_MASK) for a, b in TOP_WINDOWS] == [0, 4096, 0]
        self._letters = {do_mask: [window(self.seq, a, b, do_mask) for a, b in TOP_WINDOWS] for do_mask in (True, False)}

    def letters(self, a, b, do_mask=True):
        """uint8[b - a], 0 <= a <= b <= size, for rows of a few thousand bases"""
        out = np.full(b - a, ord("T"), dtype=np.uint8)
        lo, hi = max(a, TOP_N[0]), min(b, TOP_N[1])
        if lo < hi:
            out[lo - a:hi - a] = ord("N")
        lo, hi = max(a, TOP_MASK[0]), min(b, TOP_MASK[1])
        if do_mask and lo < hi:
            out[lo - a:hi - a] |= 0x20
        for (w0, w1), text in zip(TOP_WINDOWS, self._letters[bool(do_mask)]):
            lo, hi = max(a, w0), min(b, w1)
            if lo < hi:
                out[lo - a:hi - a] = text[lo - w0:hi - w0]
        return out

    def row(self, start, length, do_mask=True, pad=ord("N")):
        out = np.full(length, pad, dtype=np.uint8)
        lo, hi = max(start, 0), min(start + length, self.size)
        if lo < hi:
            out[lo - start:hi - start] = self.letters(lo, hi, do_mask)
        return out

    def composition(self, starts, ends, do_mask=True):
        """int64 [n, 6]: int64, so that a count beyond int32 would show as a difference, not wrap with the device's"""
        out = np.zeros((len(starts), 6), dtype=np.int64)
        for i, (s, e) in enumerate(zip(starts, ends)):
            s, e = max(int(s), 0), min(int(e), self.size)
            if s >= e:
                continue
            counts, inside, masked_inside = np.zeros(6, dtype=np.int64), 0, 0
            for (w0, w1), text in zip(TOP_WINDOWS, self._letters[bool(do_mask)]):
                lo, hi = max(s, w0), min(e, w1)
                if lo < hi:
                    counts += counts_of_letters(text[lo - w0:hi - w0])
                    inside += hi - lo
                    masked_inside += overlap(lo, hi, *TOP_MASK)
            n_outside = overlap(s, e, *TOP_N)
            counts[3] += (e - s) - inside - n_outside  # T
            counts[4] += n_outside
            if do_mask:
                counts[5] += overlap(s, e, *TOP_MASK) - masked_inside
            out[i] = counts
        return out


def top_sequence():
    if "top" not in _cases:
        _cases["top"] = TopSequence()
    return _cases["top"]
