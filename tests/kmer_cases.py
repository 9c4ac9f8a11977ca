"""
Seeded k-mer cases at the smallest shapes that can go wrong, for tests/test_kmer_kernel_host.py and tests/test_gpu_kmers.py (a
helper: no tests here, no GPU).  A case is a dict -- seqs, track_of, starts, lengths (ragged) or width (windows), k, radix, table
(kmer_model.table_of) and `runs`, the ways a device is asked (force, grid, slack, slab_rows: a device ignores what it has no handle
for) -- and `check` holds every device to the model's answer, computed once per case and do_mask setting.  What a case is there
for is asserted on the model's answer where it is built, so a case cannot pass vacuously.

A device is an object with
    counts(seqs, track_of, starts, k, radix, digits, lengths=None, width=0, do_mask=True, **run) -> int32 [n, radix ** k]
"""
import numpy as np

import kmer_model as K
import twobit_cases as TC
import twobit_model as M
from kmer_model import LDS_BINS, BINS_MAX, CUT, RUN, TILE
from twobit_model import CHUNK

TABLES = {
    "acgt": (K.table_of(K.MAPPINGS["acgt"][0]), 4),
    "dna": (K.table_of(K.MAPPINGS["dna"][0]), 4),
    "ry": (K.table_of(K.MAPPINGS["ry"][0]), 2),
    "ry_folded": (K.table_of({"A": 0, "G": 0, "a": 0, "g": 0, "C": 1, "T": 1, "c": 1, "t": 1}), 2),
    "no_g": (K.table_of({"A": 0, "C": 1, "T": 2, "a": 0, "c": 1, "t": 2}), 3),  # an upper-case letter without a digit; radix 3
    "shared": (K.table_of({"A": 0, "a": 0, "C": 1, "t": 1, "G": 2, "T": 3}), 4),    # two letters on one digit, T and t on different ones
}
WAYS = ({}, {"force": 1}, {"force": 2})
_cases = {}


def made_once(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def sequence(seed, size, n_blocks=10, m_blocks=8, n_longest=30, m_longest=120):
    """random packed bytes under a few short random blocks (twobit_cases.random_blocks; not random_sequence, which asks a sequence
    of this many blocks for edges it has no room for)"""
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8)
    n, m = TC.random_blocks(rng, size, n_blocks, n_longest), TC.random_blocks(rng, size, m_blocks, m_longest)
    return TC.sequence_of(size, n[0], n[1], m[0], m[1], packed)


def boundary_rows(k, size):
    """ragged rows: one that ends 3 elements before the first tile's end, one of 20 bases that crosses it (its first windows take
    their letters from the next tile's share), rows of 0, k - 1, k and k + 1 bases, a row over several tiles, rows that end at the
    size, pass it and begin below 0, a row that names no track"""
    rows = [(0, 5, TILE - 3), (0, 100, 20), (0, 0, 0), (0, 50, k - 1), (0, 60, k), (0, 70, k + 1), (0, 80, 0), (0, 7, 2 * TILE + 17),
            (0, size - 30, 30), (0, size - 10, 25), (0, -4, 20), (-1, 5, 30), (0, 16 - k // 2, k + 1), (0, 3, 40)]
    t, s, n = zip(*rows)
    return list(t), list(s), list(n)


def boundary_case(k, table="acgt"):
    """windows across a 16-base word, a thread's run, a tile and a row segment, on a random sequence of three tiles and a bit"""
    def make():
        seq = sequence(400 + k, 3 * TILE + 77)
        t, s, n = boundary_rows(k, seq.size)
        tab, radix = TABLES[table]
        runs = WAYS + ({"grid": 2, "slack": 3 * TILE + 5}, {"slab_rows": 3})
        return dict(seqs=[seq], track_of=t, starts=s, lengths=n, k=k, radix=radix, table=tab, runs=runs, expect=boundary_expect)
    return made_once(("boundary", k, table), make)


def boundary_expect(case, want, do_mask):
    k, n = case["k"], case["lengths"]
    sums = want.sum(axis=1)
    assert (sums[[2, 3, 6, 11]] == 0).all() and (sums <= np.maximum(np.array(n) - k + 1, 0)).all()
    assert sums[0] > 0 and sums[7] > 0
    if all(case["table"][ord(ch)] >= 0 for ch in "ACGT"):  # most windows are words: the blocks are few and short
        assert sums[0] > TILE // 4 and sums[7] > TILE // 2 and sums[1] > 0 and sums[4] + sums[5] + sums[12] > 0


def block_edge_case(k):
    """One-base N and mask blocks at every offset of a window.  Rows of k + e bases, e in 0, 2, with the block at offset d of the
    row, d in -1 .. k + e: it kills exactly the windows over it -- min(d, e) - max(d - k + 1, 0) + 1 of the e + 1 -- and none from
    just outside the row (d = -1, d = k + e).  The mask block kills only with do_mask, under a table without lower case."""
    def make():
        rng = np.random.default_rng(420 + k)
        size, n_at, m_at = 400, 131, 262
        seq = TC.sequence_of(size, [n_at], [1], [m_at], [1], rng.integers(0, 256, size // 4, dtype=np.uint8))
        rows, killed = [], []
        for at, is_mask in ((n_at, False), (m_at, True)):
            for e in (0, 2):
                for d in range(-1, k + e + 1):
                    rows.append((0, at - d, k + e))
                    killed.append((is_mask, e, min(d, e) - max(d - k + 1, 0) + 1 if 0 <= d < k + e else 0))
        t, s, n = zip(*rows)
        tab, radix = TABLES["acgt"]
        return dict(seqs=[seq], track_of=list(t), starts=list(s), lengths=list(n), k=k, radix=radix, table=tab, runs=WAYS, killed=killed,
                    expect=block_edge_expect)
    return made_once(("edge", k), make)


def block_edge_expect(case, want, do_mask):
    sums = want.sum(axis=1).tolist()
    for got, (is_mask, e, dead) in zip(sums, case["killed"]):
        assert got == e + 1 - (dead if do_mask or not is_mask else 0), (got, is_mask, e, dead, do_mask)
    assert any(dead == 0 for _, _, dead in case["killed"]) and any(dead == 3 for _, e, dead in case["killed"] if e == 2) == (case["k"] >= 3)


def stretch_case(k=2, table="acgt"):
    """twobit_model.ragged_case() on the structural sequences: the stretch of CHUNK + 5 one-base N blocks of blocks.2bit inside one
    segment (two chunks of the list), rows of one base, pad positions on both sides, a row that names no track, the size-0 sequence"""
    def make():
        t, s, n = M.ragged_case()
        tab, radix = TABLES[table]
        return dict(seqs=M.structural_sequences(), track_of=t, starts=s, lengths=n, k=k, radix=radix, table=tab, runs=WAYS, expect=stretch_expect)
    return made_once(("stretch", k, table), make)


def stretch_expect(case, want, do_mask):
    t, s, n = case["track_of"], case["starts"], case["lengths"]
    row = n.index(2 * (CHUNK + 5) + 6)
    assert s[row] == M.stretch_start() - 3
    # every second base of the stretch is an N: no window of two letters survives inside it
    assert want[row].sum() <= 6 if case["k"] == 2 else True
    assert want.sum() > 1000 and (want[[i for i, x in enumerate(t) if x == -1 or x == 2]] == 0).all()


def window_case(width, k, table="dna"):
    """twobit_model.matrix_case(width): windows of one width that start below 0 and end beyond the sequence, block edges, no track"""
    def make():
        t, s = M.matrix_case(width)
        tab, radix = TABLES[table]
        return dict(seqs=M.structural_sequences(), track_of=t, starts=s, width=width, k=k, radix=radix, table=tab, runs=WAYS + ({"slab_rows": 4},))
    return made_once(("window", width, k, table), make)


def bins_case(k, table):
    """the boundary rows under radix ** k words: KM_BINS_MAX, KM_LDS_BINS (the largest histogram LDS holds) and the next ones"""
    case = boundary_case(k, table)
    assert case["radix"] ** k in (BINS_MAX, LDS_BINS, 2 * LDS_BINS, 3 ** 8)
    return case


def plan_case():
    """k = 4 at radix 4, 256 words: segments of 3 .. 500 window starts, on both sides of KM_CUT"""
    def make():
        seq = sequence(440, 2 * TILE)
        lengths = [10, CUT - 1, CUT, CUT + 1, 3, CUT + 116]
        starts = [20 + 37 * i for i in range(len(lengths))]
        assert sum(lengths) < TILE  # (one tile: every row is one segment)
        assert [K.use_lds(256, n) for n in lengths] == [False, False, True, True, False, True]
        tab, radix = TABLES["dna"]
        return dict(seqs=[seq], track_of=[0] * len(lengths), starts=starts, lengths=lengths, k=4, radix=radix, table=tab, runs=WAYS)
    return made_once("plan", make)


def long_row_case(tiles=5, k=3):
    """one row of more tiles than the grid (two workgroups), and a total that is only a bound several grid fills beyond it"""
    def make():
        seq = sequence(450, tiles * TILE + 200, n_blocks=30, m_blocks=30)
        tab, radix = TABLES["acgt"]
        runs = ({"grid": 2}, {"grid": 2, "slack": 7 * TILE + 5, "force": 1}, {"grid": 2, "force": 2})
        return dict(seqs=[seq], track_of=[0], starts=[9], lengths=[tiles * TILE + 9], k=k, radix=radix, table=tab, runs=runs)
    return made_once(("long", tiles, k), make)


def many_rows_case(rows=2500, k=2):
    """thousands of rows of 0 .. 3 bases in one tile"""
    def make():
        rng = np.random.default_rng(460)
        seq = sequence(460, TILE)
        lengths = rng.integers(0, 4, rows)
        lengths[:8] = [1, 2, 3, 0, 0, 2, 2, 1]
        starts = rng.integers(-2, TILE, rows)
        offsets = np.concatenate([[0], np.cumsum(lengths)])
        per_tile = np.bincount(offsets[:-1][lengths > 0] // TILE)
        assert per_tile.max() > 1000
        tab, radix = TABLES["dna"]
        return dict(seqs=[seq], track_of=[0] * rows, starts=starts.tolist(), lengths=lengths.tolist(), k=k, radix=radix, table=tab,
                    runs=({}, {"force": 1}), do_masks=(True,))
    return made_once(("many", rows, k), make)


def want_of(case, do_mask):
    """the model's answer, made once per case and setting and never changed"""
    key = ("want", bool(do_mask))
    if key not in case:
        n = len(case["starts"])
        lengths = case["lengths"] if "lengths" in case else [case["width"]] * n
        want = K.Counts(case["seqs"]).counts(case["track_of"], case["starts"], lengths, case["k"], case["radix"], case["table"], do_mask)
        if "expect" in case:
            case["expect"](case, want, do_mask)
        want.setflags(write=False)
        case[key] = want
    return case[key]


def check(devices, case, where=""):
    digits = K.digits8(case["table"])
    for do_mask in case.get("do_masks", (True, False)):
        want = want_of(case, do_mask)
        for dev in devices:
            for run in case["runs"]:
                got = dev.counts(case["seqs"], case["track_of"], case["starts"], case["k"], case["radix"], digits, lengths=case.get("lengths"),
                                 width=case.get("width", 0), do_mask=do_mask, **run)
                assert got.dtype == np.int32 and got.shape == want.shape, (where, got.dtype, got.shape)
                assert np.array_equal(got, want), (where, type(dev).__name__, do_mask, run, np.flatnonzero((got != want).any(axis=1))[:10])


assert RUN == 8  # (the rows above are placed for runs of 8 window starts in tiles of 2048)
