"""
Seeded strand cases at the smallest shapes that can go wrong, for tests/test_strand_kernel_host.py and tests/test_gpu_strand.py (a
helper: no tests here, no GPU).  A case is a dict of rows with a strand each and `runs`, the ways a device is asked (misalign, slab,
force, grid, slack, slab_rows: a device ignores what it has no handle for); the check functions hold every device to the answer of
tests/strand_model.py, computed once per case and setting.  What a case is there for is asserted on the MODEL's answer, and at least
that the minus answer differs from the plus answer, so a case cannot pass vacuously.

A device is an object with
    bases(seqs, track_of, starts, strands, lengths=None, width=0, do_mask=True, pad=78, **run) -> uint8 [total]
    composition(seqs, track_of, starts, ends, strands, do_mask=True) -> int32 [n, 6]
    counts(seqs, track_of, starts, strands, k, radix, digits, lengths=None, width=0, do_mask=True, **run) -> int32 [n, radix ** k]
strands is None (the unstranded kernel or entry point) or a list of 0 / 1.
"""
import numpy as np

import kmer_cases as KC
import kmer_model as K
import strand_model as S
import twobit_cases as TC
import twobit_model as M
from twobit_model import CHUNK, TILE

CODE = {"T": 0, "C": 1, "A": 2, "G": 3}


def pack(text):
    """the packed bytes of upper-case letters: four to a byte, the first in the two most significant bits"""
    codes = np.array([CODE[ch] for ch in text] + [0] * (-len(text) % 4), dtype=np.uint8).reshape(-1, 4)
    return (codes[:, 0] << 6 | codes[:, 1] << 4 | codes[:, 2] << 2 | codes[:, 3]).astype(np.uint8)


def alternate(n, first=1):
    return [(first + i) % 2 for i in range(n)]


# ---------------------------------------------------------------- letters --
def letters_ragged_case():
    """ragged rows on the structural sequences: minus rows of 0, 1, 15, 16, 17 and 33 bases; plus and minus rows of 5 bases
    alternating inside one tile, through block edges; a minus row that crosses a thread's 16 bytes, a packed word and the first tile's
    end; a minus row over three tiles; the stretch of CHUNK + 5 one-base N blocks under a minus row; minus rows that begin below 0 and
    end past the size; a row inside an N block; rows that name no track and the size-0 sequence"""
    st = M.stretch_start()
    rows = [(0, 100 + 7 * i, n, 1) for i, n in enumerate((0, 1, 15, 16, 17, 33))]
    rows += [(0, 95 + i, 5, i % 2) for i in range(40)]
    head = sum(r[2] for r in rows)
    rows += [(0, 3000, TILE - head - 9, 0), (0, 10, 30, 1)]                     # the second: 9 bytes in tile 0, 21 in tile 1
    rows += [(0, 4000, 2 * TILE + 17, 1), (0, st - 3, 2 * (CHUNK + 5) + 6, 1)]  # three tiles; the stretch
    rows += [(0, -7, 20, 1), (0, 20000, 40, 1), (1, -3, 50, 1), (3, 2570, 20, 1), (0, -7, 20, 0)]
    rows += [(0, 7100, 300, 1), (-1, 5, 9, 1), (2, 0, 5, 1), (2, -2, 3, 1), (3, 0, 2579, 1), (1, 0, 41, 0), (1, 0, 41, 1)]
    t, s, n, m = (list(x) for x in zip(*rows))
    return dict(seqs=M.structural_sequences(), track_of=t, starts=s, lengths=n, strands=m, runs=({}, {"misalign": 1}, {"slab": 2}, {"slab": 1, "misalign": 7}),
                settings=((True, ord("N")), (False, ord(".")), (True, ord("A")), (True, 0)), expect=letters_ragged_expect)


def letters_ragged_expect(case, want, offsets, do_mask, pad):
    t, s, n, m = case["track_of"], case["starts"], case["lengths"], case["strands"]
    rows = [want[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    cross = n.index(30)
    assert offsets[cross] == TILE - 9 and m[cross] == 1 and (offsets[cross] % 16, s[cross] % 16) == (7, 10)
    three = n.index(2 * TILE + 17)
    assert offsets[three] // TILE + 2 == (offsets[three + 1] - 1) // TILE and m[three] == 1
    low = rows[s.index(-7)]  # a minus row that begins 7 below 0: the pad is at its END
    assert m[s.index(-7)] == 1 and (low[-7:] == pad).all() and (pad in (ord("A"), ord("N")) or not (low[:13] == pad).any())
    high = rows[s.index(20000)]  # one that ends 29 past the size: the pad is at its START
    assert (high[:29] == pad).all() and (pad in (ord("A"), ord("N")) or not (high[29:] == pad).any())
    for i in (t.index(-1), t.index(2)):
        assert (rows[i] == pad).all()
    if pad == ord("A"):  # a pad that is a letter is not complemented
        assert (low[-7:] == ord("A")).all() and (rows[t.index(-1)] == ord("A")).all()
    assert set(rows[s.index(7100)].tolist()) <= {ord("N"), ord("n")}
    stretch = rows[n.index(2 * (CHUNK + 5) + 6)]
    assert np.isin(stretch, (ord("N"), ord("n"))).sum() >= CHUNK + 5
    if not do_mask:
        assert not (want >= ord("a")).any() or pad >= ord("a")


def letters_matrix_case(width):
    """twobit_model.matrix_case(width) with alternating strands, the first row minus: windows that start below 0 and end beyond
    the sequence (the pad at the mirrored end), block edges, no track"""
    t, s = M.matrix_case(width)
    return dict(seqs=M.structural_sequences(), track_of=t, starts=s, width=width, strands=alternate(len(t)),
                runs=({}, {"slab": 1, "misalign": 5}) if width in (37, TILE + 1) else ({},), settings=((True, ord("-")), (False, ord("A"))))


def letters_edge_case():
    """One-base N and mask blocks at the first and at the last position of a minus row and just outside it, rows of 1, 5, 16, 17
    bases.  Of a minus row that starts at the block the LAST element is the block's; of one that ends with it the FIRST."""
    rng = np.random.default_rng(470)
    size, n_at, m_at = 400, 131, 262
    seq = TC.sequence_of(size, [n_at], [1], [m_at], [1], rng.integers(0, 256, size // 4, dtype=np.uint8))
    rows, where = [], []
    for at in (n_at, m_at):
        for length in (1, 5, 16, 17):
            for start, place in ((at, length - 1), (at - length + 1, 0), (at + 1, None), (at - length, None)):
                rows.append((0, start, length, 1))
                where.append((at == m_at, place))
    t, s, n, m = (list(x) for x in zip(*rows))
    return dict(seqs=[seq], track_of=t, starts=s, lengths=n, strands=m, where=where, runs=({}, {"misalign": 3}),
                settings=((True, ord("N")), (False, ord("N"))), expect=letters_edge_expect)


def letters_edge_expect(case, want, offsets, do_mask, pad):
    special = lambda row: np.flatnonzero((row == ord("N")) | (row >= ord("a")))  # noqa: E731
    for (is_mask, place), a, b in zip(case["where"], offsets[:-1], offsets[1:]):
        row = want[a:b]
        if place is None or (is_mask and not do_mask):
            assert len(special(row)) == 0, (is_mask, place)
        else:
            assert special(row).tolist() == [place] and (row[place] >= ord("a")) == is_mask


def want_letters(case, do_mask, pad):
    key = ("want", bool(do_mask), pad)
    if key not in case:
        model = S.Strand(case["seqs"])
        lengths = case["lengths"] if "lengths" in case else [case["width"]] * len(case["starts"])
        want, offsets = model.bases(case["track_of"], case["starts"], lengths, case["strands"], do_mask, pad)
        plus, _ = model.bases(case["track_of"], case["starts"], lengths, None, do_mask, pad)
        assert len(want) == len(plus) and (want != plus).any(), "the strands change nothing"
        for i, minus in enumerate(case["strands"]):  # a plus row of a mixed batch is the unstranded row
            if not minus:
                assert np.array_equal(want[offsets[i]:offsets[i + 1]], plus[offsets[i]:offsets[i + 1]])
        if "expect" in case:
            case["expect"](case, want, offsets.tolist(), do_mask, pad)
        want.setflags(write=False)
        plus.setflags(write=False)
        case[key] = want, plus
    return case[key]


def check_letters(devices, case, where=""):
    kw = dict(lengths=case.get("lengths"), width=case.get("width", 0))
    zeros = [0] * len(case["starts"])
    for do_mask, pad in case["settings"]:
        want, plus = want_letters(case, do_mask, pad)
        for dev in devices:
            for run in case["runs"]:
                got = dev.bases(case["seqs"], case["track_of"], case["starts"], case["strands"], do_mask=do_mask, pad=pad, **kw, **run)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (where, type(dev).__name__, do_mask, pad, run, np.flatnonzero(got != want)[:10])
            # a strand array of zeros, the unstranded form and the model's plus rows: byte for byte
            all_plus = dev.bases(case["seqs"], case["track_of"], case["starts"], zeros, do_mask=do_mask, pad=pad, **kw)
            unstranded = dev.bases(case["seqs"], case["track_of"], case["starts"], None, do_mask=do_mask, pad=pad, **kw)
            assert all_plus.tobytes() == unstranded.tobytes() == plus.tobytes(), (where, type(dev).__name__, do_mask, pad)


# ---------------------------------------------------------------- base counts --
def composition_case():
    """the rows of the letters cases and of twobit_model.composition_case, strands alternating"""
    ragged = letters_ragged_case()
    t, s, e = M.composition_case()
    t = t + ragged["track_of"]
    e = e + [a + n for a, n in zip(ragged["starts"], ragged["lengths"])]
    s = s + ragged["starts"]
    return dict(seqs=M.structural_sequences(), track_of=t, starts=s, ends=e, strands=alternate(len(t)))


def check_composition(devices, case, where=""):
    model = S.Strand(case["seqs"])
    zeros = [0] * len(case["starts"])
    for do_mask in (True, False):
        want = model.composition(case["track_of"], case["starts"], case["ends"], case["strands"], do_mask)
        plus = M.Letters(case["seqs"]).composition(case["track_of"], case["starts"], case["ends"], do_mask)
        swapped = np.where(np.array(case["strands"], dtype=bool)[:, None], plus[:, [3, 2, 1, 0, 4, 5]], plus)
        assert np.array_equal(want, swapped) and (want != plus).any() and np.array_equal(want[:, 4:], plus[:, 4:])
        for dev in devices:
            got = dev.composition(case["seqs"], case["track_of"], case["starts"], case["ends"], case["strands"], do_mask)
            assert got.dtype == np.int32 and np.array_equal(got, want), (where, type(dev).__name__, do_mask, np.flatnonzero((got != want).any(axis=1))[:10])
            all_plus = dev.composition(case["seqs"], case["track_of"], case["starts"], case["ends"], zeros, do_mask)
            unstranded = dev.composition(case["seqs"], case["track_of"], case["starts"], case["ends"], None, do_mask)
            assert np.array_equal(all_plus, unstranded) and np.array_equal(unstranded, plus), (where, type(dev).__name__, do_mask)


# ---------------------------------------------------------------- k-mers --
def kmer_case(base, strands=None, runs=None, name=None):
    """a case of tests/kmer_cases.py (imported, never edited) with a strand per row; its `expect` is not taken over"""
    n = len(base["starts"])
    case = {k: v for k, v in base.items() if k in ("seqs", "track_of", "starts", "lengths", "width", "k", "radix", "table", "do_masks")}
    case["strands"] = alternate(n) if strands is None else strands
    case["runs"] = base["runs"] if runs is None else runs
    case["name"] = name
    return case


_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def boundary_case(k, table="acgt"):
    """kmer_cases.boundary_case: windows across a word, a thread's run, a tile and a segment, rows of k - 1, k and k + 1 bases, rows
    below 0 and past the size, the ways forced, a grid of two, host slabs of 3 rows -- strands alternating, so every slab is mixed"""
    return made_once(("boundary", k, table), lambda: kmer_case(KC.boundary_case(k, table)))


def plan_case():
    """kmer_cases.plan_case: segments on both sides of KM_CUT, both ways forced; minus, plus, minus, minus, plus, minus"""
    return made_once("plan", lambda: kmer_case(KC.plan_case(), strands=[1, 0, 1, 1, 0, 1]))


def long_row_case(tiles=5):
    """one MINUS row of more tiles than the grid of two"""
    return made_once(("long", tiles), lambda: kmer_case(KC.long_row_case(tiles), strands=[1]))


def many_rows_case(rows=2500):
    """thousands of rows of 0 .. 3 bases in one tile, a random half of them minus"""
    def make():
        base = KC.many_rows_case(rows)
        return kmer_case(base, strands=np.random.default_rng(480).integers(0, 2, rows).tolist())
    return made_once(("many", rows), make)


def window_case(width, k):
    """kmer_cases.window_case: windows of one width (the matrix form), alternating strands, host slabs of 4 rows"""
    return made_once(("window", width, k), lambda: kmer_case(KC.window_case(width, k)))


def palindrome_case(k=3):
    """a row that is its own reverse complement (minus counts == plus counts) beside one that is not, both strands of each"""
    def make():
        rng = np.random.default_rng(490)
        half = "".join("ACGT"[i] for i in rng.integers(0, 4, 30))
        text = "ACCGTTGA" + half + S.reverse_complement_str(half) + "TTGACAAC"
        seq = TC.sequence_of(len(text), [], [], [], [], pack(text))
        tab, radix = KC.TABLES["acgt"]
        return dict(seqs=[seq], track_of=[0] * 4, starts=[8, 8, 0, 0], lengths=[60, 60, 40, 40], strands=[1, 0, 1, 0], k=k, radix=radix, table=tab,
                    runs=KC.WAYS, name="palindrome")
    return made_once(("palindrome", k), make)


def want_counts(case, do_mask):
    key = ("want", bool(do_mask))
    if key not in case:
        n = len(case["starts"])
        lengths = case["lengths"] if "lengths" in case else [case["width"]] * n
        model = S.Strand(case["seqs"])
        want = model.counts(case["track_of"], case["starts"], lengths, case["strands"], case["k"], case["radix"], case["table"], do_mask)
        plus = K.Counts(case["seqs"]).counts(case["track_of"], case["starts"], lengths, case["k"], case["radix"], case["table"], do_mask)
        minus = np.array(case["strands"], dtype=bool)
        assert np.array_equal(want[~minus], plus[~minus])
        if case.get("name") == "palindrome":
            assert np.array_equal(want[0], plus[0]) and want[0].sum() == 60 - case["k"] + 1 and not np.array_equal(want[2], plus[2])
        else:
            assert (want != plus).any(), "the strands change nothing"
        if closed(case["table"], case["radix"]):  # the helper's permutation of the plus columns
            rc = strand_columns_of(case)
            assert np.array_equal(want[minus], plus[minus][:, rc])
        elif do_mask or not closed_upper(case["table"]):  # whatever digit is taken for the complement of each digit, the columns of
            for rc in digit_permutations(case["k"], case["radix"]):  # the plus counts, so permuted, are not these counts
                assert not np.array_equal(want[minus], plus[minus][:, rc]), "a table that is not closed under complement, and nothing shows it"
        want.setflags(write=False)
        case[key] = want
    return case[key]


def closed(table, radix):
    """whether the complements of the letters of every digit have one digit"""
    comp = {}
    for ch in K.LETTERS:
        d = int(table[ord(ch)])
        if d >= 0:
            c = int(table[S.COMPLEMENT[ord(ch)]])
            if c < 0 or comp.setdefault(d, c) != c:
                return False
    return True


def digit_permutations(k, radix):
    """for every permutation c of the digits, the columns w -> the word of c[digits of w] in reverse order"""
    import itertools

    index = np.arange(radix ** k)
    for c in itertools.permutations(range(radix)):
        out = np.zeros_like(index)
        for t in range(k):
            out += np.array(c)[(index // radix ** t) % radix] * radix ** (k - 1 - t)
        yield out
        yield np.argsort(out)


def closed_upper(table):
    """`closed` on the upper-case letters alone: what is left of a table without do_mask"""
    upper = table.copy()
    upper[[ord(ch) for ch in "acgt"]] = -1
    return closed(upper, 0)


def strand_columns_of(case):
    from bxmi import kmers  # (a pure helper: no device)

    letter_digits = {ch: int(case["table"][ord(ch)]) for ch in K.LETTERS if case["table"][ord(ch)] >= 0}
    return kmers.strand_columns(case["k"], letter_digits)


def check_counts(devices, case, where=""):
    digits = K.digits8(case["table"])
    kw = dict(lengths=case.get("lengths"), width=case.get("width", 0))
    zeros = [0] * len(case["starts"])
    for do_mask in case.get("do_masks", (True, False)):
        want = want_counts(case, do_mask)
        for dev in devices:
            for run in case["runs"]:
                got = dev.counts(case["seqs"], case["track_of"], case["starts"], case["strands"], case["k"], case["radix"], digits, do_mask=do_mask, **kw, **run)
                assert got.dtype == np.int32 and got.shape == want.shape, (where, got.dtype, got.shape)
                assert np.array_equal(got, want), (where, type(dev).__name__, do_mask, run, np.flatnonzero((got != want).any(axis=1))[:10])
            all_plus = dev.counts(case["seqs"], case["track_of"], case["starts"], zeros, case["k"], case["radix"], digits, do_mask=do_mask, **kw)
            unstranded = dev.counts(case["seqs"], case["track_of"], case["starts"], None, case["k"], case["radix"], digits, do_mask=do_mask, **kw)
            assert np.array_equal(all_plus, unstranded), (where, type(dev).__name__, do_mask)
