"""
Seeded cases for the stranded pwm calls at the smallest shapes that can go wrong, for tests/test_pwm_strand_kernel_host.py and
tests/test_gpu_pwm_strand.py (a helper: no tests here, no GPU).  PW_TILE is 1024 and a thread stages 8 columns.  A case is a dict of
rows with a strand each, matrices, and `runs`: the ways a device is asked for the planes (misalign, slab_tiles: a device ignores what
it has no handle for).  `check` holds every device to tests/pwm_strand_model.py, computed once per case and setting: planes bit for
bit, best hits, and the hits at -inf, at a score that occurs per matrix and at +inf.  What a case is there for is asserted on the
MODEL's answer, and always that the minus answer differs from the plus answer, so no case passes vacuously.
tests/test_pwm_strand_cases.py pins the model and shows which case catches which wrong device.

A device is an object with
    scores(seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, **run) -> float32 [n_mats, total]
    best(seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, **best_run) -> (float32, int32) [n_mats, n]
    hits(seqs, mats, track_of, starts, strands, thresholds, lengths=None, width=0, do_mask=True, **hits_run)
        -> (mat_hits int64 [n_mats + 1], rows int32, pos int32, score float32)
strands is None (the unstranded kernel or entry point) or a list of 0 / 1.
"""
import numpy as np

import pwm_cases as PC
import pwm_hits_cases as H
import pwm_model as P
import pwm_strand_model as PS
import strand_cases as SC
import strand_model as S
import twobit_cases as K
import twobit_model as M
from pwm_model import TILE, WIDTH_MAX

INF = np.float32(np.inf)
_made = {}


def made_once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def alternate(n, first=1):
    return [(first + i) % 2 for i in range(n)]


def case_of(seqs, mats, rows, **more):
    """rows: (track, start, length, strand)"""
    t, s, n, m = (list(x) for x in zip(*rows))
    return dict(seqs=seqs, mats=mats, track_of=t, starts=s, lengths=n, strands=m, **more)


# ---- the cases ----
def short_rows_case():
    """minus rows of 0, 1, W - 1, W, W + 1, 15, 16, 17 and 33 bases for W in 1, 4, 20, 256 -- one handle of the four recorded
    matrices over ACGT -- on a random sequence with blocks; every length once as a plus row too"""
    def make():
        rng = np.random.default_rng(600)
        seq = PC.sparse_sequence(rng, 30_000)
        lengths = sorted({0, 1, 15, 16, 17, 33} | {w + d for w in (1, 4, 20, WIDTH_MAX) for d in (-1, 0, 1)})
        rows = [(0, int(rng.integers(2000, 25_000)), n, 1) for n in lengths] + [(0, int(rng.integers(2000, 25_000)), n, 0) for n in lengths]
        return case_of([seq], [P.matrix(k) for k in ("w1", "w4", "w20", "wmax")], rows, runs=({}, {"misalign": 1}), name="short rows")
    return made_once("short", make)


def boundary_case():
    """pwm_model.ragged_case() -- a window across a tile boundary, a row that ends on one, rows around W = 20, windows across each
    edge of an N and of a mask block, the stretch of more than TB_CHUNK one-base N blocks, rows below 0 and past the size, rows
    without a track, the size-0 sequence, a row over three tiles -- with strands ALTERNATING row by row, then the same rows all
    minus; a minus row of 30 that crosses a thread's 8 staged columns, a packed word and a tile boundary; one minus row over three
    tiles under W = 256 (a halo of 255 columns crosses two segment boundaries); widths 1, 256 and 20 in one handle.  total % 4 == 1."""
    def make():
        t, s, n = P.ragged_case()
        rows = [(a, b, c, m) for (a, b, c), m in zip(zip(t, s, n), alternate(len(t)))]
        total = sum(n)
        rows.append((0, 3000, (-total - 9) % TILE, 0))
        rows.append((0, 10, 30, 1))                 # 9 elements in one tile, 21 in the next; start 10: mid word, mid thread
        cross = len(rows) - 1
        rows.append((0, 4000, 2 * TILE + 300, 1))  # three tiles under wmax
        rows += [(a, b, c, 1) for a, b, c in zip(t, s, n) if c < 400]
        rows.append((0, 50, (1 - sum(r[2] for r in rows)) % 4, 1))
        case = case_of(M.structural_sequences(), P.structural_mats(), rows, runs=({}, {"misalign": 1}, {"slab_tiles": 2}, {"slab_tiles": 1, "misalign": 3}),
                       name="boundary", cross=cross)
        offsets = H.offsets_of(case["lengths"])
        assert offsets[cross] % TILE == TILE - 9 and offsets[-1] % 4 == 1
        assert offsets[cross + 1] // TILE + 2 == (offsets[cross + 2] - 1) // TILE  # the long minus row: three tiles
        return case
    return made_once("boundary", make)


def edge_case():
    """strand_cases.letters_edge_case's rows: one-base N and mask blocks at the first and at the last position of a minus row and
    just outside it, rows of 1, 5, 16, 17 bases; a random set over all ten letters (every class its own column), widths 1 and 4"""
    def make():
        base = SC.letters_edge_case()
        rng = np.random.default_rng(610)
        rows = list(zip(base["track_of"], base["starts"], base["lengths"], base["strands"]))
        sample = np.concatenate(PS.texts(base["seqs"], base["track_of"], base["starts"], base["lengths"], base["strands"]))
        mats = PC.random_matrix_set(rng, (1, 4), 10, "all", sample)
        return case_of(base["seqs"], mats, rows, runs=({},), name="edges")
    return made_once("edges", make)


def matrix_form_case(width):
    """twobit_model.matrix_case(width): windows of one width -- below 0, past the size, block edges, no track -- strands alternating,
    the first minus; matrices over ACGTN and ACGTacgt (not closed under complement) need a handle each"""
    def make():
        t, s = M.matrix_case(width)
        return dict(seqs=M.structural_sequences(), mats=[P.matrix("w20n"), P.matrix("w4n")], track_of=t, starts=s, width=width, strands=alternate(len(t)),
                    runs=({}, {"slab_tiles": 1, "misalign": 3}) if width == 37 else ({},), name="matrix form %d" % width)
    return made_once(("matrix", width), make)


def set_case(name, rows=30, size=20_000, longest=1500):
    """pwm_cases.matrix_set_case(name) -- a set above PW_LDS_VALUES staged matrix by matrix, PW_MATS_MAX matrices, the mixed, g_top
    and n_top alphabets in 16 columns -- a random half of its rows minus; the order of the additions shows on the minus rows' own
    texts (pwm_cases.order_share, asserted here)"""
    def make():
        base = PC.matrix_set_case(name, rows, size, longest)
        rng = np.random.default_rng(620 + sorted(PC.MATRIX_SETS).index(name))
        strands = rng.integers(0, 2, len(base["track_of"])).tolist()
        strands[:8] = [1, 1, 1, 1, 0, 1, 1, 1]
        case = dict(base, strands=strands, runs=({},), name=name)
        minus_text = np.concatenate([r for r, m in zip(PS.texts(base["seqs"], base["track_of"], base["starts"], base["lengths"], strands), strands) if m])
        if any(m.width >= 3 for m in base["mats"]):
            assert PC.order_share(base["mats"], minus_text) >= 0.25, name
        return case
    return made_once(("set", name, rows, size, longest), make)


SETS = ("lds_plus_4", "lds_256x16", "mats_max", "cols16_mixed", "cols16_g_top")  # above the LDS; n_top; PW_MATS_MAX; mixed; g_top


def extremes_case(rows=60, size=20_000, longest=2000):
    """pwm_cases.extremes_case (+-inf, inf - inf, NaN entries, denormals), strands alternating"""
    def make():
        base = PC.extremes_case(rows, size, longest)
        return dict(base, strands=alternate(len(base["track_of"])), runs=({},), name="extremes")
    return made_once(("extremes", rows, size, longest), make)


def lane_case(which=PC.LANE_SAMPLE):
    """pwm_cases.lane_case MIRRORED: every row minus, under the complements of its two matrices (C scores highest where G did).
    Stretch i has its G at genomic offset i -- offset TILE - 1 - i of the strand's string -- and a one-base N block at genomic
    i + k, which in the strand's string comes FIRST: under the second matrix, where they tie, the N at TILE - 1 - i - k wins."""
    def make():
        base = PC.lane_case(which)
        mats = [P.Matrix("ACGTN", [[-3.0, 1.0, 0.25, -1.5, 0.5]]), P.Matrix("ACGTN", [[-3.0, 1.0, 0.25, -1.5, 1.0]])]
        case = dict(base, mats=mats, strands=[1] * len(base["track_of"]), runs=({},), name="lanes", do_masks=(True,))
        want = PS.MODEL.best(case["seqs"], mats, case["track_of"], case["starts"], case["strands"], case["lengths"])
        w, k = np.asarray(base["which"]), np.asarray(base["step"])
        assert np.array_equal(want[1][0], TILE - 1 - w) and np.array_equal(want[1][1], TILE - 1 - w - k) and (want[0] == 1).all() and (k > 0).any()
        return case
    return made_once(("lanes", tuple(which)), make)


def long_row_case(tiles=5):
    """pwm_cases.long_row_case: one MINUS row of more tiles than a grid of two, between short rows; under the zeros matrix every
    offset ties and the first scoreable one OF THE STRAND'S STRING wins; the planted motif's complement stands at both ends"""
    def make():
        base = PC.long_row_case(tiles)
        return dict(base, strands=[0, 1, 1, 1, 0], runs=(), best_runs=({"grid": 2}, {"grid": 2, "slack": 7 * TILE + 5}), hits_runs=({"grid": 2},),
                    name="long row", do_masks=(True,))
    return made_once(("long", tiles), make)


def many_rows_case(rows=2500):
    """2 500 rows of 0 or 1 bases in ONE tile, a random half minus, under the recorded one-row matrix over ACGTacgt and a width-4 one"""
    def make():
        rng = np.random.default_rng(630)
        seq = PC.sparse_sequence(rng, 20_000)
        lengths = (rng.random(rows) < 0.38).astype(np.int64)
        assert 800 < lengths.sum() <= TILE
        starts = rng.integers(-3, seq.size + 3, rows)
        return dict(seqs=[seq], mats=[P.matrix("w1lc"), P.matrix("w20lc")], track_of=[0] * rows, starts=starts.tolist(), lengths=lengths.tolist(),
                    strands=rng.integers(0, 2, rows).tolist(), runs=({},), name="many rows")
    return made_once(("many", rows), make)


def palindrome_case():
    """a row that is its own reverse complement under a random matrix and its reverse complement: the minus planes ARE the plus
    planes; beside it a row that is not"""
    def make():
        rng = np.random.default_rng(640)
        half = "".join("ACGT"[i] for i in rng.integers(0, 4, 40))
        text = "ACCGTTGA" + half + S.reverse_complement_str(half) + "TTGACAAC"
        seq = K.sequence_of(len(text), [], [], [], [], SC.pack(text))
        mat = PC.random_matrix_set(rng, (7,), 4, "acgt")[0]
        case = case_of([seq], [mat, mat.reverse_complement()], [(0, 8, 80, 1), (0, 8, 80, 0), (0, 0, 50, 1), (0, 0, 50, 0)], runs=({},), name="palindrome",
                       do_masks=(True,))
        got = PS.MODEL.scores([seq], case["mats"], case["track_of"], case["starts"], case["strands"], case["lengths"])
        assert np.array_equal(P.bits(got[:, :80]), P.bits(got[:, 80:160])) and not np.array_equal(P.bits(got[:, 160:210]), P.bits(got[:, 210:]))
        return case
    return made_once("palindrome", make)


def small_top_case():
    """pwm_cases.small_top_case: the phases of the top of int32 on 2^15 - 1 bases, every row once on each strand"""
    def make():
        base = PC.small_top_case()
        n = len(base["track_of"])
        both = {k: np.concatenate([base[k], base[k]]) for k in ("track_of", "starts", "lengths")}
        return dict(base, **both, strands=[1] * n + [0] * n, runs=({},), name="small top")
    return made_once("small top", make)


# ---- the comparison ----
def rows_of(case):
    n = len(case["track_of"])
    return case.get("lengths"), case.get("width", 0), n


def want_of(case, do_mask):
    """(sums, scoreable, offsets, best, plus planes) of the model, once per case and setting"""
    key = ("want", bool(do_mask))
    if key not in case:
        lengths, width, n = rows_of(case)
        texts = case.get("texts")
        rows = None
        if texts is not None:  # (sequences with a model of their own)
            rows = [S.reverse_complement(r) if m else r for r, m in zip(texts[do_mask], case["strands"])]
        acc, ok, offsets = PS.MODEL.planes(case["seqs"], case["mats"], case["track_of"], case["starts"], case["strands"], lengths, width, do_mask, rows)
        plus = PC.MODEL.planes(case["seqs"], case["mats"], case["track_of"], case["starts"], lengths, width, do_mask, texts and texts[do_mask])
        want, there = np.where(ok, acc, P.NAN), np.where(plus[1], plus[0], P.NAN)
        assert not np.array_equal(P.bits(want), P.bits(there)), "the strands change nothing"
        for i, minus in enumerate(case["strands"]):  # a plus row of a mixed batch is the unstranded row
            if not minus:
                assert np.array_equal(P.bits(want[:, offsets[i]:offsets[i + 1]]), P.bits(there[:, offsets[i]:offsets[i + 1]]))
        for a in (acc, ok):
            a.setflags(write=False)
        case[key] = acc, ok, offsets, PC.MODEL.best_of_planes(acc, ok, offsets), (plus[0], plus[1])
    return case[key]


def thresholds_of(case, do_mask):
    acc, ok, _, _, _ = want_of(case, do_mask)
    return (-INF, H.occurring(np.where(ok & ~np.isnan(acc), acc, P.NAN)), INF)


def check(devices, case, planes=True, best=True, hits=True, where=""):
    lengths, width, n = rows_of(case)
    kw = dict(lengths=lengths, width=width)
    args = (case["seqs"], case["mats"], case["track_of"], case["starts"])
    zeros = [0] * n
    where = where or case.get("name", "")
    for do_mask in case.get("do_masks", (True, False)):
        acc, ok, offsets, top, plus = want_of(case, do_mask)
        for dev in devices:
            who = (where, type(dev).__name__, do_mask)
            for run in case["runs"] if planes else ():
                PC.assert_planes(dev.scores(*args, case["strands"], do_mask=do_mask, **kw, **run), acc, ok, who + (run,))
            if planes and case["runs"]:  # a strand array of zeros, the unstranded form and the model's plus rows: bit for bit
                all_plus = dev.scores(*args, zeros, do_mask=do_mask, **kw)
                unstranded = dev.scores(*args, None, do_mask=do_mask, **kw)
                PC.assert_planes(unstranded, plus[0], plus[1], who + ("unstranded",))
                assert all_plus.tobytes() == unstranded.tobytes(), who + ("zeros",)
            for run in case.get("best_runs", ({},)) if best else ():
                PC.assert_best(dev.best(*args, case["strands"], do_mask=do_mask, **kw, **run), top, who + ("best", run))
            for run in case.get("hits_runs", ({},)) if hits else ():
                for t in thresholds_of(case, do_mask):
                    want = H.expected(np.where(ok, acc, P.NAN), offsets, t, ok)
                    got = dev.hits(*args, case["strands"], t, do_mask=do_mask, **kw, **run)
                    H.assert_hits(got, want, who + ("hits", run))
                    # ascending in (matrix, row, offset of the strand's string)
                    for m in range(len(case["mats"])):
                        part = slice(got[0][m], got[0][m + 1])
                        key = got[1][part].astype(np.int64) * (1 << 32) + got[2][part]
                        assert (np.diff(key) > 0).all(), who + ("order",)
