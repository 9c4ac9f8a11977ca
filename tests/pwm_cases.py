"""
Seeded matrices, sequences and rows for tests/test_pwm_kernel_host.py and tests/test_gpu_pwm.py (a helper: no tests here, no GPU),
modelled on tests/twobit_cases.py.  tests/test_pwm_cases.py pins the model below to tests/pwm_model.py and to a scalar transcription
of the reference's loop, checks what every generator promises, and shows that a stand-in "device" -- the model with one deliberate
change -- fails the case made for it.

  Model               the two contracts over a whole batch at once: all rows concatenated, one float32 chain per matrix position over
                      the whole text (every element's own chain in ascending j, as pwm_model.Matrix.score), windows that pass their
                      row's end struck out afterwards.  It keeps the sum and whether the window is scoreable apart, so that an
                      ARITHMETIC NaN (inf - inf, a NaN entry: scoreable, the sum a NaN) is told from an unscoreable window.
                      Model(descending=True) and its like are the stand-ins.
  random_matrix_set   matrices of mixed magnitudes over an alphabet of up to 16 columns; asserted: the order of the additions shows
  matrix_set_case     the named sets around PW_LDS_VALUES, of 16 columns, of PW_MATS_MAX matrices, each over ragged rows
  extremes_case       negative, denormal, +inf, inf - inf and NaN matrices in one handle
  lane_case           1024 rows of one tile, the greatest score of row i at offset i; a second matrix under which i and i + k tie
  long_row_case       one row of many tiles: every offset ties, or the greatest score at the far end and its equal at the near end
  many_rows_case      the same total in a few thousand rows
  top_rows            rows at the top of twobit_cases.TopSequence, and a small sequence with the same phases for the host program
"""
import numpy as np

import pwm_model as P
import twobit_cases as K
import twobit_model as M
from pwm_model import COLS_MAX, MATS_MAX, NAN, TILE, WIDTH_MAX

LDS_VALUES = WIDTH_MAX * COLS_MAX  # PW_LDS_VALUES of csrc/pwm.hpp
FILLERS = "#$%&*+-./0123456789:;<=>?@BDEFHIJKLMOPQRSUVWXYZ"  # columns no base selects; all sort below 'a'
ALPHABETS = {"all": "TCAGNtcagn",   # every letter class has a column
             "no_n": "TCAGtcag",    # N and n have none
             "upper": "TCAGN",      # only upper case has one
             "g_top": "TCAGNcag",   # t and n have none: with 16 columns g is the last one
             "n_top": "TCAGNcagn",  # t has none: n is the last one
             "mixed": "CGNtcan",    # T and A only in lower case, G only in upper case
             "acgt": "TCAG"}
TIE_STEPS = (1, 3, 4, 63, 64, 65, 255, 256)
_cases = {}


# ---- the model of a batch ----
def chain(values, index, text, descending=False):
    """(float32 [n], bool [n]) for uint8 letters `text`: the sum ((0 + v[0][c0]) + v[1][c1]) + ... of the window at every offset --
    where a letter has no column its term is left out -- and whether every letter of the window has a column and the window ends
    inside the text.  descending: the same terms from the last to the first."""
    text = np.asarray(text, dtype=np.uint8)
    n, w = len(text), values.shape[0]
    col = np.concatenate([index[text], np.full(w, -1, dtype=np.int16)]).astype(np.intp)
    padded = np.concatenate([values, np.zeros((w, 1), dtype=np.float32)], axis=1)  # column -1: +0.0, which changes no sum that began at +0.0
    without = np.concatenate([[0], np.cumsum(col < 0)])
    ok = without[w:w + n] == without[:n]  # no letter of [i, i + w) lacks a column
    acc = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in (range(w - 1, -1, -1) if descending else range(w)):
            acc = acc + padded[j][col[j:j + n]]
    assert acc.dtype == np.float32
    return acc, ok


_letters = {}


def letters_of(seqs):
    key = tuple(id(s) for s in seqs)
    if key not in _letters:
        _letters[key] = (list(seqs), P.Scores(seqs))
    return _letters[key][1]


class Model:
    """scores / best of a batch as a device under test gives them.  Without arguments the model; with one, a stand-in:
      descending    every sum in descending j
      last_wins     of equal greatest scores the last offset
      nan_greatest  an arithmetic NaN is the greatest score
      short_halo    the halo one column short: the widest matrices leave out their last column at the last element of a segment
      four_bits     the column of a letter looked up in 4 bits of the packed argument: column 15 reads as no column"""

    def __init__(self, descending=False, last_wins=False, nan_greatest=False, short_halo=False, four_bits=False):
        self.descending, self.last_wins, self.nan_greatest, self.short_halo, self.four_bits = descending, last_wins, nan_greatest, short_halo, four_bits

    def planes(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True, texts=None):
        """(sums float32 [n_mats, total], scoreable bool [n_mats, total], offsets int64 [n + 1]); texts: the rows' letters, when
        the sequences have a model of their own"""
        n = len(track_of)
        lengths = [width] * n if lengths is None else lengths
        if texts is None:
            texts = letters_of(seqs).rows(track_of, starts, lengths, do_mask)
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in texts])]).astype(np.int64)
        total = int(offsets[-1])
        text = np.concatenate(texts) if n else np.zeros(0, dtype=np.uint8)
        left = np.repeat(offsets[1:], np.diff(offsets)) - np.arange(total)  # elements from this one to its row's end
        widest = max(m.width for m in mats)
        acc, ok = np.zeros((len(mats), total), dtype=np.float32), np.zeros((len(mats), total), dtype=bool)
        for m, mat in enumerate(mats):
            index = mat.char_to_index
            if self.four_bits:
                index = np.where(index >= 15, -1, index).astype(np.int16)
            acc[m], ok[m] = chain(mat.values, index, text, self.descending)
            ok[m] &= left >= mat.width
            if self.short_halo and mat.width == widest:
                ends = (np.arange(total) % TILE == TILE - 1) | (left == 1)  # the last element of a segment
                a, k = chain(mat.values[:-1], index, text, self.descending)
                acc[m, ends], ok[m, ends] = a[ends], (k & (left >= mat.width - 1))[ends]
        return acc, ok, offsets

    def scores(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True, texts=None):
        acc, ok, _ = self.planes(seqs, mats, track_of, starts, lengths, width, do_mask, texts)
        return np.where(ok, acc, NAN)

    def best_of_planes(self, acc, ok, offsets):
        n = len(offsets) - 1
        score, pos = np.full((len(acc), n), NAN, dtype=np.float32), np.full((len(acc), n), -1, dtype=np.int32)
        for m in range(len(acc)):
            for i in range(n):
                a, k = acc[m, offsets[i]:offsets[i + 1]], ok[m, offsets[i]:offsets[i + 1]]
                nans = k & np.isnan(a)
                if self.nan_greatest and nans.any():
                    pos[m, i] = np.flatnonzero(nans)[0]
                    continue
                cand = k & ~nans
                if cand.any():
                    score[m, i] = a[cand].max()
                    at = np.flatnonzero(cand & (a == score[m, i]))
                    pos[m, i] = at[-1] if self.last_wins else at[0]
        return score, pos

    def best(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True, texts=None, **_):
        return self.best_of_planes(*self.planes(seqs, mats, track_of, starts, lengths, width, do_mask, texts))


MODEL = Model()


# ---- the comparison ----
def assert_planes(got, acc, ok, where=""):
    """bit for bit, except where the model has an arithmetic NaN -- a NaN in a window that has all its columns and lies in its row
    -- where the device's element must be a NaN, of whatever sign and payload; a NaN of an unscoreable window is 0x7FC00000"""
    arith = ok & np.isnan(acc)
    want = np.where(ok, acc, NAN)
    assert got.shape == want.shape and got.dtype == np.float32, (where, got.shape, want.shape)
    assert np.isnan(got[arith]).all(), (where, "an arithmetic NaN of the model is a number")
    bad = (P.bits(got) != P.bits(want)) & ~arith
    assert not bad.any(), (where, int(bad.sum()), [(int(m), int(e)) for m, e in zip(*np.nonzero(bad))][:8])


def assert_best(got, want, where=""):
    """exactly: an arithmetic NaN is never a candidate, so no best score is one"""
    bad = (P.bits(got[0]) != P.bits(want[0])) | (got[1] != want[1])
    assert got[0].shape == want[0].shape and got[1].dtype == np.int32 and not bad.any(), \
        (where, [(int(m), int(i), float(got[0][m, i]), int(got[1][m, i]), float(want[0][m, i]), int(want[1][m, i])) for m, i in zip(*np.nonzero(bad))][:8])


def check_batch(devs, case, do_masks=(True, False), planes=True, best=True, where="", best_args=({},)):
    """a case through every device of `devs` -- objects with Model's scores and best -- against the model, computed once;
    best_args: the best hits are asked for once with each of these keyword arguments"""
    seqs, mats, t, s, n = case["seqs"], case["mats"], case["track_of"], case["starts"], case["lengths"]
    texts = case.get("texts")
    for do_mask in do_masks:
        acc, ok, offsets = MODEL.planes(seqs, mats, t, s, n, do_mask=do_mask, texts=texts and texts[do_mask])
        want = MODEL.best_of_planes(acc, ok, offsets)
        for k, dev in enumerate(devs):
            if planes:
                assert_planes(dev.scores(seqs, mats, t, s, lengths=n, do_mask=do_mask), acc, ok, (where, do_mask, k, "scores"))
            for args in best_args if best else ():
                assert_best(dev.best(seqs, mats, t, s, lengths=n, do_mask=do_mask, **args), want, (where, do_mask, k, "best", args))
    width = case.get("matrix_width", 0)
    if width and planes:  # as windows of one width
        acc, ok, _ = MODEL.planes(seqs, mats, t, s, width=width)
        for k, dev in enumerate(devs):
            assert_planes(dev.scores(seqs, mats, t, s, width=width), acc, ok, (where, k, "score_matrix"))


# ---- random matrices ----
def order_share(mats, text):
    """the share of the scoreable windows of `text`, under the matrices of at least three rows (a + b = b + a: two terms have no
    order), whose float32 sum in descending j differs in bits from the sum in ascending j"""
    differ = scored = 0
    for mat in mats:
        if mat.width >= 3:
            up, ok = chain(mat.values, mat.char_to_index, text)
            down, _ = chain(mat.values, mat.char_to_index, text, descending=True)
            differ += int((ok & (P.bits(up) != P.bits(down))).sum())
            scored += int(ok.sum())
    return differ / max(scored, 1)


def random_matrix_set(rng, widths, n_cols, kind="all", sample=None, share=0.25):
    """len(widths) matrices over one alphabet of n_cols columns: the letters of ALPHABETS[kind] and fillers that sort below the last of them, in random order (the
    columns are the sorted alphabet's).  The values are normals scaled by 2^k, k uniform in -12 .. 12, so that a float32 sum
    depends on its order: asserted on `sample` (uint8 letters the matrices will score).  With 16 columns the last column must be
    one a base can select: the top bits of the packed letter_col argument are then in use."""
    letters = ALPHABETS[kind]
    assert len(letters) <= n_cols <= COLS_MAX
    alphabet = list(letters) + [str(c) for c in rng.choice([c for c in FILLERS if c < max(letters)], n_cols - len(letters), replace=False)]
    alphabet = [alphabet[i] for i in rng.permutation(n_cols)]
    mats = [P.Matrix(alphabet, (rng.normal(size=(w, n_cols)) * 2.0 ** rng.integers(-12, 13, (w, n_cols))).astype(np.float32)) for w in widths]
    if n_cols == COLS_MAX:
        assert mats[0].sorted_alphabet[-1] in P.LETTERS
    if sample is not None and any(w >= 3 for w in widths):
        got = order_share(mats, sample)
        assert got >= share, (kind, widths, got)
    return mats


def top_classes(mats):
    """the letter classes (indices into TCAGNtcagn) whose column is 15"""
    return [k for k, ch in enumerate(P.LETTERS) if mats[0].char_to_index[ord(ch)] == 15]


def ragged_rows(rng, sizes, n, longest, widest):
    """n rows over sequences of `sizes`: lengths log-uniform in 0 .. longest, a fifth of 0 .. 2, rows of widest - 1, widest and
    widest + 1, starts from -50 to size + 50, rows that name no sequence, the total a multiple of 4 plus 1"""
    track_of = rng.integers(0, len(sizes), n)
    track_of[rng.random(n) < 0.6] = 0
    track_of[rng.integers(0, n, 3)] = -1
    size_of = np.array(list(sizes) + [0])[track_of]
    lengths = K.log_uniform(rng, 1, longest + 1, n) - 1
    short = rng.random(n) < 0.2
    lengths[short] = rng.integers(0, 3, int(short.sum()))
    starts = rng.integers(-50, np.maximum(size_of - lengths // 2, 0) + 51)
    track_of[:8] = 0
    lengths[:5] = (longest, widest - 1, widest, widest + 1, 0)
    starts[:5] = (sizes[0] // 3, 100, 700, 1300, 5)
    starts[6:8], lengths[6:8] = (-30, sizes[0] - 10), (widest + 40, 60)  # across either end of the sequence
    size_of = np.array(list(sizes) + [0])[track_of]
    lengths[5] += (1 - lengths.sum()) % 4
    assert lengths.min() == 0 and starts.min() < 0 and ((starts + lengths > size_of) & (track_of >= 0)).any() and lengths.sum() % 4 == 1
    return track_of, starts, lengths


def sparse_sequence(rng, size):
    """random bases under twobit_cases.random_blocks of at most 400 bases, sparse enough that windows of 256 plain bases are there"""
    blocks = K.random_blocks(rng, size, max(size // 2000, 8), 400) + K.random_blocks(rng, size, max(size // 1000, 12), 400)
    return K.sequence_of(size, *blocks, rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8))


MATRIX_SETS = {  # name: (widths, columns, alphabet)
    "lds_4x256x4": ((256,) * 4, 4, "acgt"),          # exactly PW_LDS_VALUES values
    "lds_256x16": ((256,), 16, "n_top"),              # the same in the largest single matrix
    "lds_plus_4": ((256,) * 4 + (1,), 4, "acgt"),    # PW_LDS_VALUES + n_cols: the smallest set staged matrix by matrix
    "lds_plus_16": ((256, 1), 16, "g_top"),
    "mats_max": (None, 16, "all"),                   # PW_MATS_MAX matrices of 1 .. 256 rows
    "cols16_all": ((7, 20, 33), 16, "all"),
    "cols16_g_top": ((20, 3), 16, "g_top"),
    "cols16_no_n": ((5, 20), 16, "no_n"),
    "cols16_upper": ((20, 9), 16, "upper"),
    "cols16_mixed": ((6, 20), 16, "mixed"),
}


def matrix_set_case(name, n_rows=100, size=300_000, longest=8000):
    """MATRIX_SETS[name] over n_rows ragged rows of two random sequences (the second of 1025 bases) and as windows of one width"""
    key = (name, n_rows, size, longest)
    if key in _cases:
        return _cases[key]
    widths, n_cols, kind = MATRIX_SETS[name]
    rng = np.random.default_rng(500 + sorted(MATRIX_SETS).index(name))
    if widths is None:  # the halo comes from one matrix, which is not the first; most are far narrower
        widths = [int(w) for w in K.log_uniform(rng, 1, 40, MATS_MAX)]
        widths[0], widths[3], widths[11] = 1, 2, WIDTH_MAX
        assert len(widths) == MATS_MAX and sorted(widths)[-2] <= 40 and np.median(widths) < 20
    seqs = [sparse_sequence(rng, size), K.random_sequence(rng, 1025, 3, 5)]
    track_of, starts, lengths = ragged_rows(rng, [s.size for s in seqs], n_rows, longest, max(widths))
    sample = np.concatenate(letters_of(seqs).rows(track_of, starts, lengths, True))
    mats = random_matrix_set(rng, widths, n_cols, kind, sample)
    values = sum(m.width for m in mats) * n_cols
    if name.startswith("lds_plus"):
        assert values == LDS_VALUES + n_cols
    elif name.startswith("lds_"):
        assert values == LDS_VALUES
    case = dict(seqs=seqs, mats=mats, track_of=track_of, starts=starts, lengths=lengths, matrix_width=max(widths) + 44)
    acc, ok, _ = MODEL.planes(seqs, mats, track_of, starts, lengths)
    assert ok.any(axis=1).all() and not ok.all(axis=1).any()  # every matrix scores something and not everything
    _cases[key] = case
    return case


def sixteen_column_classes():
    """the letter classes that select column 15 in some set of MATRIX_SETS: g (8) and n (9) among them"""
    out = set()
    for name, (_, n_cols, _) in MATRIX_SETS.items():
        if n_cols == COLS_MAX:
            out.update(top_classes(matrix_set_case(name, 40, 20_000, 3000)["mats"]))
    assert {8, 9} <= out, out
    return out


# ---- extremes ----
def is_denormal(x):
    return (x != 0) & (np.abs(x) < np.float32(1.17549435e-38))


def extremes_case(n_rows=100, size=30_000, longest=3000):
    """One handle over ACGT: all-negative finite values; the recorded denormals, and three rows of them scaled down; +inf in some cells; +inf and -inf, so that some
    windows sum to inf - inf; one NaN entry.  Ragged rows of a random sequence, and rows of one window that sums to -inf.
    Asserted on the model: among the best scores are a negative finite one, a denormal, +inf and -inf, and the greatest score of
    some row lies next to an arithmetic NaN."""
    key = ("extremes", n_rows, size, longest)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(520)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    neg = -(np.abs(rng.normal(size=(5, 4))) + 0.125)
    pinf = rng.normal(size=(4, 4))
    pinf[1, 1] = pinf[3, 0] = inf
    both = rng.normal(size=(3, 4))
    both[0, 0], both[1, 1] = inf, -inf  # A..: +inf, .C.: -inf, AC.: NaN
    nan1 = rng.normal(size=(4, 4))
    nan1[2, 2] = nan
    tiny = P.matrix("denorm").values[:3] * np.float32(0.25)  # three of them still sum to a denormal
    mats = [P.Matrix("ACGT", neg), P.matrix("denorm"), P.Matrix("ACGT", tiny), P.Matrix("ACGT", pinf), P.Matrix("ACGT", both), P.Matrix("ACGT", nan1)]
    seq = sparse_sequence(rng, size)
    track_of, starts, lengths = ragged_rows(rng, [seq.size], n_rows, longest, 5)
    whole = M.letters(seq, True)
    one = np.flatnonzero(np.isin(whole[:-2], list(b"CGT")) & (whole[1:-1] == ord("C")) & np.isin(whole[2:], list(b"ACGT")))[:3]  # .C. without A
    assert len(one) == 3
    track_of, starts, lengths = np.concatenate([track_of, [0] * 3]), np.concatenate([starts, one]), np.concatenate([lengths, [3] * 3])
    case = dict(seqs=[seq], mats=mats, track_of=track_of, starts=starts, lengths=lengths)
    for do_mask in (True, False):
        acc, ok, offsets = MODEL.planes([seq], mats, track_of, starts, lengths, do_mask=do_mask)
        score, pos = MODEL.best_of_planes(acc, ok, offsets)
        assert not np.isnan(score[pos >= 0]).any()
        assert (score[0][pos[0] >= 0] < 0).all() and np.isfinite(score[0][pos[0] >= 0]).all() and (pos[0] >= 0).sum() > n_rows // 4
        assert is_denormal(score[2]).any() and np.isposinf(score[3]).any() and np.isposinf(score[4]).any() and np.isneginf(score[4]).any()
        arith = ok & np.isnan(acc)
        assert arith[4].any() and arith[5].any() and not arith[:4].any()
        beside = 0
        for m in (4, 5):
            for i in np.flatnonzero(pos[m] >= 0):
                at = offsets[i] + pos[m, i]
                beside += bool(arith[m, max(at - 1, offsets[i])] or arith[m, min(at + 1, offsets[i + 1] - 1)])
        assert beside >= 1, beside
    _cases[key] = case
    return case


# ---- every lane, every element ----
def lane_case(which=None):
    """One sequence of 1024 x 1024 bases without G but for one in every stretch of 1024: stretch i has its G at offset i, and a
    one-base N block at offset i + k, k = TIE_STEPS[i % 8] (the next one that fits, none in the last stretch).  Row i is stretch i:
    one tile.  Two matrices of one row over ACGTN: under the first G scores highest, alone; under the second G and N tie.
    which: the rows taken (all 1024)."""
    if "lane" not in _cases:
        rng = np.random.default_rng(530)
        size = TILE * TILE
        codes = rng.integers(0, 3, size).astype(np.uint8)  # T C A
        i = np.arange(TILE)
        codes[i * TILE + i] = 3
        step = np.zeros(TILE, dtype=np.int64)
        for r in range(TILE - 1):
            step[r] = next(k for k in TIE_STEPS[r % 8:] + TIE_STEPS if r + k < TILE)
        tied = step > 0
        quads = codes.reshape(-1, 4)
        packed = (quads[:, 0] << 6) | (quads[:, 1] << 4) | (quads[:, 2] << 2) | quads[:, 3]
        seq = K.sequence_of(size, (i * TILE + i + step)[tied], np.ones(int(tied.sum()), dtype=np.int64), [], [], packed)
        mats = [P.Matrix("ACGTN", [[-1.5, 0.25, 1.0, -3.0, 0.5]]), P.Matrix("ACGTN", [[-1.5, 0.25, 1.0, -3.0, 1.0]])]
        _cases["lane"] = (seq, mats, step)
    seq, mats, step = _cases["lane"]
    which = np.arange(TILE) if which is None else np.asarray(which, dtype=np.int64)
    case = dict(seqs=[seq], mats=mats, track_of=np.zeros(len(which), dtype=np.int64), starts=which * TILE, lengths=np.full(len(which), TILE), step=step[which],
                which=which)
    key = ("lane checked", tuple(which.tolist()))
    if key not in _cases:
        acc, ok, offsets = MODEL.planes(**{k: case[k] for k in ("seqs", "mats", "track_of", "starts", "lengths")})
        score, pos = MODEL.best_of_planes(acc, ok, offsets)
        assert ok.all() and np.array_equal(pos[0], which) and np.array_equal(pos[1], which) and (score == 1).all()
        rows = acc.reshape(2, len(which), TILE)
        assert ((rows[0] == 1).sum(axis=1) == 1).all()  # alone under the first matrix
        has = case["step"] > 0
        assert ((rows[1] == 1).sum(axis=1) == 1 + has).all() and (rows[1][np.flatnonzero(has), (which + case["step"])[has]] == 1).all()
        _cases[key] = True
    return case


LANE_SAMPLE = (0, 1, 2, 3, 4, 5, 62, 63, 64, 65, 191, 192, 252, 255, 256, 257, 510, 511, 512, 767, 768, 769, 771, 1020, 1021, 1022, 1023)
# (for the host program: every element of a thread, the first and last lane of every wave; offsets 4 t + q are thread t's element q)


# ---- rows longer than a grid fill ----
def plant(packed, at, codes):
    for k, c in enumerate(codes):
        byte, shift = (at + k) // 4, 6 - 2 * ((at + k) % 4)
        packed[byte] = (int(packed[byte]) & ~(3 << shift)) | (int(c) << shift)


def long_row_case(tiles):
    """One row of tiles * PW_TILE + 37 elements from position 0 of a random sequence -- which begins inside an N block -- between
    short rows and an empty one.  Two matrices over ACGT: the recorded zeros, under which every scoreable offset ties, so the first
    one wins; and a random one of 16 rows whose highest-scoring string is planted in the first and in the last tenth of the row
    and stands nowhere else: the greatest score in the far end, its equal in the near end."""
    key = ("long", tiles)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(540)
    length = tiles * TILE + 37
    size = length + 300
    blocks = K.random_blocks(rng, size, max(size // 3000, 4), 200) + K.random_blocks(rng, size, max(size // 1500, 6), 200)
    draft = K.sequence_of(size, *blocks, rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8))
    assert draft.n_starts[0] == 0
    values = rng.normal(size=(16, 4)).astype(np.float32)
    rnd = P.Matrix("ACGT", values)
    motif = [b"TCAG".index(b"ACGT"[c]) for c in rnd.values.argmax(axis=1)]  # 2bit codes of the string
    whole = M.letters(draft, True)
    clear = np.convolve(np.isin(whole, list(b"ACGT")), np.ones(16, dtype=np.int64))[15:] == 16  # 16 plain bases from here on
    near = int(np.flatnonzero(clear[length // 20:])[0]) + length // 20
    far = int(np.flatnonzero(clear[length - length // 20:length - 16])[0]) + length - length // 20
    packed = np.array(draft.packed, dtype=np.uint8)
    plant(packed, near, motif), plant(packed, far, motif)
    seq = K.sequence_of(size, draft.n_starts, draft.n_sizes, draft.m_starts, draft.m_sizes, packed)
    mats = [P.matrix("zeros"), rnd]
    case = dict(seqs=[seq], mats=mats, track_of=np.array([0, 0, 0, 0, 0]), starts=np.array([5, 300, 0, 9, 77]), lengths=np.array([300, 3, length, 0, 41]),
                near=near, far=far)
    acc, ok, offsets = MODEL.planes(case["seqs"], mats, case["track_of"], case["starts"], case["lengths"])
    score, pos = MODEL.best_of_planes(acc, ok, offsets)
    row = slice(offsets[2], offsets[3])
    assert pos[0, 2] == np.flatnonzero(ok[0, row])[0] > 0 and score[0, 2] == 0 and ok[0, row].sum() > length // 10
    top = np.flatnonzero(ok[1, row] & (acc[1, row] == score[1, 2]))
    assert top.tolist() == [near, far] and pos[1, 2] == near < length // 10 and far > length - length // 10
    _cases[key] = case
    return case


def many_rows_case(tiles):
    """a few thousand rows, log-uniform up to 6000 elements (a quarter of the total, if that is less), of the sequence of long_row_case(tiles), in all tiles * PW_TILE + 37
    elements: the tiles a workgroup takes on its second trip begin inside rows and hold several segments"""
    key = ("many", tiles)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(541)
    base = long_row_case(tiles)
    seq, total = base["seqs"][0], tiles * TILE + 37
    longest = min(6000, total // 4)
    lengths = K.log_uniform(rng, 1, longest + 1, 40 * total // longest + 50) - 1
    lengths[1] = 0
    n = int(np.searchsorted(np.cumsum(lengths), total)) + 1
    lengths = lengths[:n]
    lengths[-1] -= lengths.sum() - total
    assert lengths.sum() == total and lengths.min() == 0 and n > total // 1000
    starts = rng.integers(-20, seq.size - lengths // 2)
    case = dict(seqs=[seq], mats=base["mats"], track_of=np.zeros(n, dtype=np.int64), starts=starts, lengths=lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    cuts = np.arange(1, tiles) * TILE
    assert (np.isin(cuts, offsets).mean() < 0.05) and len(offsets) > 1.2 * tiles  # a tile begins mid-row and holds more than one segment
    _cases[key] = case
    return case


# ---- the top of int32 ----
def top_rows(size, n_block, mask_block, widths=(20, 256)):
    """[(start, length)] around the end of a sequence of `size` bases and the edges of two blocks: rows that end at the size, cross
    it, of W - 1, W and W + 1 bases ending at it, across both edges of either block, a row from the last base and one from the size"""
    rows = [(size - 3000, 3000), (size - 100, 300), (size - 1, 50), (size, 50), (size - 2 * TILE - 7, 2 * TILE + 7)]
    for w in widths:
        rows += [(size - w + 1, w - 1), (size - w, w), (size - w - 1, w + 1), (size - w, w + 9)]
    for edge in tuple(n_block) + tuple(mask_block):
        rows.append((edge - 300, 600))
    return rows


def top_case():
    """top_rows on twobit_cases.TopSequence (and a row across the middle window), its letters from TopSequence's own model; two
    matrices of 20 and 256 rows over all ten letters in 16 columns"""
    if "top" not in _cases:
        top = K.top_sequence()
        rows = top_rows(top.size, K.TOP_N, K.TOP_MASK) + [((1 << 30) - 500, 1000)]
        starts, lengths = (np.array(x, dtype=np.int64) for x in zip(*rows))
        assert starts.max() == top.size and (starts + lengths).max() > 2 ** 31 and starts.max() < 2 ** 31
        texts = {do_mask: [top.row(int(s), int(n), do_mask, 0) for s, n in rows] for do_mask in (True, False)}
        mats = random_matrix_set(np.random.default_rng(550), (20, 256), 16, "all", np.concatenate(texts[True]))
        _cases["top"] = dict(seqs=[top.seq], mats=mats, track_of=np.zeros(len(rows), dtype=np.int64), starts=starts, lengths=lengths, texts=texts)
    return _cases["top"]


SMALL_TOP = 2 ** 15 - 1  # the same phase as 2^31 - 1 in a packed word, a thread's 8 columns and a tile


def small_top_case():
    """the same rows on a sequence of 2^15 - 1 bases whose blocks' edges have the phases of TopSequence's, for the host program"""
    if "small top" not in _cases:
        size = SMALL_TOP
        rng = np.random.default_rng(551)
        n_block, mask_block = (1 << 13, (1 << 13) + (1 << 12)), (5000, size - 9000)
        assert all(a % 16 == b % 16 for a, b in zip((size,) + n_block + mask_block, (K.TOP_SIZE,) + K.TOP_N + K.TOP_MASK))
        n = [(0, 3), n_block, (size - 8190, size - 8100), (size - 20, size - 10)]
        m = [(10, 20), mask_block, (size - 8000, size - 7990), (size - 4097, size - 4095), (size - 5, size)]
        seq = K.sequence_of(size, [a for a, _ in n], [b - a for a, b in n], [a for a, _ in m], [b - a for a, b in m], rng.integers(0, 256, (size + 3) // 4, dtype=np.uint8))
        rows = top_rows(size, n_block, mask_block)
        starts, lengths = (np.array(x, dtype=np.int64) for x in zip(*rows))
        sample = np.concatenate(letters_of([seq]).rows([0] * len(rows), starts, lengths, True))
        mats = random_matrix_set(rng, (20, 256), 16, "all", sample)
        _cases["small top"] = dict(seqs=[seq], mats=mats, track_of=np.zeros(len(rows), dtype=np.int64), starts=starts, lengths=lengths)
    return _cases["small top"]
