"""CPU-only: the batch model of tests/pwm_cases.py agrees with tests/pwm_model.py (which tests/test_pwm_model_golden.py pins to the
reference's recordings) and with a scalar transcription of the reference's loop -- the second, independent statement of the contract
that the random matrices need, since no recording covers them; the seeded cases hold what they promise; and a stand-in "device", the
model with one deliberate change, fails the case made to catch that change."""
import numpy as np
import pytest

import pwm_cases as PC
import pwm_model as P

TILES = 5  # of the long rows here; the device test takes more than a grid fill


def scalar_score(mat, text, at):
    """the reference's loop for one offset, one float32 at a time: 0.0, then for every position j of the matrix the value of the
    letter's column added, NaN as soon as a letter has none (or the window leaves the string)"""
    if at + mat.width > len(text):
        return P.NAN
    score = np.float32(0.0)
    with np.errstate(all="ignore"):
        for j in range(mat.width):
            index = int(mat.char_to_index[text[at + j]])
            if index < 0:
                return P.NAN
            score = np.float32(score + mat.values[j][index])
    return score


def batch(case):
    return case["seqs"], case["mats"], case["track_of"], case["starts"], case["lengths"]


def small_cases():
    out = {name: PC.matrix_set_case(name, 40, 20_000, 3000) for name in PC.MATRIX_SETS}
    out.update(extremes=PC.extremes_case(60, 20_000, 2000), lanes=PC.lane_case(PC.LANE_SAMPLE), long=PC.long_row_case(TILES), many=PC.many_rows_case(TILES),
               small_top=PC.small_top_case())
    return out


@pytest.mark.parametrize("name", sorted(PC.MATRIX_SETS) + ["extremes", "lanes", "long", "many", "small_top"])
def test_batch_model_is_the_row_model_and_the_scalar_loop(name):
    """Model.scores against pwm_model.Scores.scores (row by row, Matrix.score) on every case, both against the scalar loop on a few
    thousand sampled offsets of each; the best hits against pwm_model.best_of"""
    case = small_cases()[name]
    seqs, mats, t, s, n = batch(case)
    rng = np.random.default_rng(600)
    for do_mask in (True, False):
        got = PC.MODEL.scores(seqs, mats, t, s, n, do_mask=do_mask)
        rows = PC.letters_of(seqs).rows(t, s, n, do_mask)
        offsets = np.concatenate([[0], np.cumsum(n)])
        few = rng.choice(len(rows), min(len(rows), 60), replace=False)  # (the row model loops over rows and matrix positions)
        for i in few:
            for m, mat in enumerate(mats):
                assert np.array_equal(P.bits(got[m, offsets[i]:offsets[i + 1]]), P.bits(mat.score(rows[i]))), (name, do_mask, i, m)
        score, pos = PC.MODEL.best(seqs, mats, t, s, n, do_mask=do_mask)
        for i in few:
            for m in range(len(mats)):
                top, at = P.best_of(got[m, offsets[i]:offsets[i + 1]])
                assert P.bits(score[m, i]) == P.bits(top) and pos[m, i] == at, (name, do_mask, i, m)
        checked = 0
        scored = np.argwhere(~np.isnan(got))
        picks = [(int(rng.integers(len(mats))), int(rng.integers(got.shape[1]))) for _ in range(1500)] + scored[rng.integers(0, len(scored), 1500)].tolist()
        for m, e in picks:  # half of them anywhere, half where the model has a score
            i = int(np.searchsorted(offsets, e, side="right")) - 1
            want = scalar_score(mats[m], rows[i], e - int(offsets[i]))
            assert P.bits(got[m, e]) == P.bits(want) or (np.isnan(got[m, e]) and np.isnan(want) and P.bits(want) != P.NAN_BITS), (name, do_mask, i, m, e)
            checked += not np.isnan(want)
        assert checked > 1000, (name, checked)


def test_matrix_sets_are_what_their_names_say():
    for name, (widths, n_cols, kind) in PC.MATRIX_SETS.items():
        case = PC.matrix_set_case(name, 40, 20_000, 3000)
        mats = case["mats"]
        values = sum(m.width for m in mats) * n_cols
        assert all(m.values.shape[1] == n_cols for m in mats) and len({tuple(m.sorted_alphabet) for m in mats}) == 1
        assert set(P.LETTERS) & set(mats[0].alphabet) == set(PC.ALPHABETS[kind])
        if name in ("lds_4x256x4", "lds_256x16"):
            assert values == PC.LDS_VALUES
        if name.startswith("lds_plus"):
            assert values == PC.LDS_VALUES + n_cols and len(mats) >= 2
        if name == "mats_max":
            w = [m.width for m in mats]
            assert len(w) == P.MATS_MAX and max(w) == P.WIDTH_MAX and w.count(P.WIDTH_MAX) == 1 and w[0] != P.WIDTH_MAX and min(w) == 1 and np.median(w) < 20
        sample = np.concatenate(PC.letters_of(case["seqs"]).rows(case["track_of"], case["starts"], case["lengths"], True))
        assert PC.order_share(mats, sample) >= 0.25, name  # the order of the additions shows in a quarter of the scores
    assert PC.matrix_set_case("lds_256x16", 40, 20_000, 3000)["mats"][0].values.shape == (P.WIDTH_MAX, P.COLS_MAX)  # the largest single matrix
    assert {8, 9} <= PC.sixteen_column_classes()  # column 15 from g and from n: the top bits of the packed letters
    kinds = {kind for _, _, kind in PC.MATRIX_SETS.values()}
    assert {"all", "no_n", "upper"} <= kinds


def test_lane_case_covers_every_thread_and_element():
    case = PC.lane_case()
    score, pos = PC.MODEL.best(*batch(case))
    assert np.array_equal(pos[0], np.arange(P.TILE)) and np.array_equal(pos[1], np.arange(P.TILE)) and len(pos[0]) == 4 * P.THREADS
    assert (np.asarray(case["lengths"]) == P.TILE).all() and (np.asarray(case["starts"]) % P.TILE == 0).all()  # every row is one tile
    step, at = case["step"], np.arange(P.TILE)
    assert set(step[:-1].tolist()) == set(PC.TIE_STEPS) and step[-1] == 0
    both = step > 0
    same_thread = both & (at // 4 == (at + step) // 4)
    same_wave = both & ~same_thread & (at // 256 == (at + step) // 256)
    assert same_thread.sum() > 50 and same_wave.sum() > 100 and (both & ~same_thread & ~same_wave).sum() > 100
    sample = PC.lane_case(PC.LANE_SAMPLE)
    assert {w % 4 for w in PC.LANE_SAMPLE} == {0, 1, 2, 3} and {w // 256 for w in PC.LANE_SAMPLE} == {0, 1, 2, 3}
    assert set(sample["step"].tolist()) >= set(PC.TIE_STEPS)


def test_long_rows_and_the_top_rows():
    case = PC.long_row_case(TILES)
    length = int(case["lengths"][2])
    assert length == TILES * P.TILE + 37 and case["near"] < length // 10 and case["far"] > length - length // 10
    many = PC.many_rows_case(TILES)
    assert many["lengths"].sum() == length and many["seqs"][0] is case["seqs"][0]
    small = PC.small_top_case()
    size = small["seqs"][0].size
    s, n = small["starts"], small["lengths"]
    assert size == PC.SMALL_TOP and size % 16 == (2 ** 31 - 1) % 16 and size % P.TILE == (2 ** 31 - 1) % P.TILE
    for w in (20, 256):
        for length in (w - 1, w, w + 1):
            assert ((s + n == size) & (n == length)).any()
    assert ((s + n > size) & (s < size)).any() and (s == size - 1).any() and (s == size).any()
    for do_mask in (True, False):
        got = PC.MODEL.scores(*batch(small), do_mask=do_mask)
        assert (~np.isnan(got)).any(axis=1).all()
    offsets = np.concatenate([[0], np.cumsum(n)])
    i = int(np.flatnonzero((s + n == size) & (n == 256))[0])
    got = PC.MODEL.scores(*batch(small), do_mask=False)
    assert not np.isnan(got[1, offsets[i]]) and np.isnan(got[1, offsets[i] + 1:offsets[i + 1]]).all()  # the one window that ends at the size


STAND_INS = {
    "descending": ("cols16_all", "lds_256x16", "mats_max"),
    "last_wins": ("lanes", "long"),
    "nan_greatest": ("extremes",),
    "short_halo": ("lds_4x256x4", "cols16_all", "small_top", "many"),
    "four_bits": ("cols16_all", "cols16_g_top", "lds_plus_16"),
}


@pytest.mark.parametrize("change", sorted(STAND_INS))
def test_a_changed_model_fails_its_cases(change):
    """the model passes every case as a device; with one change it fails the cases named for that change"""
    cases = small_cases()
    stand_in = PC.Model(**{change: True})
    for name in STAND_INS[change]:
        PC.check_batch([PC.MODEL], cases[name], where=name)
        with pytest.raises(AssertionError):
            PC.check_batch([stand_in], cases[name], where=name)
