"""
Position weight matrices scored over 2bit rows on the device (bxmi_pwm_*, bxmi_twobit_pwm_*, bxmi.motif, TwoBitSet.scores / score_matrix
/ best, bxmi.cli.twobit_pwm_scores) against the answers recorded from the reference's ScoringMatrix.score_string (tests/golden/pwm)
and, beyond them, against tests/pwm_model.py -- itself pinned to those recordings by tests/test_pwm_model_golden.py.  Every
comparison is of the 32 bits of a float: no tolerance anywhere -- but where the model's own sum is an arithmetic NaN (inf - inf, a NaN
entry), whose sign and payload include/bxmi.h leaves open: there the device's element must be a NaN (tests/pwm_cases.py, whose seeded
cases tests/test_pwm_cases.py checks without a device).
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import pwm_cases as PC
import pwm_model as P
import twobit_cases as K
import twobit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_pwm_scores_dev", "bxmi_twobit_pwm_best_dev")
SENTINEL = np.array([0xEEEEEEEE], dtype=np.uint32).view(np.float32)[0]
SENTINEL_BITS = 0xEEEEEEEE


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(P.bits(got), P.bits(want))


def device_set(mats):
    """model matrices as a motif.MatrixSet"""
    from bxmi import motif

    return motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mats])


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def scores_host(tracks, ms, track_of, starts, width=0, lengths=None, do_mask=True):
    """bxmi_twobit_pwm_scores with the rows as they are (no clipping), `out` filled with the sentinel first -> float32 [n_mats, total]"""
    from bxmi import _ffi as ffi

    t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
    offsets = None if lengths is None else offsets_of(lengths)
    total = len(t) * width if offsets is None else int(offsets[-1])
    out = np.full((ms.n_mats, total), SENTINEL, dtype=np.float32)
    ffi.call("bxmi_twobit_pwm_scores", ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), width, ffi.ptr(offsets), total, int(do_mask), ms._h,
             ffi.ptr(out))
    return out


def scores_dev(tracks, ms, track_of, starts, width=0, lengths=None, do_mask=True, lead=16, tail=9):
    """bxmi_twobit_pwm_scores_dev on arrays in device memory, on the null stream, `out` `lead` floats into an allocation of sentinel
    floats, which must still be there on both sides afterwards -> float32 [n_mats, total]"""
    from bxmi import _ffi as ffi

    offsets = None if lengths is None else offsets_of(lengths)
    total = len(track_of) * width if offsets is None else int(offsets[-1])
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts)]
    rows += [ffi.DeviceArray.from_numpy(offsets)] if offsets is not None else []
    cells = ms.n_mats * total
    out = ffi.DeviceArray.from_numpy(np.full(lead + cells + tail, SENTINEL, dtype=np.float32))
    assert out.ptr % 16 == 0
    ffi.call("bxmi_twobit_pwm_scores_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, len(track_of), width,
             rows[2].ptr if offsets is not None else None, total, int(do_mask), ms._h, out.ptr + 4 * lead, None)
    ffi.call("bxmi_synchronize", None)
    words = out.to_numpy(np.uint32)
    for a in rows + [out]:
        a.free()
    assert (words[:lead] == SENTINEL_BITS).all() and (words[lead + cells:] == SENTINEL_BITS).all(), "written outside the planes"
    return words[lead:lead + cells].view(np.float32).reshape(ms.n_mats, total)


def best_host(tracks, ms, track_of, starts, width=0, lengths=None, do_mask=True):
    from bxmi import _ffi as ffi

    t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
    offsets = None if lengths is None else offsets_of(lengths)
    total = len(t) * width if offsets is None else int(offsets[-1])
    score = np.full((ms.n_mats, len(t)), SENTINEL, dtype=np.float32)
    pos = np.full((ms.n_mats, len(t)), -7, dtype=np.int32)
    ffi.call("bxmi_twobit_pwm_best", ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), width, ffi.ptr(offsets), total, int(do_mask), ms._h,
             ffi.ptr(score), ffi.ptr(pos))
    return score, pos


def best_dev(tracks, ms, track_of, starts, width=0, lengths=None, do_mask=True, lead=3, tail=5, slack=0):
    """bxmi_twobit_pwm_best_dev, sentinels before and after both outputs; `slack`: how far beyond row_off[n] the `total` given lies"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    offsets = None if lengths is None else offsets_of(lengths)
    total = n * width if offsets is None else int(offsets[-1]) + slack
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts)]
    rows += [ffi.DeviceArray.from_numpy(offsets)] if offsets is not None else []
    cells = ms.n_mats * n
    score = ffi.DeviceArray.from_numpy(np.full(lead + cells + tail, SENTINEL, dtype=np.float32))
    pos = ffi.DeviceArray.from_numpy(np.full(lead + cells + tail, -7, dtype=np.int32))
    ffi.call("bxmi_twobit_pwm_best_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, n, width, rows[2].ptr if offsets is not None else None,
             total, int(do_mask), ms._h, score.ptr + 4 * lead, pos.ptr + 4 * lead, None)
    ffi.call("bxmi_synchronize", None)
    s, p = score.to_numpy(np.uint32), pos.to_numpy(np.int32)
    for a in rows + [score, pos]:
        a.free()
    assert (s[:lead] == SENTINEL_BITS).all() and (s[lead + cells:] == SENTINEL_BITS).all(), "written outside the scores"
    assert (p[:lead] == -7).all() and (p[lead + cells:] == -7).all(), "written outside the positions"
    return s[lead:lead + cells].view(np.float32).reshape(ms.n_mats, n), p[lead:lead + cells].reshape(ms.n_mats, n)


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", M.FILES)
def test_recorded_scores(name):
    """the recorded regions of a file as one ragged batch per do_mask setting and alphabet, through the Python layer (which clips as
    `get`), the host form, the _dev form and both forms of the best hit: the reference's own float32 answers"""
    from bxmi import motif, sequence

    checked = 0
    for do_mask in (True, False):
        genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
        tracks = list(genome.tracks.values())
        for names, seqs, track_of, starts, ends, want in P.recorded_batches(name, do_mask):
            ms = device_set([P.matrix(k) for k in names])
            assert (ms.n_mats, ms.max_width) == (len(names), max(P.matrix(k).width for k in names)) and len(ms) == len(names)
            got, offsets = genome.scores(track_of, starts, ends, ms)
            assert got.dtype == np.float32 and offsets.dtype == np.int64 and np.diff(offsets).tolist() == [e - s for s, e in zip(starts, ends)]
            lengths = np.diff(offsets)
            assert same_bits(scores_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask), got)
            top, at = genome.best(track_of, starts, ends, ms)
            top_dev, at_dev = best_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask)
            assert same_bits(top_dev, top) and np.array_equal(at_dev, at)
            for m, k in enumerate(names):
                for row, answer in want[k]:
                    assert same_bits(got[m, offsets[row]:offsets[row + 1]], answer), (name, do_mask, k, row)
                    score, pos = P.best_of(answer)
                    assert same_bits(top[m, row], np.float32(score)) and at[m, row] == pos, (name, do_mask, k, row)
                    checked += 1
            # matrices given as such are put on the device for the call
            again, _ = motif.scores(tracks, track_of, starts, ends, ms.matrices, do_mask)
            assert same_bits(again, got)
            ms.close()
        genome.close()
    assert checked == len(P.manifest()["files"][name]["entries"])


# ------------------------------------------------------------ structural cases against the model --
@pytest.fixture(scope="module")
def structural():
    """the four structural sequences on the device and the model of them"""
    from bxmi import sequence

    seqs = M.structural_sequences()
    tracks = [sequence.TwoBitTrack(s) for s in seqs]
    yield tracks, P.Scores(seqs)
    for t in tracks:
        t.close()


@pytest.mark.parametrize("n_mats,extra", [(m, x) for m in (1, 2, 3) for x in (0, 1, 2, 3)])
def test_ragged_structural_cases(structural, n_mats, extra):
    """twobit_model.ragged_case() -- rows of one base, empty rows between rows, a row inside an N block, more one-base blocks in a
    segment than TB_CHUNK stages, positions outside the sequence on both sides, a row naming no track, the size-0 sequence -- plus
    pwm_model.ragged_case()'s rows: a window from one tile into the next, a row ending on a tile boundary, rows of W - 1, W and
    W + 1, windows across block edges.  Widths 1 and WIDTH_MAX in one handle; n_mats of 1, 2, 3 with total % 4 of 1, 2, 3 (the
    planes after the first are misaligned) and 0; `out` aligned and 4 bytes past a 16-byte boundary; sentinels around the planes"""
    tracks, model = structural
    mats = P.structural_mats()[:n_mats] if n_mats > 1 else [P.matrix("w20")]
    track_of, starts, lengths = P.ragged_case()
    assert sum(lengths) % 4 == 0
    track_of, starts, lengths = track_of + [0] * extra, starts + [50] * extra, lengths + [1] * extra
    ms = device_set(mats)
    for do_mask in (True, False):
        want = model.scores(track_of, starts, lengths, mats, do_mask)
        assert want.shape[1] % 4 == extra and (~np.isnan(want)).any(axis=1).all() and np.isnan(want).any()
        assert same_bits(scores_host(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask), want), (do_mask, "host form")
        for lead in (16, 1):
            got = scores_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask, lead=lead)
            assert same_bits(got, want), (do_mask, lead, np.flatnonzero((P.bits(got) != P.bits(want)).any(axis=0))[:10])
    ms.close()


@pytest.mark.parametrize("width", (1, 37, P.TILE + 1))
def test_score_matrix_widths(structural, width):
    """windows of one width over block edges, both ends of every sequence, no track: the alphabets with N and with lower case, the
    -inf, denormal and zero matrices, and a set of more values than stay in LDS (staged matrix by matrix)"""
    from bxmi import motif

    tracks, model = structural
    track_of, starts = M.matrix_case(width)
    wmax = P.matrix("wmax")
    for mats in ([P.matrix("w20n"), P.matrix("w4n")], [P.matrix("w20lc"), P.matrix("w1lc")], [P.matrix(k) for k in ("ninf", "denorm", "zeros")],
                 [wmax, wmax.reverse_complement(), wmax, P.matrix("w1"), wmax.reverse_complement(), wmax]):
        ms = device_set(mats)
        want = model.scores(track_of, starts, [width] * len(starts), mats, True).reshape(len(mats), len(starts), width)
        got = motif.score_matrix(tracks, track_of, starts, width, ms)
        assert same_bits(got, want), (width, len(mats))
        assert same_bits(scores_dev(tracks, ms, track_of, starts, width=width, lead=1).reshape(want.shape), want), (width, len(mats), "device form")
        ms.close()
    mats = [P.matrix("ninf"), P.matrix("denorm")]
    want = model.scores(track_of, starts, [width] * len(starts), mats, False)
    if width == 37:
        assert np.isneginf(want[0]).any() and ((np.abs(want[1]) < 1.2e-38) & (want[1] != 0)).any()  # -inf scores, denormal scores
    ms = device_set(mats)
    assert same_bits(scores_host(tracks, ms, track_of, starts, width=width, do_mask=False), want)
    ms.close()


def test_reverse_complement_and_alphabets():
    """ScoringMatrix lays out its columns as the reference's from_rows, whatever the order of the alphabet given; the reverse
    complement is the reversed rows and columns"""
    from bxmi import motif

    rng = np.random.default_rng(7)
    rows = rng.normal(size=(5, 4)).astype(np.float32)
    a, b = motif.ScoringMatrix("TGCA", rows), P.Matrix("TGCA", rows)
    assert a.sorted_alphabet == list("ACGT") and np.array_equal(a.values, b.values) and np.array_equal(a.char_to_index, b.char_to_index)
    assert a.char_to_index.dtype == np.int16 and a.values.dtype == np.float32 and a.width == 5
    rc = a.reverse_complement()
    assert np.array_equal(rc.values, a.values[::-1, ::-1]) and np.array_equal(rc.values, b.reverse_complement().values)
    with pytest.raises(ValueError):
        motif.MatrixSet([a, motif.ScoringMatrix("ACGTN", np.zeros((2, 5)))])


def test_best_structural_cases(structural):
    """against the model's NaN-aware maximum and first position: the zeros matrix (every score ties: the first scoreable offset), rows
    with no scoreable window (NaN and -1), a row over three tiles with its maximum in the last tile and an equal score in the
    first, sentinels around both outputs, host and _dev forms, a `total` that is only a bound"""
    from bxmi import sequence

    tracks, model = structural
    track_of, starts, lengths = P.ragged_case()
    mats = [P.matrix("zeros"), P.matrix("w4"), P.matrix("ninf")]
    ms = device_set(mats)
    for do_mask in (True, False):
        score, pos = model.best(track_of, starts, lengths, mats, do_mask)
        assert (pos[0] == -1).any() and (pos[0] > 0).any() and np.isnan(score[0][pos[0] == -1]).all() and (score[0][pos[0] >= 0] == 0).all()
        got = best_host(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask)
        assert same_bits(got[0], score) and np.array_equal(got[1], pos), (do_mask, "host form")
        for slack in (0, 40 * P.TILE + 3):
            got = best_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask, slack=slack)
            assert same_bits(got[0], score) and np.array_equal(got[1], pos), (do_mask, slack)
    t, s = M.matrix_case(37)
    score, pos = model.best(t, s, [37] * len(s), mats, True)
    for got in (best_host(tracks, ms, t, s, width=37), best_dev(tracks, ms, t, s, width=37)):
        assert same_bits(got[0], score) and np.array_equal(got[1], pos)
    ms.close()
    seq, row_t, row_s, row_n, mat = P.tie_case()
    score, pos = P.Scores([seq]).best(row_t, row_s, row_n, [mat], True)
    assert pos[0].tolist() == [-1, 95, -1] and score[0, 1] == 4.0
    track, ms = sequence.TwoBitTrack(seq), device_set([mat])
    for got in (best_host([track], ms, row_t, row_s, lengths=row_n), best_dev([track], ms, row_t, row_s, lengths=row_n)):
        assert same_bits(got[0], score) and np.array_equal(got[1], pos)
    whole = scores_host([track], ms, row_t, row_s, lengths=row_n)[0, 10:10 + 3 * P.TILE]
    assert np.flatnonzero(whole == 4.0).tolist() == [95, 2 * P.TILE + 495]  # the equal score two tiles on
    ms.close()
    track.close()


def test_nothing_to_do_and_bad_arguments(structural):
    from bxmi import _ffi as ffi
    from bxmi import motif

    tracks, _ = structural
    ms = device_set([P.matrix("w4")])
    got, offsets = motif.scores(tracks, [], [], [], ms)
    assert got.shape == (1, 0) and offsets.tolist() == [0]
    assert motif.score_matrix(tracks, [], [], 5, ms).shape == (1, 0, 5)
    score, pos = motif.best(tracks, [0, 2, -1], [5, 0, 9], [5, 0, 30], ms)
    assert (P.bits(score) == P.NAN_BITS).all() and (pos == -1).all() and score.shape == (1, 3)
    for call in (lambda: motif.score_matrix(tracks, [0], [0], 0, ms), lambda: motif.score_matrix(tracks, [len(tracks)], [0], 4, ms),
                 lambda: motif.scores(tracks, [0, len(tracks)], [0, 0], [4, 4], ms), lambda: motif.best(tracks, [len(tracks) + 7], [0], [4], ms)):
        with pytest.raises(ffi.BxmiError) as e:
            call()
        assert e.value.code == ffi.EINVAL
    ms.close()
    # total * n_mats beyond what the output index holds: refused by the forms that write planes, before the rows are looked at
    # (no rows: nothing could be launched); the best hits have no planes and take the same total as the bound it may be
    ms = device_set([P.matrix("w4"), P.matrix("w1")])
    lib = ffi.load()
    huge = 2 ** 62
    offsets = np.array([0, huge], dtype=np.int64)
    d_off = ffi.DeviceArray.from_numpy(offsets[:1])
    out = np.zeros(4, dtype=np.float32)
    pos = np.zeros(4, dtype=np.int32)
    word = b"total = %d elements in each of 2 planes is more than the output index holds" % huge
    rc = lib.bxmi_twobit_pwm_scores_dev(ffi.handles(tracks), len(tracks), None, None, 0, 0, d_off.ptr, huge, 1, ms._h, None, None)
    assert rc == ffi.EINVAL and b"bxmi_twobit_pwm_scores_dev: " + word in lib.bxmi_last_error(), lib.bxmi_last_error()
    rc = lib.bxmi_twobit_pwm_scores(ffi.handles(tracks), len(tracks), None, None, 0, 0, ffi.ptr(offsets), huge, 1, ms._h, ffi.ptr(out))
    assert rc == ffi.EINVAL and b"bxmi_twobit_pwm_scores: " + word in lib.bxmi_last_error(), lib.bxmi_last_error()
    assert lib.bxmi_twobit_pwm_scores_dev(ffi.handles(tracks), len(tracks), None, None, 0, 0, d_off.ptr, huge // 16, 1, ms._h, None, None) == ffi.OK
    assert lib.bxmi_twobit_pwm_best_dev(ffi.handles(tracks), len(tracks), None, None, 0, 0, d_off.ptr, huge, 1, ms._h, None, None, None) == ffi.OK
    # (the host form of the best hits reads its offsets and asks that they end at `total`, so no rows means a total of 0; what it
    # says of this one is about the offsets, not about planes)
    rc = lib.bxmi_twobit_pwm_best(ffi.handles(tracks), len(tracks), None, None, 0, 0, ffi.ptr(offsets), huge, 1, ms._h, ffi.ptr(out), ffi.ptr(pos))
    assert rc == ffi.EINVAL and b"row_off[n] = 0, but total" in lib.bxmi_last_error() and b"planes" not in lib.bxmi_last_error()
    d_off.free()
    ms.close()


# ------------------------------------------------------------ a seeded case of about 1 Mb --
def test_random_sequences_at_scale():
    """two random sequences of twobit_cases.random_sequence with every block edge, about 1 Mb of ragged rows and of windows, two
    matrices (one and its reverse complement): scores, score_matrix and best, host and _dev forms"""
    from bxmi import motif, sequence

    rng = np.random.default_rng(360)
    seqs = [K.random_sequence(rng, 300_000, 700, 2000), K.random_sequence(rng, 70_001, 150, 400)]
    w20 = P.matrix("w20")
    mats = [w20, w20.reverse_complement()]
    n = 400
    track_of = rng.integers(0, 2, n)
    track_of[rng.integers(0, n, 5)] = -1
    size_of = np.array([s.size for s in seqs] + [0])[track_of]
    lengths = K.log_uniform(rng, 1, 30_000, n) - 1
    lengths[:3] = (0, 19, 3 * P.TILE)
    starts = rng.integers(-50, np.maximum(size_of - lengths // 2, 0) + 51)
    assert 700_000 < lengths.sum() < 1_600_000
    model = P.Scores(seqs)
    tracks = [sequence.TwoBitTrack(s) for s in seqs]
    ms = device_set(mats)
    for do_mask in (True, False):
        want = model.scores(track_of, starts, lengths, mats, do_mask)
        assert 0.2 < np.isnan(want).mean() < 0.95
        assert same_bits(scores_host(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask), want), do_mask
        assert same_bits(scores_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask, lead=1), want), do_mask
        score, pos = model.best(track_of, starts, lengths, mats, do_mask)
        for got in (best_host(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask),
                    best_dev(tracks, ms, track_of, starts, lengths=lengths, do_mask=do_mask, slack=12345)):
            assert same_bits(got[0], score) and np.array_equal(got[1], pos), do_mask
    width = 1000
    want = model.scores(track_of, starts, [width] * n, mats, True).reshape(2, n, width)
    assert same_bits(motif.score_matrix(tracks, track_of, starts, width, ms), want)
    # the Python layer clips as `get`
    ends = starts + lengths
    s_c, n_c = P.clipped(seqs, track_of, starts, ends)
    got, offsets = motif.scores(tracks, track_of, starts, ends, ms, True)
    assert np.diff(offsets).tolist() == n_c and same_bits(got, model.scores(track_of, s_c, n_c, mats, True))
    score, pos = model.best(track_of, s_c, n_c, mats, True)
    got = motif.best(tracks, track_of, starts, ends, ms, True)
    assert same_bits(got[0], score) and np.array_equal(got[1], pos)
    ms.close()
    for t in tracks:
        t.close()


def test_host_form_across_a_slab_boundary():
    """bxmi_twobit_pwm_scores in slabs of PW_SLAB elements over all planes (pwm_model.slab_elements per plane): with two matrices,
    four rows of slab // 2 + 1001 elements, so the first slab ends inside the second row and the second inside the fourth; the
    windows across a cut read letters of both slabs.  With PW_MATS_MAX matrices the slab is 128 tiles and the same rows cross it
    many times: every plane's part of every slab lands where it belongs"""
    from bxmi import sequence

    rng = np.random.default_rng(361)
    slab = P.slab_elements(2)
    half = slab // 2 + 1001
    seq = K.random_sequence(rng, half + 5000, 300, 900)
    w20 = P.matrix("w20")
    mats = [w20, w20.reverse_complement()]
    track_of, starts, lengths = [0, 0, 0, 0, 0], [7, 1000, 2500, 3000, 40], [half, half, half, half, 77]
    assert slab == P.PW_SLAB // 2 and sum(lengths[:1]) < slab < sum(lengths[:2]) and sum(lengths[:3]) < 2 * slab < sum(lengths[:4]) and slab % P.TILE == 0
    model = P.Scores([seq])
    want = model.scores(track_of, starts, lengths, mats, True)
    track, ms = sequence.TwoBitTrack(seq), device_set(mats)
    got = scores_host([track], ms, track_of, starts, lengths=lengths)
    assert same_bits(got, want), np.flatnonzero((P.bits(got) != P.bits(want)).any(axis=0))[:10]
    assert not np.isnan(want[:, slab - 40:slab + 40]).all() and not np.isnan(want[:, 2 * slab - 40:2 * slab + 40]).all()
    ms.close()
    many = [w20, w20.reverse_complement(), P.matrix("w4"), P.matrix("w1")] * (P.MATS_MAX // 4)
    small = P.slab_elements(len(many))
    track_of, starts, lengths = [0, 0, 0, 0], [7, 1000, 2500, 40], [small // 2 + 101, small + 7, 3 * small - 50, 9]
    assert len(many) == P.MATS_MAX and small == 128 * P.TILE and sum(lengths) > 4 * small
    want = model.scores(track_of, starts, lengths, many[:4], True)
    ms = device_set(many)
    got = scores_host([track], ms, track_of, starts, lengths=lengths)
    for k in range(len(many)):
        assert same_bits(got[k], want[k % 4]), k
    ms.close()
    track.close()


# ------------------------------------------------------------ the seeded cases of tests/pwm_cases.py --
class Held:
    """the tracks and matrix sets that the cases of a test put on the device, each once, all closed again whatever the test does"""

    def __init__(self):
        self.tracks, self.sets = {}, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in list(self.sets.values()) + list(self.tracks.values()):
            h[1].close()

    def tracks_of(self, seqs):
        from bxmi import sequence

        for s in seqs:
            if id(s) not in self.tracks:
                self.tracks[id(s)] = (s, sequence.TwoBitTrack(s))
        return [self.tracks[id(s)][1] for s in seqs]

    def set_of(self, mats):
        if id(mats) not in self.sets:
            self.sets[id(mats)] = (mats, device_set(mats))
        return self.sets[id(mats)][1]


class OnDevice:
    """one form of the library, host arrays or the _dev entry points, as a device of pwm_cases.check_batch; `slack` goes to the
    _dev form of the best hits alone: the host form asks that `total` is where the offsets end"""

    def __init__(self, held, dev):
        self.held, self.dev = held, dev

    def scores(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True):
        form = scores_dev if self.dev else scores_host
        return form(self.held.tracks_of(seqs), self.held.set_of(mats), track_of, starts, width=width, lengths=lengths, do_mask=do_mask)

    def best(self, seqs, mats, track_of, starts, lengths=None, width=0, do_mask=True, slack=0):
        tracks, ms = self.held.tracks_of(seqs), self.held.set_of(mats)
        if self.dev:
            return best_dev(tracks, ms, track_of, starts, width=width, lengths=lengths, do_mask=do_mask, slack=slack)
        return best_host(tracks, ms, track_of, starts, width=width, lengths=lengths, do_mask=do_mask)


def both_forms(held):
    return [OnDevice(held, False), OnDevice(held, True)]


@pytest.mark.parametrize("name", sorted(PC.MATRIX_SETS))
def test_seeded_matrix_sets(name):
    """random matrices of mixed magnitudes, so that a sum in another order has other bits (asserted by the generator): exactly
    PW_LDS_VALUES values as four matrices of 256 x 4 and as the largest single matrix, 256 x 16; PW_LDS_VALUES + n_cols values, the
    smallest set staged matrix by matrix; PW_MATS_MAX matrices of 1 .. 256 rows, the halo from one of them; 16 columns with column
    15 selected by t, by g, by n, by T, alphabets without N and n, without lower case, and with T and A in lower case only.  100 ragged rows of two sequences and
    the same as windows of one width: scores, score_matrix and best, host and _dev forms, with and without the mask"""
    with Held() as held:
        PC.check_batch(both_forms(held), PC.matrix_set_case(name), where=name)


def test_extremes_and_arithmetic_nans():
    """pwm_cases.extremes_case: best scores that are negative, denormal, +inf (at its first offset) and -inf; windows that sum to
    inf - inf or meet a NaN entry are a NaN in the planes, of whatever sign and payload, and never a candidate for the best hit,
    also where the greatest score lies next to one; every other element bit for bit, the unscoreable ones 0x7FC00000"""
    with Held() as held:
        PC.check_batch(both_forms(held), PC.extremes_case(), where="extremes")


def test_best_hit_on_every_lane():
    """pwm_cases.lane_case: 1024 rows of one tile, about 1 M elements, the greatest score of row i at offset i -- the winning key
    comes from every lane of every wave and from each of a thread's four elements; under the second matrix offsets i and i + k tie,
    k of 1 .. 256: within a thread, across the lanes of a wave, across waves, and the first offset wins"""
    case = PC.lane_case()
    with Held() as held:
        devs = both_forms(held)
        PC.check_batch(devs, case, do_masks=(True,), planes=False, where="lanes")
        for dev in devs:
            score, pos = dev.best(case["seqs"], case["mats"], case["track_of"], case["starts"], case["lengths"])
            assert np.array_equal(pos[0], np.arange(P.TILE)) and np.array_equal(pos[1], np.arange(P.TILE)) and (score == 1).all()


def test_best_walks_more_tiles_than_the_grid():
    """the grid of the best hits is at most compute units x 8 workgroups, each walking every gridDim.x-th tile: with half as many
    tiles again some workgroups take two tiles and some one.  One row of all of them -- every workgroup sends keys to the same
    cell: under the zeros matrix they all tie and the first scoreable offset wins; under the other the greatest score lies in the
    far end of the row and its equal in the near end -- then a `total` several grid fills beyond the rows, then the same total in
    a few thousand rows, so that the tiles of the second trip begin inside rows and hold several segments"""
    import ctypes as C

    from bxmi import _ffi

    dev, cus = C.c_int(0), C.c_int(0)
    _ffi.call("bxmi_get_device", C.byref(dev))
    _ffi.call("bxmi_device_info", dev.value, None, 0, C.byref(cus), None)
    fill = cus.value * 8
    tiles = fill + fill // 2
    assert cus.value > 0 and tiles > fill  # (or nothing here would take the second trip)
    with Held() as held:
        devs = both_forms(held)
        PC.check_batch(devs, PC.long_row_case(tiles), planes=False, where="one long row", best_args=({}, dict(slack=5 * fill * P.TILE + 3)))
        PC.check_batch(devs, PC.many_rows_case(tiles), planes=False, where="many rows")


def test_scores_at_the_top_of_int32():
    """pwm_cases.top_case on twobit_cases.TopSequence, 2^31 - 1 bases (512 MiB of device memory: given back whatever happens):
    rows that end at the size, cross it, of W - 1, W and W + 1 bases ending at it, from its last base and from the size itself,
    across the edges of an N block of 2^28 bases and of a mask block of nearly everything; matrices of 20 and 256 rows, whose
    halo reaches past the size.  Positions, the packed word and the blocks' edges next to the top of int32"""
    with Held() as held:
        PC.check_batch(both_forms(held), PC.top_case(), where="top")


# ------------------------------------------------------------ device entry points on torch tensors --
def test_dev_forms_on_torch_tensors():
    """scores_dev / score_matrix_dev / best_dev on torch tensors, on torch's current stream and on a stream of the caller's (best_dev
    also while the current stream is busy, so that its clipping is late), through
    TwoBitSet as well, in a process of its own: torch brings its own HIP runtime, which the rest of the suite keeps out of the
    test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import twobit_model as M
import pwm_model as P
from bxmi import motif, sequence

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

def same(got, want):
    got = got.cpu().numpy()
    return got.shape == want.shape and np.array_equal(P.bits(got), P.bits(want))

seqs = M.structural_sequences()
model = P.Scores(seqs)
dev = [sequence.TwoBitTrack(s) for s in seqs]
mats = P.structural_mats()
ms = motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mats])
side = torch.cuda.Stream()
busy = torch.zeros(1 << 27, dtype=torch.float32, device="cuda")

track_of, starts, lengths = P.ragged_case()
ends = [s + n for s, n in zip(starts, lengths)]
s_c, n_c = P.clipped(seqs, track_of, starts, ends)
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
for do_mask in (True, False):
    want = model.scores(track_of, s_c, n_c, mats, do_mask)
    top, at = model.best(track_of, s_c, n_c, mats, do_mask)
    got, offsets = motif.scores_dev(dev, *d, ms, do_mask=do_mask)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.float32 and offsets.dtype == torch.int64 and np.diff(offsets.cpu().numpy()).tolist() == n_c
    assert same(got, want), do_mask
    got, offsets = motif.scores_dev(dev, *d, ms, do_mask=do_mask, stream=side.cuda_stream)
    churn = [torch.zeros(len(track_of), dtype=torch.int32, device="cuda") for _ in range(4)]  # (what could take a freed block)
    side.synchronize()
    assert same(got, want), (do_mask, "side stream")
    with torch.cuda.stream(side):
        score, pos = motif.best_dev(dev, *d, ms, do_mask=do_mask)
    side.synchronize()
    assert score.dtype == torch.float32 and pos.dtype == torch.int32 and same(score, top) and np.array_equal(pos.cpu().numpy(), at), do_mask
    # torch's current stream is busy when the clipping is queued behind it: the side stream must wait for the clipping, on the
    # device, before its kernels read the offsets
    for _ in range(20):
        busy.add_(1)
    score, pos = motif.best_dev(dev, *d, ms, do_mask=do_mask, stream=side.cuda_stream)
    churn = [torch.zeros(len(track_of) + 1, dtype=torch.int64, device="cuda") for _ in range(4)]
    side.synchronize()
    assert same(score, top) and np.array_equal(pos.cpu().numpy(), at), (do_mask, "side stream")

for width in (37, P.TILE + 1):
    track_of_m, starts_m = M.matrix_case(width)
    want = model.scores(track_of_m, starts_m, [width] * len(starts_m), mats, True).reshape(len(mats), len(starts_m), width)
    rows = [dev_i32(track_of_m, 1), dev_i32(starts_m, 2)]
    got = motif.score_matrix_dev(dev, *rows, width, ms, stream=side.cuda_stream)
    side.synchronize()
    assert same(got, want), width
    out = torch.full(want.shape, 5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        res = motif.score_matrix_dev(dev, *rows, width, ms, out=out)
    side.synchronize()
    assert res is out and same(out, want), width

# through TwoBitSet; entries the device forms cannot refuse are rows of NaN
genome = sequence.TwoBitSet({"blocks": seqs[0], "odd": seqs[1]}, do_mask=True)
t2, s2, e2 = dev_i32(np.array([0, 1, 5, -1]), 0), dev_i32(np.array([100, 0, 3, 3]), 0), dev_i32(np.array([400, 41, 30, 30]), 0)
want = P.Scores(seqs[:2]).scores([0, 1, -1, -1], [100, 0, 0, 0], [300, 41, 0, 0], mats, True)
got, offsets = genome.scores_dev(t2, s2, e2, ms)
assert offsets.cpu().numpy().tolist() == [0, 300, 341, 341, 341] and same(got, want)
score, pos = genome.best_dev(t2, s2, e2, ms)
top, at = P.Scores(seqs[:2]).best([0, 1, -1, -1], [100, 0, 0, 0], [300, 41, 0, 0], mats, True)
torch.cuda.synchronize()
assert same(score, top) and np.array_equal(pos.cpu().numpy(), at)
got = genome.score_matrix_dev(t2, s2, 6, ms)
torch.cuda.synchronize()
assert same(got, P.Scores(seqs[:2]).scores([0, 1, -1, -1], [100, 0, 3, 3], [6] * 4, mats, True).reshape(len(mats), 4, 6))
got, offsets = motif.scores_dev(dev, d[0][:0], d[1][:0], d[2][:0], ms, stream=side.cuda_stream)
assert tuple(got.shape) == (len(mats), 0) and offsets.tolist() == [0]
assert tuple(motif.best_dev(dev, d[0][:0], d[1][:0], d[2][:0], ms)[1].shape) == (len(mats), 0)
try:
    motif.best_dev(dev, *d, mats)
    raise SystemExit("matrices that are not on the device were accepted")
except ValueError:
    pass
genome.close()
ms.close()
for t in dev:
    t.close()
print("pwm dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pwm dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ------------------------------------------------------------ the command line --
def test_command_line_prints_the_models_lines(tmp_path):
    from bxmi.cli import twobit_pwm_scores as cli

    name = "multi.2bit"
    seqs = M.read(name)
    names = list(seqs)
    mat = P.matrix("w4")
    path = tmp_path / "matrix.txt"
    path.write_text("".join(mat.alphabet) + "\n" + "".join(" ".join(repr(float(x)) for x in row) + "\n" for row in mat.rows))
    rows = [("ckpt", 990, 1030), ("odd", 0, 41), ("ckpt", 2565, 2600), ("empty", 0, 5), ("chrNone", 7, 9), ("odd", 38, 41)]
    bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r for r in rows)
    track_of = [names.index(c) if c in names else -1 for c, _, _ in rows]
    model = P.Scores([seqs[k] for k in names])
    for flags, do_mask, mats in (([], True, [mat]), (["-u", "-r"], False, [mat, mat.reverse_complement()])):
        s_c, n_c = P.clipped([seqs[k] for k in names], track_of, [r[1] for r in rows], [r[2] for r in rows])
        want = model.scores(track_of, s_c, n_c, mats, do_mask)
        offsets = offsets_of(n_c)
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), str(path)] + flags, stdin=io.StringIO(bed), out=out)
        text = "".join("> %s %d %d\n" % r + "".join(" ".join(repr(float(x)) for x in want[m, offsets[i]:offsets[i + 1]]) + "\n" for m in range(len(mats)))
                       for i, r in enumerate(rows))
        assert out.getvalue() == text and "nan" in text and any(ch.isdigit() for ch in text.split("\n")[1]), flags
        score, pos = model.best(track_of, s_c, n_c, mats, do_mask)
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), "-b", str(path)] + flags, stdin=io.StringIO(bed), out=out)
        text = "".join("\t".join([r[0], str(r[1]), str(r[2])] + ["%s\t%d" % (repr(float(score[m, i])), pos[m, i]) for m in range(len(mats))]) + "\n"
                       for i, r in enumerate(rows))
        assert out.getvalue() == text, flags
