"""
The thresholded hits of position weight matrices on the device (bxmi_twobit_pwm_hits, bxmi_twobit_pwm_hits_dev, bxmi.motif.hits /
hits_dev, TwoBitSet.hits / hits_dev, bxmi.cli.twobit_pwm_hits) against the existing models: the nonzero of (plane >= threshold and
not NaN) of tests/pwm_model.py -- pinned to the reference's recorded answers -- and of tests/pwm_cases.py, in ascending (matrix,
row, offset).  Rows and positions are compared exactly, scores by their 32 bits; the hit arrays lie inside sentinel-filled
allocations that must be intact on both sides.  tests/test_pwm_hits_kernel_host.py runs the same kernels on the host.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import pwm_cases as PC
import pwm_hits_cases as H
import pwm_model as P
import twobit_cases as K
import twobit_model as M
from pwm_hits_cases import INF, offsets_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_pwm_hits_dev",)
SENTINEL_BITS = 0xEEEEEEEE


def device_set(mats):
    from bxmi import motif

    return motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mats])


def _rows(track_of, starts, width, lengths):
    t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
    offsets = None if lengths is None else offsets_of(lengths)
    return t, s, offsets, len(t) * width if offsets is None else int(offsets[-1])


def hits_host(tracks, ms, track_of, starts, thresholds, width=0, lengths=None, do_mask=True, cap=None, lead=3, tail=5):
    """bxmi_twobit_pwm_hits with the rows as they are; the hit arrays `lead` entries into sentinel-filled ones -> (rc, (mat_hits,
    rows, pos, score)): with cap None a counts-only call comes first and the arrays hold exactly the hits"""
    from bxmi import _ffi as ffi

    t, s, offsets, total = _rows(track_of, starts, width, lengths)
    least = H.thresholds_of(ms.n_mats, thresholds)
    mat_hits = np.full(ms.n_mats + 1, -7, dtype=np.int64)
    args = (ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), width, ffi.ptr(offsets), total, int(do_mask), ms._h, ffi.ptr(least))
    if cap is None:
        rc = ffi.call("bxmi_twobit_pwm_hits", *args, 0, ffi.ptr(mat_hits), None, None, None, allow=(ffi.ERANGE,))
        assert rc == (ffi.ERANGE if mat_hits[-1] else ffi.OK)
        cap = int(mat_hits[-1])
    arrays = [np.full(lead + cap + tail, SENTINEL_BITS, dtype=np.uint32) for _ in range(3)]
    rc = ffi.call("bxmi_twobit_pwm_hits", *args, cap, ffi.ptr(mat_hits), *[ffi.ptr(a[lead:]) for a in arrays], allow=(ffi.ERANGE,))
    return rc, _checked(mat_hits, arrays, cap, lead, rc)


def hits_dev(tracks, ms, track_of, starts, thresholds, width=0, lengths=None, do_mask=True, cap=None, lead=3, tail=5):
    """bxmi_twobit_pwm_hits_dev on arrays in device memory, on the null stream"""
    from bxmi import _ffi as ffi

    t, s, offsets, total = _rows(track_of, starts, width, lengths)
    least = H.thresholds_of(ms.n_mats, thresholds)
    mat_hits = np.full(ms.n_mats + 1, -7, dtype=np.int64)
    rows = [ffi.DeviceArray.from_numpy(t), ffi.DeviceArray.from_numpy(s)] + ([ffi.DeviceArray.from_numpy(offsets)] if offsets is not None else [])
    args = (ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, len(t), width, rows[2].ptr if offsets is not None else None, total, int(do_mask),
            ms._h, ffi.ptr(least))
    if cap is None:
        rc = ffi.call("bxmi_twobit_pwm_hits_dev", *args, 0, ffi.ptr(mat_hits), None, None, None, None, allow=(ffi.ERANGE,))
        assert rc == (ffi.ERANGE if mat_hits[-1] else ffi.OK)
        cap = int(mat_hits[-1])
    out = [ffi.DeviceArray.from_numpy(np.full(lead + cap + tail, SENTINEL_BITS, dtype=np.uint32)) for _ in range(3)]
    rc = ffi.call("bxmi_twobit_pwm_hits_dev", *args, cap, ffi.ptr(mat_hits), *[a.ptr + 4 * lead for a in out], None, allow=(ffi.ERANGE,))
    ffi.call("bxmi_synchronize", None)
    arrays = [a.to_numpy(np.uint32) for a in out]
    for a in rows + out:
        a.free()
    return rc, _checked(mat_hits, arrays, cap, lead, rc)


def _checked(mat_hits, arrays, cap, lead, rc):
    """the sentinels around the hits -- around nothing when the call gave BXMI_ERANGE -- and the hits themselves"""
    from bxmi import _ffi as ffi

    found = int(mat_hits[-1])
    assert mat_hits[0] == 0 and (np.diff(mat_hits) >= 0).all() and (rc == ffi.ERANGE) == (found > cap)
    written = 0 if rc == ffi.ERANGE else found
    for a in arrays:
        assert (a[:lead] == SENTINEL_BITS).all() and (a[lead + written:] == SENTINEL_BITS).all(), "written outside the hits"
    body = [a[lead:lead + written] for a in arrays]
    return mat_hits, body[0].view(np.int32), body[1].view(np.int32), body[2].view(np.float32)


FORMS = (hits_host, hits_dev)


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", M.FILES)
def test_recorded_hits(name):
    """the recorded regions of a file as one ragged batch per do_mask setting and alphabet, at thresholds -inf, +inf and, per
    matrix, a score that occurs in its recorded answers: both forms against the model, every recorded (matrix, row) against the
    reference's own answer"""
    from bxmi import sequence

    checked = boundary = 0
    for do_mask in (True, False):
        genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
        tracks = list(genome.tracks.values())
        for names, seqs, track_of, starts, ends, want in P.recorded_batches(name, do_mask):
            mats = [P.matrix(k) for k in names]
            ms = device_set(mats)
            lengths = [e - s for s, e in zip(starts, ends)]
            offsets = offsets_of(lengths)
            planes = P.Scores(seqs).scores(track_of, starts, lengths, mats, do_mask)
            seen = H.occurring([np.concatenate([a for _, a in want[k]]) for k in names])
            for t in (-INF, INF, seen):
                expect = H.expected(planes, offsets, t)
                for form in FORMS:
                    rc, got = form(tracks, ms, track_of, starts, t, lengths=lengths, do_mask=do_mask)
                    H.assert_hits(got, expect, (name, do_mask, t, form.__name__))
                for m, k in enumerate(names):
                    part = slice(got[0][m], got[0][m + 1])
                    for row, answer in want[k]:
                        mine = got[1][part] == row
                        with np.errstate(invalid="ignore"):
                            at = np.flatnonzero(answer >= H.thresholds_of(len(names), t)[m])
                        assert np.array_equal(got[2][part][mine], at) and np.array_equal(P.bits(got[3][part][mine]), P.bits(answer[at])), (name, do_mask, k, row)
                        checked += 1
            boundary += int((got[3] == np.repeat(seen, np.diff(got[0]))).sum())
            ms.close()
        genome.close()
    assert checked == 3 * len(P.manifest()["files"][name]["entries"]) and boundary > 0


# ------------------------------------------------------------ structural cases against the model --
@pytest.fixture(scope="module")
def structural():
    from bxmi import sequence

    seqs = M.structural_sequences()
    tracks = [sequence.TwoBitTrack(s) for s in seqs]
    yield tracks, P.Scores(seqs)
    for t in tracks:
        t.close()


def test_ragged_structural_cases(structural):
    """pwm_model.ragged_case() with widths 1 and WIDTH_MAX in one handle, zero-length rows between rows; at -inf every scored element
    is a hit: all four elements of a thread, every lane, every wave.  BXMI_ERANGE at cap = total - 1 with the counts valid and
    the arrays untouched, success at cap = total and with room to spare; the same call twice gives the same arrays"""
    from bxmi import _ffi as ffi

    tracks, model = structural
    mats = P.structural_mats()
    track_of, starts, lengths = P.ragged_case()
    offsets = offsets_of(lengths)
    ms = device_set(mats)
    for do_mask in (True, False):
        planes = model.scores(track_of, starts, lengths, mats, do_mask)
        for t in (-INF, H.occurring(planes), [0.0, INF, -INF]):
            expect = H.expected(planes, offsets, t)
            for form in FORMS:
                rc, got = form(tracks, ms, track_of, starts, t, lengths=lengths, do_mask=do_mask)
                H.assert_hits(got, expect, (do_mask, t, form.__name__))
        assert H.expected(planes, offsets, -INF)[0][-1] == (~np.isnan(planes)).sum() > P.TILE
    expect = H.expected(model.scores(track_of, starts, lengths, mats, True), offsets, 0.0)
    total = int(expect[0][-1])
    for form in FORMS:
        rc, got = form(tracks, ms, track_of, starts, 0.0, lengths=lengths, cap=total - 1)
        assert rc == ffi.ERANGE and np.array_equal(got[0], expect[0]) and len(got[1]) == 0
        assert b"%d hits need larger arrays than cap=%d" % (total, total - 1) in ffi.load().bxmi_last_error()
        for cap, lead in ((total, 3), (total + 9, 0), (total, 1)):
            rc, again = form(tracks, ms, track_of, starts, 0.0, lengths=lengths, cap=cap, lead=lead)
            assert rc == ffi.OK
            H.assert_hits(again, expect, (form.__name__, cap))
    ms.close()


@pytest.mark.parametrize("width", (1, 37, P.TILE + 1))
def test_matrix_form_widths(structural, width):
    tracks, model = structural
    track_of, starts = M.matrix_case(width)
    offsets = np.arange(len(starts) + 1, dtype=np.int64) * width
    wmax = P.matrix("wmax")
    for mats in ([P.matrix("w20n"), P.matrix("w4n")], [P.matrix("w20lc")], [P.matrix(k) for k in ("ninf", "denorm", "zeros")],
                 [wmax, wmax.reverse_complement(), wmax, P.matrix("w1"), wmax.reverse_complement(), wmax]):  # (more values than stay in LDS)
        ms = device_set(mats)
        planes = model.scores(track_of, starts, [width] * len(starts), mats, True)
        for t in (-INF, H.occurring(planes)):
            for form in FORMS:
                rc, got = form(tracks, ms, track_of, starts, t, width=width)
                H.assert_hits(got, H.expected(planes, offsets, t), (width, len(mats), t, form.__name__))
        ms.close()


def test_nothing_to_find_and_bad_arguments(structural):
    from bxmi import _ffi as ffi
    from bxmi import motif

    tracks, _ = structural
    ms = device_set([P.matrix("w4"), P.matrix("w1")])
    track_of, starts, lengths = P.ragged_case()
    for form in FORMS:
        for args in (dict(lengths=lengths, thresholds=INF), dict(lengths=[0, 0], track_of=[0, 1], starts=[3, 4]), dict(width=5, track_of=[], starts=[])):
            args = dict(dict(track_of=track_of, starts=starts, thresholds=-INF), **args)
            rc, got = form(tracks, ms, args.pop("track_of"), args.pop("starts"), args.pop("thresholds"), **args)
            assert rc == ffi.OK and got[0].tolist() == [0, 0, 0] and len(got[1]) == 0
    # a NaN threshold is refused by its index; counts alone need no arrays
    lib = ffi.load()
    t, s = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    mat_hits = np.full(3, -7, dtype=np.int64)
    least = np.array([0.0, np.nan], dtype=np.float32)
    for rc in (lib.bxmi_twobit_pwm_hits(ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), 2, 9, None, 18, 1, ms._h, ffi.ptr(least), 0, ffi.ptr(mat_hits),
                                        None, None, None),
               lib.bxmi_twobit_pwm_hits_dev(ffi.handles(tracks), len(tracks), None, None, 2, 9, None, 18, 1, ms._h, ffi.ptr(least), 0, ffi.ptr(mat_hits),
                                            None, None, None, None)):
        assert rc == ffi.EINVAL and b"threshold[1] is NaN" in lib.bxmi_last_error() and (mat_hits == -7).all()
    got = motif.hits(tracks, [], [], [], ms, 0.0)
    assert got[0].tolist() == [0, 0, 0] and [len(a) for a in got[1:]] == [0, 0, 0] and got[3].dtype == np.float32
    with pytest.raises(ValueError):
        motif.hits(tracks, [0], [0], [9], ms, [1.0, 2.0, 3.0])
    with pytest.raises(ffi.BxmiError) as e:
        motif.hits(tracks, [len(tracks)], [0], [4], ms, 0.0)
    assert e.value.code == ffi.EINVAL
    ms.close()


# ------------------------------------------------------------ the seeded cases of tests/pwm_cases.py --
def check_case(case, thresholds, do_mask=True, tracks=None, ms=None):
    from bxmi import sequence

    own = tracks is None
    if own:
        tracks, ms = [sequence.TwoBitTrack(s) for s in case["seqs"]], device_set(case["mats"])
    try:
        texts = case.get("texts")
        acc, ok, offsets = PC.MODEL.planes(case["seqs"], case["mats"], case["track_of"], case["starts"], case["lengths"], do_mask=do_mask,
                                           texts=texts and texts[do_mask])
        out = []
        for t in thresholds:
            t = H.occurring(np.where(ok, acc, P.NAN)) if t is None else t
            expect = H.expected(acc, offsets, t, ok)
            for form in FORMS:
                rc, got = form(tracks, ms, case["track_of"], case["starts"], t, lengths=case["lengths"], do_mask=do_mask)
                H.assert_hits(got, expect, (t, do_mask, form.__name__))
            out.append((acc, ok, got))
        return out
    finally:
        if own:
            ms.close()
            for t in tracks:
                t.close()


def test_one_hit_per_row_on_every_lane():
    """pwm_cases.lane_case: 1024 rows of one tile, row i's only 1.0 under the first matrix at offset i: one hit from every lane
    of every wave and from each of a thread's four elements, each the only hit of its tile"""
    case = PC.lane_case()
    (_, _, got), = check_case(case, (1.0,))
    assert got[0][1] == P.TILE and np.array_equal(got[1][:P.TILE], np.arange(P.TILE)) and np.array_equal(got[2][:P.TILE], np.arange(P.TILE))


def test_extremes_and_arithmetic_nans():
    """arithmetic NaNs are never hits, not even at -inf; +inf scores are hits at +inf; -inf scores are hits only at -inf"""
    case = PC.extremes_case()
    for do_mask in (True, False):
        (acc, ok, low), (_, _, high), (_, _, some) = check_case(case, (-INF, INF, -3.0e38), do_mask)
        arith = int((ok & np.isnan(acc)).sum())
        assert arith > 0 and low[0][-1] == ok.sum() - arith and np.isneginf(low[3]).any()
        assert high[0][-1] == (ok & np.isposinf(acc)).sum() > 0 and np.isposinf(high[3]).all()
        assert not np.isneginf(some[3]).any() and some[0][-1] == low[0][-1] - np.isneginf(low[3]).sum()


@pytest.mark.parametrize("name", ("mats_max", "lds_plus_4", "cols16_g_top"))
def test_seeded_matrix_sets(name):
    """PW_MATS_MAX matrices; the smallest set staged matrix by matrix; 16 columns with column 15 in use"""
    check_case(PC.matrix_set_case(name), (None,))


def test_more_tiles_than_fit_the_device_at_once():
    """1.5 x (compute units x 8) tiles, more workgroups than are resident together, in one long row and in a few thousand rows:
    every tile's count and base at its own place, whenever its workgroup ran"""
    import ctypes as C

    from bxmi import _ffi

    dev, cus = C.c_int(0), C.c_int(0)
    _ffi.call("bxmi_get_device", C.byref(dev))
    _ffi.call("bxmi_device_info", dev.value, None, 0, C.byref(cus), None)
    tiles = cus.value * 8 + cus.value * 4
    assert cus.value > 0
    check_case(PC.long_row_case(tiles), (None,))
    check_case(PC.many_rows_case(tiles), (None, -INF))


def test_one_row_of_300000_bases():
    """many tiles of one row: every tile's hits land behind those of the tiles before it"""
    rng = np.random.default_rng(570)
    seq = K.random_sequence(rng, 300_500, 300, 900)
    w20 = P.matrix("w20")
    case = dict(seqs=[seq], mats=[w20, w20.reverse_complement()], track_of=[0], starts=[200], lengths=[300_000])
    for _, _, got in check_case(case, (None, -INF)):
        assert got[0][-1] > 1000 and (np.diff(got[2][:got[0][1]]) > 0).all()


def test_hits_at_the_top_of_int32():
    """pwm_cases.top_case on twobit_cases.TopSequence, 2^31 - 1 bases: positions, the packed word and the blocks' edges next to
    the top of int32; and the Python layer, which clips the regions, against the nonzero of its own `scores`"""
    from bxmi import motif, sequence

    case = PC.top_case()
    tracks, ms = [sequence.TwoBitTrack(s) for s in case["seqs"]], device_set(case["mats"])
    try:
        (acc, ok, _), = check_case(case, (None,), tracks=tracks, ms=ms)
        t = H.occurring(np.where(ok, acc, P.NAN))
        ends = np.minimum(case["starts"] + case["lengths"], 2 ** 31 - 1)  # (the size: what lies beyond is clipped anyway)
        planes, offsets = motif.scores(tracks, case["track_of"], case["starts"], ends, ms)
        got = motif.hits(tracks, case["track_of"], case["starts"], ends, ms, t)
        H.assert_hits(got, H.expected(planes, offsets, t), "python layer")
        assert got[0][-1] > 0
    finally:
        ms.close()
        for t in tracks:
            t.close()


def test_python_layer_equals_the_nonzero_of_scores():
    """motif.hits and TwoBitSet.hits on pwm_cases.matrix_set_case at its defaults: a scalar threshold and one per matrix"""
    from bxmi import motif, sequence

    case = PC.matrix_set_case("cols16_all")
    tracks, ms = [sequence.TwoBitTrack(s) for s in case["seqs"]], device_set(case["mats"])
    try:
        ends = case["starts"] + case["lengths"]
        planes, offsets = motif.scores(tracks, case["track_of"], case["starts"], ends, ms)
        for t in (0.0, H.occurring(planes), -INF):
            H.assert_hits(motif.hits(tracks, case["track_of"], case["starts"], ends, ms, t), H.expected(planes, offsets, t), t)
        got = motif.hits(tracks, case["track_of"], case["starts"], ends, ms.matrices, 0.0)  # matrices put on the device for the call
        H.assert_hits(got, H.expected(planes, offsets, 0.0), "matrices")
    finally:
        ms.close()
        for t in tracks:
            t.close()


# ------------------------------------------------------------ device entry points on torch tensors --
def test_hits_dev_on_torch_tensors():
    """motif.hits_dev / TwoBitSet.hits_dev with and without max_hits, on torch's current stream and on a stream of the caller's,
    against the nonzero of scores_dev, on pwm_cases.matrix_set_case at its defaults and on pwm_cases.top_case(); in a process of
    its own: torch brings its own HIP runtime"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import pwm_cases as PC
import pwm_hits_cases as H
import pwm_model as P
from bxmi import _ffi, motif, sequence

def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).astype(np.int32)).cuda()

side = torch.cuda.Stream()
for case in (PC.matrix_set_case("cols16_all"), PC.top_case()):
    tracks = [sequence.TwoBitTrack(s) for s in case["seqs"]]
    ms = motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in case["mats"]])
    ends = np.minimum(np.asarray(case["starts"]) + np.asarray(case["lengths"]), 2 ** 31 - 1)
    d = [dev_i32(case["track_of"]), dev_i32(case["starts"]), dev_i32(ends)]
    planes, offsets = motif.scores_dev(tracks, *d, ms)
    torch.cuda.synchronize()
    planes, offsets = planes.cpu().numpy(), offsets.cpu().numpy()
    for t in (H.occurring(planes), 0.0):
        want = H.expected(planes, offsets, t)
        total = int(want[0][-1])
        assert total > 0
        for max_hits, stream in ((None, None), (total, None), (total + 1000, side.cuda_stream), (None, side.cuda_stream)):
            got = motif.hits_dev(tracks, *d, ms, t, max_hits=max_hits, stream=stream)
            churn = [torch.zeros(total + 7, dtype=torch.int32, device="cuda") for _ in range(4)]  # (what could take a freed block)
            side.synchronize()
            torch.cuda.synchronize()
            assert isinstance(got[0], np.ndarray) and all(a.is_cuda for a in got[1:])
            H.assert_hits((got[0],) + tuple(a.cpu().numpy() for a in got[1:]), want, (t, max_hits))
        try:
            motif.hits_dev(tracks, *d, ms, t, max_hits=total - 1)
            raise SystemExit("hits that do not fit were accepted")
        except _ffi.BxmiError as err:
            assert err.code == _ffi.ERANGE and str(np.diff(want[0]).tolist()) in str(err) and "max_hits = %d" % (total - 1) in str(err), str(err)
    got = motif.hits_dev(tracks, d[0][:0], d[1][:0], d[2][:0], ms, 0.0)
    assert got[0].tolist() == [0] * (ms.n_mats + 1) and tuple(got[1].shape) == (0,)
    ms.close()
    for t in tracks:
        t.close()

# through TwoBitSet
case = PC.matrix_set_case("cols16_all")
genome = sequence.TwoBitSet({"a": case["seqs"][0], "b": case["seqs"][1]})
ms = motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in case["mats"]])
d = [dev_i32(case["track_of"]), dev_i32(case["starts"]), dev_i32(np.asarray(case["starts"]) + np.asarray(case["lengths"]))]
planes, offsets = genome.scores_dev(*d, ms)
got = genome.hits_dev(*d, ms, 0.0)
torch.cuda.synchronize()
H.assert_hits((got[0],) + tuple(a.cpu().numpy() for a in got[1:]), H.expected(planes.cpu().numpy(), offsets.cpu().numpy(), 0.0), "TwoBitSet")
ms.close()
genome.close()
print("pwm hits dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "pwm hits dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ------------------------------------------------------------ the command line --
def test_command_line_prints_the_sites(tmp_path):
    """BED6 lines computed from genome.scores: ordered by BED row, position, "+" before "-"; with and without -r and -u"""
    from bxmi import motif, sequence
    from bxmi.cli import twobit_pwm_hits as cli

    name = "multi.2bit"
    mat = P.matrix("w4")
    path = tmp_path / "matrix.txt"
    path.write_text("".join(mat.alphabet) + "\n" + "".join(" ".join(repr(float(x)) for x in row) + "\n" for row in mat.rows))
    rows = [("ckpt", 990, 1030), ("odd", 0, 41), ("ckpt", 2565, 2600), ("empty", 0, 5), ("chrNone", 7, 9), ("odd", 38, 41), ("ckpt", 1000, 1020)]
    bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r for r in rows)
    dmat = motif.ScoringMatrix(mat.alphabet, mat.rows)
    for flags, do_mask, mats in (([], True, [dmat]), (["-u"], False, [dmat]), (["-r"], True, [dmat, dmat.reverse_complement()]),
                                 (["-u", "-r"], False, [dmat, dmat.reverse_complement()])):
        genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
        planes, offsets = genome.scores([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], mats)
        genome.close()
        threshold = float(np.sort(planes[0][~np.isnan(planes[0])])[-8])  # (a score that occurs: a handful of sites)
        lines = []
        for i, (chrom, start, end) in enumerate(rows):
            for j in range(int(offsets[i + 1] - offsets[i])):
                for m in range(len(mats)):
                    x = planes[m, offsets[i] + j]
                    if x >= threshold:
                        lines.append("%s\t%d\t%d\t%s:%d-%d\t%s\t%s\n" % (chrom, start + j, start + j + mat.width, chrom, start, end, repr(float(x)), "+-"[m]))
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), str(path), repr(threshold)] + flags, stdin=io.StringIO(bed), out=out)
        assert out.getvalue() == "".join(lines) and len(lines) >= 8, flags
        if "-r" in flags:
            assert any(ln.endswith("-\n") for ln in lines) and any(ln.endswith("+\n") for ln in lines)
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), str(path), "inf"] + flags, stdin=io.StringIO(bed), out=out)
        assert out.getvalue() == ""
