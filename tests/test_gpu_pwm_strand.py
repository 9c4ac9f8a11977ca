"""
Strand-aware position weight matrices on the device (bxmi_twobit_pwm_scores_strand, _best_strand, _hits_strand and their _dev forms,
the `strands` keyword of bxmi.motif and TwoBitSet, motif.site_starts, the -s flag of both command lines) against the answers recorded
from the reference (tests/golden/pwm_strand) and the model of tests/pwm_strand_model.py on the seeded cases of
tests/pwm_strand_cases.py: planes bit for bit, best hits and hits exactly.  The host forms write into arrays pre-filled with garbage,
the _dev forms between sentinels that must be intact.  tests/test_pwm_strand_kernel_host.py runs the same kernels on the host.
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
import pwm_strand_cases as C
import pwm_strand_model as PS
import strand_model as S
import twobit_cases as K
import twobit_model as M
from pwm_hits_cases import INF, offsets_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_pwm_scores_strand_dev", "bxmi_twobit_pwm_best_strand_dev", "bxmi_twobit_pwm_hits_strand_dev")
GARBAGE = 0x5A5A5A5A
SENTINEL = 0xEEEEEEEE


def i8(strands):
    return np.ascontiguousarray(strands, dtype=np.int8)


class Held:
    """the tracks and the matrix sets that the cases of a test put on the device, each once, all closed again whatever happens"""

    def __init__(self):
        self.tracks, self.sets = {}, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for _, handle in list(self.tracks.values()) + list(self.sets.values()):
            handle.close()

    def tracks_of(self, seqs):
        from bxmi import sequence

        for s in seqs:
            if id(s) not in self.tracks:
                self.tracks[id(s)] = (s, sequence.TwoBitTrack(s))
        return [self.tracks[id(s)][1] for s in seqs]

    def set_of(self, mats):
        from bxmi import motif

        key = tuple(id(m) for m in mats)
        if key not in self.sets:
            self.sets[key] = (mats, motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mats]))
        return self.sets[key][1]


def on_device(arrays):
    from bxmi import _ffi as ffi

    return [ffi.DeviceArray.from_numpy(a) if a is not None and len(a) else None for a in arrays]


def ptr_of(a):
    return a.ptr if a is not None else None


def banded(cells, lead, tail, fill=GARBAGE):
    """a device allocation of 32-bit words: sentinels around garbage -> (array, check() -> the body, the sentinels verified)"""
    from bxmi import _ffi as ffi

    filled = np.full(lead + cells + tail, SENTINEL, dtype=np.uint32)
    filled[lead:lead + cells] = fill
    out = ffi.DeviceArray.from_numpy(filled)

    def check(written=cells):
        got = out.to_numpy(np.uint32)
        out.free()
        assert (got[:lead] == SENTINEL).all() and (got[lead + cells:] == SENTINEL).all(), "written outside the output"
        assert (got[lead + written:lead + cells] == fill).all(), "written beyond what was asked for"
        return got[lead:lead + written]

    return out, check


class OnDevice:
    """one form of the library as a device of pwm_strand_cases.check: the host forms or the _dev entry points by their C names.
    strands None goes to the unstranded entry point.  `misalign` moves the _dev form's planes off a 16-byte boundary; `slack` adds to
    the _dev form's bound of the total; the slabs and the grids are the library's own."""

    def __init__(self, held, dev):
        self.held, self.dev = held, dev

    def _rows(self, seqs, mats, track_of, starts, strands, lengths, width):
        tracks, ms = self.held.tracks_of(seqs), self.held.set_of(mats)
        t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
        offsets = None if lengths is None else offsets_of(lengths)
        total = len(t) * width if offsets is None else int(offsets[-1])
        return tracks, ms, t, s, (None if strands is None else i8(strands)), offsets, total

    def _call(self, name, tracks, t, s, m, offsets, width, total, tail):
        """name: the unstranded host entry point; tail: the arguments after `total` -> rc.  The device form's rows live for the call."""
        from bxmi import _ffi as ffi

        name = name + ("_strand" if m is not None else "") + ("_dev" if self.dev else "")
        if not self.dev:
            return ffi.call(name, ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), *((ffi.ptr(m),) if m is not None else ()), len(t), width,
                            ffi.ptr(offsets), total, *tail, allow=(ffi.ERANGE,))
        held = on_device([t, s, m, offsets])
        try:
            rc = ffi.call(name, ffi.handles(tracks), len(tracks), ptr_of(held[0]), ptr_of(held[1]), *((ptr_of(held[2]),) if m is not None else ()), len(t),
                          width, ptr_of(held[3]), total, *tail, None, allow=(ffi.ERANGE,))
            ffi.call("bxmi_synchronize", None)
            return rc
        finally:
            for a in held:
                if a is not None:
                    a.free()

    def scores(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, misalign=0, **_):
        from bxmi import _ffi as ffi

        tracks, ms, t, s, m, offsets, total = self._rows(seqs, mats, track_of, starts, strands, lengths, width)
        cells = ms.n_mats * total
        if not self.dev:
            out = np.full(cells, GARBAGE, dtype=np.uint32)
            self._call("bxmi_twobit_pwm_scores", tracks, t, s, m, offsets, width, total, (int(do_mask), ms._h, ffi.ptr(out)))
            return out.view(np.float32).reshape(ms.n_mats, total)
        out, check = banded(cells, 4 + misalign, 7)
        self._call("bxmi_twobit_pwm_scores", tracks, t, s, m, offsets, width, total, (int(do_mask), ms._h, out.ptr + 4 * (4 + misalign)))
        return check().view(np.float32).reshape(ms.n_mats, total)

    def best(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, slack=0, **_):
        from bxmi import _ffi as ffi

        tracks, ms, t, s, m, offsets, total = self._rows(seqs, mats, track_of, starts, strands, lengths, width)
        cells = ms.n_mats * len(t)
        if not self.dev:
            score, pos = np.full(cells, GARBAGE, dtype=np.uint32), np.full(cells, GARBAGE, dtype=np.uint32)
            self._call("bxmi_twobit_pwm_best", tracks, t, s, m, offsets, width, total, (int(do_mask), ms._h, ffi.ptr(score), ffi.ptr(pos)))
        else:
            (d_score, check_score), (d_pos, check_pos) = banded(cells, 3, 5), banded(cells, 5, 3)
            self._call("bxmi_twobit_pwm_best", tracks, t, s, m, offsets, width, total + (slack if offsets is not None else 0),
                       (int(do_mask), ms._h, d_score.ptr + 12, d_pos.ptr + 20))
            score, pos = check_score(), check_pos()
        return score.view(np.float32).reshape(ms.n_mats, len(t)), pos.view(np.int32).reshape(ms.n_mats, len(t))

    def hits(self, seqs, mats, track_of, starts, strands, thresholds, lengths=None, width=0, do_mask=True, cap=None, want_rc=None, **_):
        from bxmi import _ffi as ffi

        tracks, ms, t, s, m, offsets, total = self._rows(seqs, mats, track_of, starts, strands, lengths, width)
        least = H.thresholds_of(ms.n_mats, thresholds)
        mat_hits = np.full(ms.n_mats + 1, -7, dtype=np.int64)
        head = (int(do_mask), ms._h, ffi.ptr(least))
        if cap is None:  # the counts alone first: cap == 0 with NULL arrays
            rc = self._call("bxmi_twobit_pwm_hits", tracks, t, s, m, offsets, width, total, head + (0, ffi.ptr(mat_hits), None, None, None))
            assert rc == (ffi.ERANGE if mat_hits[-1] else ffi.OK)
            cap = int(mat_hits[-1])
        lead = 3
        if not self.dev:
            arrays = [np.full(lead + cap + 5, SENTINEL, dtype=np.uint32) for _ in range(3)]
            rc = self._call("bxmi_twobit_pwm_hits", tracks, t, s, m, offsets, width, total, head + (cap, ffi.ptr(mat_hits)) + tuple(ffi.ptr(a[lead:]) for a in arrays))
            found = int(mat_hits[-1])
            written = 0 if rc == ffi.ERANGE else found
            for a in arrays:
                assert (a[:lead] == SENTINEL).all() and (a[lead + written:] == SENTINEL).all(), "written outside the hits"
            body = [a[lead:lead + written] for a in arrays]
        else:
            made = [banded(cap, lead, 5, SENTINEL) for _ in range(3)]
            rc = self._call("bxmi_twobit_pwm_hits", tracks, t, s, m, offsets, width, total, head + (cap, ffi.ptr(mat_hits)) + tuple(a.ptr + 4 * lead for a, _ in made))
            found = int(mat_hits[-1])
            written = 0 if rc == ffi.ERANGE else found
            body = [check(written) for _, check in made]
        assert (rc == ffi.ERANGE) == (found > cap) and mat_hits[0] == 0
        if want_rc is not None:
            assert rc == want_rc
        return mat_hits, body[0].view(np.int32), body[1].view(np.int32), body[2].view(np.float32)


def both_forms(held):
    return [OnDevice(held, False), OnDevice(held, True)]


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", M.FILES)
def test_recorded_cases(name):
    """the recorded regions of a file as one ragged all-minus batch per do_mask setting and alphabet through TwoBitSet, the host
    forms and the _dev forms: the reference's own answers for the reverse complement, their best hits and their hits"""
    from bxmi import motif, sequence

    checked = 0
    with Held() as held:
        for do_mask in (True, False):
            genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
            for names, seqs, track_of, starts, ends, want in PS.recorded_batches(name, do_mask):
                mats = [P.matrix(k) for k in names]
                lengths = [e - s for s, e in zip(starts, ends)]
                offsets = offsets_of(lengths)
                minus = ["-"] * len(track_of)
                dmats = [motif.ScoringMatrix(m.alphabet, m.rows) for m in mats]
                got, off = genome.scores(track_of, starts, ends, dmats, strands=minus)
                top, at = genome.best(track_of, starts, ends, dmats, strands=minus)
                assert np.array_equal(off, offsets)
                seen = H.occurring([np.concatenate([a for _, a in want[k]]) for k in names])
                found = genome.hits(track_of, starts, ends, dmats, seen, strands=minus)
                for dev in both_forms(held):
                    assert np.array_equal(P.bits(dev.scores(seqs, mats, track_of, starts, [1] * len(minus), lengths, do_mask=do_mask)), P.bits(got))
                    H.assert_hits(dev.hits(seqs, mats, track_of, starts, [1] * len(minus), seen, lengths, do_mask=do_mask), found)
                for m, k in enumerate(names):
                    part = slice(found[0][m], found[0][m + 1])
                    for row, answer in want[k]:
                        assert np.array_equal(P.bits(got[m, offsets[row]:offsets[row + 1]]), P.bits(answer)), (name, do_mask, k, row)
                        score, pos = P.best_of(answer)
                        assert P.bits(top[m, row]) == P.bits(score) and at[m, row] == pos, (name, do_mask, k, row)
                        with np.errstate(invalid="ignore"):
                            where = np.flatnonzero(answer >= seen[m])
                        mine = found[1][part] == row
                        assert np.array_equal(found[2][part][mine], where) and np.array_equal(P.bits(found[3][part][mine]), P.bits(answer[where]))
                        checked += 1
            genome.close()
    assert checked == len(PS.manifest()["files"][name]["entries"])


# ------------------------------------------------------------ the seeded cases, both forms --
@pytest.mark.parametrize("make", (C.short_rows_case, C.boundary_case, C.edge_case, C.palindrome_case, C.many_rows_case, C.small_top_case, C.extremes_case),
                         ids=lambda f: f.__name__)
def test_structural_cases(make):
    with Held() as held:
        C.check(both_forms(held), make())


@pytest.mark.parametrize("width", (5, 37, P.TILE + 1))
def test_matrix_form(width):
    with Held() as held:
        C.check(both_forms(held), C.matrix_form_case(width))


@pytest.mark.parametrize("name", C.SETS)
def test_seeded_matrix_sets(name):
    with Held() as held:
        C.check(both_forms(held), C.set_case(name))


def test_best_ties_mirrored_and_more_tiles_than_the_grid():
    """the first offset OF THE STRAND'S STRING wins on every lane; one minus row of 1.5 x (compute units x 8) tiles -- more tiles
    than the grid of the best hits -- for best and hits, the total only a bound"""
    import ctypes

    from bxmi import _ffi as ffi

    dev, cus = ctypes.c_int(0), ctypes.c_int(0)
    ffi.call("bxmi_get_device", ctypes.byref(dev))
    ffi.call("bxmi_device_info", dev.value, None, 0, ctypes.byref(cus), None)
    with Held() as held:
        C.check(both_forms(held), C.lane_case(np.arange(P.TILE)), planes=False, hits=False)
        tiles = 12 * cus.value  # 1.5 x (compute units x 8): the case tests/test_gpu_pwm.py walks on the plus strand
        assert cus.value > 0
        case = C.long_row_case(tiles)
        assert case["lengths"][2] > tiles * P.TILE and case["strands"][2] == 1
        C.check(both_forms(held), case, planes=False)


def test_hits_capacity_refusals_and_repeat():
    """cap one short (BXMI_ERANGE, counts valid, arrays untouched), cap == 0, room to spare, the same list twice; a strand entry
    other than 0 or 1 is refused by the host forms with the outputs untouched, and is minus to the device forms"""
    from bxmi import _ffi as ffi

    case = C.boundary_case()
    args = (case["seqs"], case["mats"], case["track_of"], case["starts"])
    acc, ok, offsets, top, _ = C.want_of(case, True)
    want = H.expected(np.where(ok, acc, P.NAN), offsets, 0.0, ok)
    total = int(want[0][-1])
    assert total > P.TILE
    with Held() as held:
        for dev in both_forms(held):
            got = dev.hits(*args, case["strands"], 0.0, case["lengths"], cap=total - 1, want_rc=ffi.ERANGE)
            assert np.array_equal(got[0], want[0]) and len(got[1]) == 0
            got = dev.hits(*args, case["strands"], 0.0, case["lengths"], cap=0, want_rc=ffi.ERANGE)
            assert np.array_equal(got[0], want[0])
            first = dev.hits(*args, case["strands"], 0.0, case["lengths"], cap=total + 9, want_rc=ffi.OK)
            again = dev.hits(*args, case["strands"], 0.0, case["lengths"], cap=total, want_rc=ffi.OK)
            H.assert_hits(first, want), H.assert_hits(again, want)
        host, dev = both_forms(held)
        bad = list(case["strands"])
        bad[5] = 2
        tracks, ms, t, s, m, off, n_total = host._rows(*args, bad, case["lengths"], 0)
        out = np.full(ms.n_mats * n_total, GARBAGE, dtype=np.uint32)
        score, pos = np.full(ms.n_mats * len(t), GARBAGE, dtype=np.uint32), np.full(ms.n_mats * len(t), GARBAGE, dtype=np.uint32)
        mat_hits, arrays = np.full(ms.n_mats + 1, -7, dtype=np.int64), [np.full(8, GARBAGE, dtype=np.uint32) for _ in range(3)]
        least = H.thresholds_of(ms.n_mats, 0.0)
        rows = (ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), ffi.ptr(m), len(t), 0, ffi.ptr(off), n_total, 1, ms._h)
        for name, tail in (("bxmi_twobit_pwm_scores_strand", (ffi.ptr(out),)), ("bxmi_twobit_pwm_best_strand", (ffi.ptr(score), ffi.ptr(pos))),
                           ("bxmi_twobit_pwm_hits_strand", (ffi.ptr(least), 8, ffi.ptr(mat_hits)) + tuple(ffi.ptr(a) for a in arrays))):
            with pytest.raises(ffi.BxmiError) as e:
                ffi.call(name, *rows, *tail)
            assert e.value.code == ffi.EINVAL and "strand[5] = 2 of row 5" in str(e.value) and name + ":" in str(e.value)
        assert (out == GARBAGE).all() and (score == GARBAGE).all() and (pos == GARBAGE).all() and (mat_hits == -7).all() and all((a == GARBAGE).all() for a in arrays)
        # the device forms do not check: any non-zero entry is minus
        odd = [int(v) * 77 for v in case["strands"]]
        PC.assert_best(dev.best(*args, odd, case["lengths"]), top)


def test_a_host_call_past_one_slab_with_mixed_strands():
    """bxmi_twobit_pwm_scores_strand over more than PW_SLAB elements: the strand array is cut with the rows of every slab, and a row
    that lies in two slabs keeps its strand in both"""
    from bxmi import motif, sequence

    rng = np.random.default_rng(670)
    seq = PC.sparse_sequence(rng, 60_000)
    mats = [P.matrix("w20")]
    n = 2 * P.PW_SLAB // 3000 + 40
    lengths = rng.integers(2500, 3500, n)
    assert lengths.sum() > P.PW_SLAB + 10 * P.TILE and P.slab_elements(1) == P.PW_SLAB
    starts = rng.integers(0, seq.size - 3500, n)
    strands = rng.integers(0, 2, n)
    track = sequence.TwoBitTrack(seq)
    try:
        got, offsets = motif.scores([track], [0] * n, starts, starts + lengths, [motif.ScoringMatrix(mats[0].alphabet, mats[0].rows)], strands=strands.tolist())
        cut = int(np.searchsorted(offsets, P.PW_SLAB, side="right")) - 1
        assert offsets[cut] < P.PW_SLAB < offsets[cut + 1]  # a row across the slab boundary
        whole = M.letters(seq, True)
        for i in list(range(6)) + list(range(cut - 3, cut + 4)) + list(range(n - 6, n)):  # (the model row by row: the ends and the boundary)
            row = whole[starts[i]:starts[i] + lengths[i]]
            assert np.array_equal(P.bits(got[0, offsets[i]:offsets[i + 1]]), P.bits(PS.score(mats[0], row, bool(strands[i])))), i
        assert len({int(strands[i]) for i in range(cut - 3, cut + 4)}) == 2
    finally:
        track.close()


def test_a_minus_row_at_the_top_of_int32():
    """twobit_cases.TopSequence, 2^31 - 1 bases: pwm_cases.top_case's rows, every one minus -- positions reach 2^31 - 2, cross the
    size, begin at it -- and a minus row that ends exactly at the size"""
    case = dict(PC.top_case())
    n = len(case["track_of"])
    top = K.top_sequence()
    assert any(int(s) + int(k) - 1 == 2 ** 31 - 2 for s, k in zip(case["starts"], case["lengths"]))
    case.update(strands=[1] * n, runs=({},), name="top")
    with Held() as held:
        C.check(both_forms(held), case)


# ------------------------------------------------------------ the Python layers on torch tensors --
def test_dev_forms_on_torch_tensors():
    """score_matrix_dev / scores_dev / best_dev / hits_dev with `strands` as int8, uint8 and bool tensors, on torch's current stream
    and on a side stream, with `out` given, through TwoBitSet as well, in a process of its own (torch brings its own HIP runtime)"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import pwm_cases as PC, pwm_hits_cases as H, pwm_model as P, pwm_strand_cases as C, pwm_strand_model as PS
from bxmi import motif, sequence

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

def bits(t):
    return P.bits(t.cpu().numpy())

case = C.boundary_case()
seqs, mats = case["seqs"], case["mats"]
tracks = [sequence.TwoBitTrack(s) for s in seqs]
ms = motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mats])
side = torch.cuda.Stream()
t, s, n, minus = case["track_of"], case["starts"], case["lengths"], case["strands"]
ends = [a + b for a, b in zip(s, n)]
first, clipped = P.clipped(seqs, t, s, ends)
d = [dev_i32(t, 1), dev_i32(s, 3), dev_i32(ends, 1)]
tensors = [torch.tensor(minus, dtype=torch.bool, device="cuda"), torch.tensor(minus, dtype=torch.int8, device="cuda"),
           torch.tensor([7] + [int(m) * 200 for m in minus], dtype=torch.uint8, device="cuda")[1:]]  # (any non-zero entry is minus)
acc, ok, offsets = PS.MODEL.planes(seqs, mats, t, first, minus, clipped)
want = np.where(ok, acc, P.NAN)
top = PC.MODEL.best_of_planes(acc, ok, offsets)
hits = H.expected(want, offsets, 0.0, ok)
for which, st in enumerate(tensors):
    got, off = motif.scores_dev(tracks, *d, ms, strands=st)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), P.bits(want)) and np.array_equal(off.cpu().numpy(), offsets), which
    score, pos = motif.best_dev(tracks, *d, ms, stream=side.cuda_stream, strands=st)
    side.synchronize()
    assert np.array_equal(bits(score), P.bits(top[0])) and np.array_equal(pos.cpu().numpy(), top[1]), which
    found = motif.hits_dev(tracks, *d, ms, 0.0, stream=side.cuda_stream, strands=st)
    side.synchronize()
    H.assert_hits((found[0],) + tuple(x.cpu().numpy() for x in found[1:]), hits, which)
plus, _ = motif.scores_dev(tracks, *d, ms)
torch.cuda.synchronize()
assert not np.array_equal(bits(plus), P.bits(want))
# windows of one width, `out` given on a side stream, through TwoBitSet
genome = sequence.TwoBitSet({"blocks": seqs[0], "odd": seqs[1]}, do_mask=True)
for width in (37, P.TILE + 1):
    mcase = C.matrix_form_case(width)
    keep = [i for i, q in enumerate(mcase["track_of"]) if q in (0, 1, -1)]
    tm, sm, mm = [mcase["track_of"][i] for i in keep], [mcase["starts"][i] for i in keep], [mcase["strands"][i] for i in keep]
    gms = motif.MatrixSet([motif.ScoringMatrix(m.alphabet, m.rows) for m in mcase["mats"]])
    want_m = PS.MODEL.scores(seqs, mcase["mats"], tm, sm, mm, width=width).reshape(len(mcase["mats"]), len(tm), width)
    st = torch.tensor(mm, dtype=torch.bool, device="cuda")
    out = torch.full(want_m.shape, 77.0, dtype=torch.float32, device="cuda")
    res = genome.score_matrix_dev(dev_i32(tm, 2), dev_i32(sm, 1), width, gms, stream=side.cuda_stream, out=out, strands=st)
    side.synchronize()
    assert res is out and np.array_equal(bits(out), P.bits(want_m)), width
    got = motif.score_matrix_dev(list(genome.tracks.values()), dev_i32(tm, 2), dev_i32(sm, 1), width, gms, strands=st.to(torch.int8))
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), P.bits(want_m)), width
    gms.close()
for bad in (torch.tensor(minus, dtype=torch.int32, device="cuda"), torch.tensor(minus, dtype=torch.int8), tensors[1][:-1], minus):
    for fn in (motif.scores_dev, motif.best_dev):
        try:
            fn(tracks, *d, ms, strands=bad)
        except ValueError:
            pass
        else:
            raise AssertionError("a bad strands argument was taken")
genome.close()
ms.close()
for tr in tracks:
    tr.close()
print("torch strands ok")
'''
    out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("torch strands ok"), (out.stdout[-1000:], out.stderr[-3000:])


# ------------------------------------------------------------ module functions, TwoBitSet, the command lines --
def test_module_functions_and_site_starts():
    """motif.scores / score_matrix / best / hits with "+" / "-" strands on host arrays; the genomic start of every best site and hit
    (motif.site_starts) reverse-complements to the window of the strand's string"""
    from bxmi import motif, sequence

    case = C.boundary_case()
    seqs, mats = case["seqs"], [m for m in case["mats"] if m.width == 20]
    t, s, n, minus = case["track_of"], case["starts"], case["lengths"], case["strands"]
    ends = [a + b for a, b in zip(s, n)]
    first, clipped = P.clipped(seqs, t, s, ends)
    signs = ["-" if m else "+" for m in minus]
    tracks = [sequence.TwoBitTrack(q) for q in seqs]
    dmats = [motif.ScoringMatrix(m.alphabet, m.rows) for m in mats]
    try:
        acc, ok, offsets = PS.MODEL.planes(seqs, mats, t, first, minus, clipped)
        want = np.where(ok, acc, P.NAN)
        got, off = motif.scores(tracks, t, s, ends, dmats, strands=signs)
        assert np.array_equal(P.bits(got), P.bits(want)) and np.array_equal(off, offsets)
        score, pos = motif.best(tracks, t, s, ends, dmats, strands=signs)
        PC.assert_best((score, pos), PC.MODEL.best_of_planes(acc, ok, offsets))
        found = motif.hits(tracks, t, s, ends, dmats, 2.0, strands=np.array(minus, dtype=bool))
        H.assert_hits(found, H.expected(want, offsets, 2.0, ok))
        assert found[0][-1] > 20
        letters = PC.letters_of(seqs).letters
        sites = motif.site_starts(np.asarray(first)[found[1]], np.asarray(clipped)[found[1]], found[2], 20, np.asarray(minus)[found[1]])
        for k in range(0, len(sites), max(len(sites) // 60, 1)):
            i = int(found[1][k])
            window = letters.row(int(t[i]), int(sites[k]), 20, True, 0)
            assert P.bits(mats[0].score(S.reverse_complement(window) if minus[i] else window)[0]) == P.bits(found[3][k]), k
        width = 37
        mcase = C.matrix_form_case(width)
        got = motif.score_matrix(tracks, mcase["track_of"], mcase["starts"], width, [motif.ScoringMatrix(m.alphabet, m.rows) for m in mcase["mats"]],
                                 strands=mcase["strands"])
        want_m = PS.MODEL.scores(seqs, mcase["mats"], mcase["track_of"], mcase["starts"], mcase["strands"], width=width)
        assert np.array_equal(P.bits(got.reshape(len(mcase["mats"]), -1)), P.bits(want_m))
        with pytest.raises(ValueError):
            motif.scores(tracks, t, s, ends, dmats, strands=["+"] * (len(t) - 1))
    finally:
        for tr in tracks:
            tr.close()


def test_command_lines_with_the_strand_flag(tmp_path):
    """both command lines with -s on a BED with "+", "-", "." and a missing column: the scores in the strand's order with the strand
    in the header, -b the offset in the strand's string; the sites of twobit_pwm_hits -s at the model's genomic coordinates, the
    strand flipped for the -r matrix, in BED order, then by genomic start, "+" before "-" """
    from bxmi.cli import twobit_pwm_hits as hits_cli
    from bxmi.cli import twobit_pwm_scores as scores_cli

    name = "multi.2bit"
    seqs = M.read(name)
    names = list(seqs)
    mat = P.matrix("w4")
    path = tmp_path / "matrix.txt"
    path.write_text("".join(mat.alphabet) + "\n" + "".join(" ".join(repr(float(x)) for x in row) + "\n" for row in mat.rows))
    rows = [("ckpt", 990, 1030, "-"), ("odd", 0, 41, "+"), ("ckpt", 2565, 2600, "-"), ("empty", 0, 5, "-"), ("chrNone", 7, 9, "-"), ("odd", 38, 41, "."),
            ("ckpt", 1000, 1020, None), ("odd", 2, 60, "-")]
    bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r[:3] if r[3] is None else "%s\t%d\t%d\tx\t0\t%s\n" % r for r in rows)
    minus = [r[3] == "-" for r in rows]
    sign = ["-" if m else "+" for m in minus]
    track_of = [names.index(r[0]) if r[0] in names else -1 for r in rows]
    two2bit = os.path.join(M.GOLDEN, name)
    for flags, do_mask, mats in (([], True, [mat]), (["-u", "-r"], False, [mat, mat.reverse_complement()])):
        first, clipped = P.clipped([seqs[k] for k in names], track_of, [r[1] for r in rows], [r[2] for r in rows])
        acc, ok, offsets = PS.MODEL.planes([seqs[k] for k in names], mats, track_of, first, minus, clipped, do_mask=do_mask)
        planes = np.where(ok, acc, P.NAN)
        out = io.StringIO()
        scores_cli.main([two2bit, str(path), "-s"] + flags, stdin=io.StringIO(bed), out=out)
        lines = []
        for i, r in enumerate(rows):
            lines.append("> %s %d %d %s\n" % (r[0], r[1], r[2], sign[i]))
            for m in range(len(mats)):
                lines.append(" ".join(repr(float(x)) for x in planes[m, offsets[i]:offsets[i + 1]]) + "\n")
        assert out.getvalue() == "".join(lines), flags
        top = PC.MODEL.best_of_planes(acc, ok, offsets)
        out = io.StringIO()
        scores_cli.main([two2bit, str(path), "-s", "-b"] + flags, stdin=io.StringIO(bed), out=out)
        want = ["\t".join([r[0], str(r[1]), str(r[2]), sign[i]] + ["%s\t%d" % (repr(float(top[0][m, i])), top[1][m, i]) for m in range(len(mats))]) + "\n"
                for i, r in enumerate(rows)]
        assert out.getvalue() == "".join(want), flags
        threshold = float(np.sort(planes[0][~np.isnan(planes[0])])[-10])
        sites = []
        for i, r in enumerate(rows):
            for j in range(int(offsets[i + 1] - offsets[i])):
                for m in range(len(mats)):
                    x = planes[m, offsets[i] + j]
                    if x >= threshold:
                        at = int(PS.site_starts(first[i], clipped[i], j, mat.width, minus[i]))
                        sites.append((i, at, int(minus[i]) ^ m, "%s\t%d\t%d\t%s:%d-%d\t%s\t%s\n" % (r[0], at, at + mat.width, r[0], r[1], r[2], repr(float(x)),
                                                                                                  "+-"[int(minus[i]) ^ m])))
        sites.sort(key=lambda q: q[:3])
        out = io.StringIO()
        hits_cli.main([two2bit, str(path), repr(threshold), "-s"] + flags, stdin=io.StringIO(bed), out=out)
        assert out.getvalue() == "".join(q[3] for q in sites) and len(sites) >= 10, flags
        if "-r" in flags:
            assert any(q[3].endswith("-\n") for q in sites) and any(q[3].endswith("+\n") for q in sites)
            assert any(minus[q[0]] and q[1] != first[q[0]] for q in sites)
