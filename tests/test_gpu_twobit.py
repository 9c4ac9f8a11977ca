"""
2bit sequence and base counts on the device (bxmi_twobit_*, bxmi.sequence, bx.seq.twobit.TwoBitFile, bxmi.cli.twobit_intervals_to_fasta)
against the strings recorded from the reference's bx.seq.twobit (tests/golden/twobit) and, beyond them, against
tests/twobit_model.py -- itself pinned to those recordings by tests/test_twobit_model_golden.py -- and, at scale, against the window
and running-count models of tests/twobit_cases.py, pinned to that one by tests/test_twobit_cases.py.  Every comparison is of bytes.
"""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import twobit_cases as K
import twobit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_bases_dev", "bxmi_twobit_composition_dev")
EINVAL = 1
WIDTHS = (1, 10, 64)  # of the matrices cut from the recorded regions
SENTINEL = 0xEE


def path_of(name):
    return os.path.join(M.GOLDEN, name)


def counts_of(text):
    return [text.upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in text)]


# ------------------------------------------------------------ every recorded case, through every layer --
@pytest.mark.parametrize("name", M.FILES)
def test_track_set_gives_the_recorded_strings(name):
    """all recorded regions of a file in ONE ragged call, as given (the device layer clips as `get`), a case the reference refuses
    as an empty row; as matrices, the first `width` letters of the regions that have them; their base counts"""
    from bxmi import sequence

    for do_mask in (True, False):
        genome = sequence.TwoBitSet.from_file(path_of(name), do_mask=do_mask)
        _, names, track_of, starts, ends, want = M.recorded_rows(name, do_mask)
        assert genome.chroms == names and [genome.sizes[n] for n in names] == [M.manifest()["files"][name]["sizes"][n] for n in names]
        chroms = [names[t] for t in track_of]
        assert genome.strings(chroms, starts, ends) == want, (name, do_mask)
        data, offsets = genome.sequences(track_of, starts, ends)  # (by position in `chroms`)
        assert data.dtype == np.uint8 and offsets.dtype == np.int64 and data.tobytes().decode() == "".join(want)
        assert np.diff(offsets).tolist() == [len(w) for w in want]
        # the rows as the reference was asked, unclipped: `get` cases only (a slice counts from the end)
        asked = [(c["seq"], c["args"], t) for c, t in M.recorded(name) if c["mask"] == do_mask and c["op"] == "get"]
        assert genome.strings([s for s, _, _ in asked], [a[0] for _, a, _ in asked], [a[1] for _, a, _ in asked]) == [t or "" for _, _, t in asked]
        for width in WIDTHS:
            rows = [i for i, w in enumerate(want) if len(w) >= width]
            got = genome.matrix([chroms[i] for i in rows], [starts[i] for i in rows], width)
            assert got.dtype == np.uint8 and got.shape == (len(rows), width)
            assert [r.tobytes().decode() for r in got] == [want[i][:width] for i in rows], (name, do_mask, width)
        assert genome.composition(chroms, starts, ends).tolist() == [counts_of(w) for w in want], (name, do_mask)
        assert genome.strings(["chrNone"], [0], [10]) == [""] and genome.composition(["chrNone"], [0], [10]).tolist() == [[0] * 6]
        genome.close()


@pytest.mark.parametrize("name", M.FILES)
def test_drop_in_answers_as_the_reference(name):
    """bx.seq.twobit.TwoBitFile: get_batch in one call; get and __getitem__ one row at a time, exception texts included"""
    from bx.seq.twobit import TwoBitFile

    cases = M.recorded(name)
    for do_mask in (True, False):
        f = open(path_of(name), "rb")  # (open for as long as the drop-in loads sequences from it, as the reference's)
        tbf = TwoBitFile(f, do_mask=do_mask)
        mine = [(c, t) for c, t in cases if c["mask"] == do_mask]
        gets = [(c, t) for c, t in mine if c["op"] == "get"]
        got = tbf.get_batch([c["seq"] for c, _ in gets] + ["chrNone"], [c["args"][0] for c, _ in gets] + [0], [c["args"][1] for c, _ in gets] + [9])
        assert got == [t or "" for _, t in gets] + [""], (name, do_mask)
        for case, text in mine:  # (per-slice calls: one device call each)
            seq = tbf[case["seq"]]
            try:
                answer = ("ok", seq.get(*case["args"]) if case["op"] == "get" else seq[slice(*case["args"])])
            except (Exception, AssertionError) as e:
                answer = ("error", [type(e).__name__, str(e)])
            assert answer == (("ok", text) if text is not None else ("error", case["error"])), case
        tbf.close()
        f.close()


def test_command_line_prints_the_recorded_strings():
    from bxmi.cli import twobit_intervals_to_fasta as cli

    name = "multi.2bit"
    for flags, do_mask in (([], True), (["-u"], False)):
        rows = [(c["seq"], c["args"][0], c["args"][1], t or "") for c, t in M.recorded(name) if c["mask"] == do_mask and c["op"] == "get" and c["args"][0] >= 0]
        bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r[:3] for r in rows) + "chrNone\t7\t9\n"
        out = io.StringIO()
        cli.main([path_of(name)] + flags, stdin=io.StringIO(bed), out=out)
        want = "".join("> %s %d %d\n" % r[:3] + "".join(r[3][c:c + 50] + "\n" for c in range(0, len(r[3]), 50)) for r in rows) + "> chrNone 7 9\n"
        assert out.getvalue() == want and any(len(r[3]) > 50 for r in rows), flags
        out = io.StringIO()
        cli.main([path_of(name), "-c"] + flags, stdin=io.StringIO(bed), out=out)
        want = "".join("\t".join([r[0], str(r[1]), str(r[2])] + [str(x) for x in counts_of(r[3])]) + "\n" for r in rows) + "chrNone\t7\t9" + "\t0" * 6 + "\n"
        assert out.getvalue() == want, flags


def test_command_line_as_a_process():
    name = "phases.2bit"
    rows = [(c["seq"], c["args"][0], c["args"][1], t) for c, t in M.recorded(name) if c["mask"] and c["op"] == "get" and t and c["args"][0] >= 0][:6]
    bed = "".join("%s\t%d\t%d\n" % r[:3] for r in rows)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bx-python_amd")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cmd = [sys.executable, "-m", "bxmi.cli.twobit_intervals_to_fasta", path_of(name)]
    got = subprocess.run(cmd, input=bed, env=env, check=True, stdout=subprocess.PIPE, universal_newlines=True, timeout=300).stdout
    assert got == "".join("> %s %d %d\n%s\n" % r for r in rows)


# ------------------------------------------------------------ structural cases against the model --
@pytest.fixture(scope="module")
def structural():
    """the four structural sequences on the device and the model of them"""
    from bxmi import sequence

    seqs = M.structural_sequences()
    tracks = [sequence.TwoBitTrack(s) for s in seqs]
    assert [(t.size, t.n_blocks, t.m_blocks) for t in tracks] == [(s.size, len(s.n_starts), len(s.m_starts)) for s in seqs]
    yield tracks, M.Letters(seqs)
    for t in tracks:
        t.close()


def ragged_call(tracks, track_of, starts, lengths, do_mask, pad):
    """bxmi_twobit_bases with the rows as they are (no clipping: positions outside the sequence are `pad`)"""
    from bxmi import _ffi as ffi

    t, s = np.array(track_of, dtype=np.int32), np.array(starts, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out = np.full(int(offsets[-1]), SENTINEL, dtype=np.uint8)
    ffi.call("bxmi_twobit_bases", ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), 0, ffi.ptr(offsets), len(out), int(do_mask), pad,
             ffi.ptr(out))
    return out


def test_ragged_structural_cases(structural):
    """rows of one base, a row across a tile boundary, a tile with a tail, whole rows and a head, empty rows between rows, a row
    wholly inside an N block, CHUNK + 5 one-base N blocks inside one segment, pad on both sides, no track, the size-0 sequence"""
    tracks, model = structural
    track_of, starts, lengths = M.ragged_case()
    assert 1 in lengths and 0 in lengths and max(lengths) > 2 * M.TILE and -1 in track_of and 2 in track_of
    for do_mask, pad in ((True, ord("N")), (False, ord(".")), (True, 0)):
        want, _ = model.bases(track_of, starts, lengths, do_mask, pad)
        assert np.array_equal(ragged_call(tracks, track_of, starts, lengths, do_mask, pad), want), (do_mask, pad)
    text = want.tobytes()
    assert b"n" in text and b"N" in text and b"a" in text and b"A" in text and b"\0" in text


@pytest.mark.parametrize("width", M.MATRIX_WIDTHS)
def test_matrix_of_every_width(structural, width):
    """widths that are no multiple of 16 among them, one wider than a tile"""
    from bxmi import sequence

    tracks, model = structural
    track_of, starts = M.matrix_case(width)
    got = sequence.matrix(tracks, track_of, starts, width, pad=b"-")
    assert np.array_equal(got, model.matrix(track_of, starts, width, True, ord("-"))), width
    assert np.array_equal(sequence.matrix(tracks, track_of, starts, width, pad=0, do_mask=False), model.matrix(track_of, starts, width, False, 0)), width


def test_composition_structural_cases(structural):
    """rows inside one checkpoint block, rows on checkpoints, the whole sequence, start == end, start > end, rows ending at a size
    that is no multiple of 4, rows clipped on both sides, rows made only of N, do_mask off; the host and the device form agree"""
    from bxmi import _ffi as ffi
    from bxmi import sequence

    tracks, model = structural
    track_of, starts, ends = M.composition_case()
    rows = [ffi.DeviceArray.from_numpy(np.array(a, dtype=np.int32)) for a in (track_of, starts, ends)]
    for do_mask in (True, False):
        want = model.composition(track_of, starts, ends, do_mask)
        got = sequence.composition(tracks, track_of, starts, ends, do_mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), do_mask
        lead = 3  # sentinels before and after the counts
        out = ffi.DeviceArray.from_numpy(np.full(lead + want.size + 5, -7, dtype=np.int32))
        ffi.call("bxmi_twobit_composition_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, rows[2].ptr, len(track_of), int(do_mask),
                 out.ptr + 4 * lead, None)
        ffi.call("bxmi_synchronize", None)
        words = out.to_numpy(np.int32)
        assert (words[:lead] == -7).all() and (words[lead + want.size:] == -7).all()
        assert np.array_equal(words[lead:lead + want.size].reshape(want.shape), want), (do_mask, "device form")
        out.free()
    whole = model.composition([0], [0], [20011], True)[0]
    assert whole.sum() - whole[5] == 20011 and (whole > 0).all()
    for r in rows:
        r.free()


@pytest.mark.parametrize("lead", (64, 1, 7))
def test_nothing_outside_the_rows_is_written(structural, lead):
    """bxmi_twobit_bases_dev with sentinel bytes on both sides of `out`, which is 16-byte aligned (lead 64: 16-byte stores) or 1
    and 7 bytes past such a boundary (byte by byte): the same bytes, the bands untouched"""
    from bxmi import _ffi as ffi

    tracks, model = structural
    track_of, starts, lengths = M.ragged_case()
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    want, _ = model.bases(track_of, starts, lengths, True, ord("N"))
    total, tail = len(want), 37
    rows = [ffi.DeviceArray.from_numpy(np.array(track_of, dtype=np.int32)), ffi.DeviceArray.from_numpy(np.array(starts, dtype=np.int32)),
            ffi.DeviceArray.from_numpy(offsets)]
    out = ffi.DeviceArray.from_numpy(np.full(lead + total + tail, SENTINEL, dtype=np.uint8))
    assert out.ptr % 16 == 0
    ffi.call("bxmi_twobit_bases_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, len(track_of), 0, rows[2].ptr, total, 1, ord("N"),
             out.ptr + lead, None)
    ffi.call("bxmi_synchronize", None)
    data = out.to_numpy(np.uint8)
    assert (data[:lead] == SENTINEL).all() and (data[lead + total:] == SENTINEL).all()
    assert np.array_equal(data[lead:lead + total], want), lead
    for a in rows + [out]:
        a.free()


def test_no_rows_and_bad_arguments(structural):
    from bxmi import _ffi as ffi
    from bxmi import sequence

    tracks, _ = structural
    data, offsets = sequence.sequences(tracks, [], [], [])
    assert len(data) == 0 and offsets.tolist() == [0]
    assert sequence.matrix(tracks, [], [], 5).shape == (0, 5) and sequence.composition(tracks, [], [], []).shape == (0, 6)
    assert sequence.strings(tracks, [0, 2, 0], [5, 0, 9], [5, 0, 3]) == ["", "", ""]
    for call in (lambda: sequence.matrix(tracks, [0], [0], 0), lambda: sequence.matrix(tracks, [len(tracks)], [0], 4),
                 lambda: sequence.composition(tracks, [len(tracks)], [0], [4]), lambda: sequence.matrix(tracks, [0], [0], 4, pad=300),
                 lambda: sequence.sequences(tracks, [0, len(tracks)], [0, 0], [4, 4]), lambda: sequence.strings(tracks, [len(tracks) + 7], [0], [4])):
        with pytest.raises(ffi.BxmiError) as e:
            call()
        assert e.value.code == EINVAL
    # a file whose blocks overlap is refused, naming the condition
    seq = M.structural_sequences()[1]
    with pytest.raises(ffi.BxmiError, match="not sorted and disjoint"):
        sequence.TwoBitTrack.from_arrays(seq.packed, seq.size, [3, 5], [4, 2])
    with pytest.raises(ValueError):
        sequence.matrix(tracks, [0], [0], 4, pad=b"NN")


# ------------------------------------------------------------ seeded cases and scale, host forms and _dev forms --
# Two limits of csrc/sequence.hip are deliberately not reached: TB_ROWS_PER_LAUNCH (2^25 rows per launch of the base counts: 768 MiB
# of counts and as much model) and TB_TILES_PER_LAUNCH (2^22 tiles: 16 GiB of letters).  Neither can be had in seconds.
def bases_host(tracks, track_of, starts, do_mask, pad, width=0, lengths=None):
    """bxmi_twobit_bases as it stands (no clipping), `out` filled with the sentinel first -> uint8[total]"""
    from bxmi import _ffi as ffi

    t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
    offsets = None if lengths is None else np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    out = np.full(len(t) * width if offsets is None else int(offsets[-1]), SENTINEL, dtype=np.uint8)
    ffi.call("bxmi_twobit_bases", ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), width, ffi.ptr(offsets), len(out), int(do_mask), pad,
             ffi.ptr(out))
    return out


def bases_dev(tracks, track_of, starts, do_mask, pad, width=0, lengths=None, lead=64, tail=37):
    """bxmi_twobit_bases_dev on arrays in device memory, on the null stream, `out` `lead` bytes into an allocation of sentinel
    bytes, which must still be there on both sides afterwards -> uint8[total]"""
    from bxmi import _ffi as ffi

    offsets = None if lengths is None else np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = len(track_of) * width if offsets is None else int(offsets[-1])
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts)]
    rows += [ffi.DeviceArray.from_numpy(offsets)] if offsets is not None else []
    out = ffi.DeviceArray.from_numpy(np.full(lead + total + tail, SENTINEL, dtype=np.uint8))
    assert out.ptr % 16 == 0
    ffi.call("bxmi_twobit_bases_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, len(track_of), width,
             rows[2].ptr if offsets is not None else None, total, int(do_mask), pad, out.ptr + lead, None)
    ffi.call("bxmi_synchronize", None)
    data = out.to_numpy(np.uint8)
    for a in rows + [out]:
        a.free()
    assert (data[:lead] == SENTINEL).all() and (data[lead + total:] == SENTINEL).all(), "written outside the output"
    return data[lead:lead + total]


def counts_host(tracks, track_of, starts, ends, do_mask):
    from bxmi import sequence

    got = sequence.composition(tracks, track_of, starts, ends, do_mask)
    assert got.dtype == np.int32 and got.shape == (len(track_of), 6)
    return got


def counts_dev(tracks, track_of, starts, ends, do_mask, lead=3, tail=5):
    """bxmi_twobit_composition_dev, sentinels before and after the counts -> int32 [n, 6]"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts, ends)]
    out = ffi.DeviceArray.from_numpy(np.full(lead + 6 * n + tail, -7, dtype=np.int32))
    ffi.call("bxmi_twobit_composition_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, rows[2].ptr, n, int(do_mask), out.ptr + 4 * lead, None)
    ffi.call("bxmi_synchronize", None)
    words = out.to_numpy(np.int32)
    for a in rows + [out]:
        a.free()
    assert (words[:lead] == -7).all() and (words[lead + 6 * n:] == -7).all(), "written outside the counts"
    return words[lead:lead + 6 * n].reshape(n, 6)


def through_device(tracks):
    """the `bases` and `counts` of twobit_cases.check_random_case: the host form's answer, which the _dev form's must equal (the
    letters with `out` 16-byte aligned and one byte past that)"""

    def bases(_seqs, track_of, starts, do_mask, pad, width=0, lengths=None):
        got = bases_host(tracks, track_of, starts, do_mask, pad, width, lengths)
        for lead in (64, 1):
            assert np.array_equal(bases_dev(tracks, track_of, starts, do_mask, pad, width, lengths, lead=lead), got), ("device form", lead)
        return got

    def counts(_seqs, track_of, starts, ends, do_mask):
        got = counts_host(tracks, track_of, starts, ends, do_mask)
        assert np.array_equal(counts_dev(tracks, track_of, starts, ends, do_mask), got), "device form"
        return got

    return bases, counts


@contextlib.contextmanager
def on_device(seqs):
    """the sequences as tracks on the device, closed again whatever the test does with them"""
    from bxmi import sequence

    tracks = []
    try:
        for s in seqs:
            tracks.append(sequence.TwoBitTrack(s))
        yield tracks
    finally:
        for t in tracks:
            t.close()


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_random_sequences(seed):
    """tests/test_twobit_kernel_host.py::test_random_sequences on the device: the same sequences, rows and comparisons"""
    with on_device(K.random_case(seed)["seqs"]) as tracks:
        K.check_random_case(seed, *through_device(tracks))


def test_many_chunks_and_sixteen_blocks_in_a_thread():
    """tests/test_twobit_kernel_host.py's test of that name on the device"""
    with on_device(K.many_blocks_case()["seqs"]) as tracks:
        K.check_many_blocks_case(*through_device(tracks))


@pytest.fixture(scope="module")
def big_tracks():
    """the two sequences of twobit_cases.big_sequence on the device, each made when first asked for"""
    from bxmi import sequence

    made = {}

    def get(which):
        if which not in made:
            made[which] = sequence.TwoBitTrack(K.big_sequence(which))
        return made[which]

    yield get
    for t in made.values():
        t.close()


@pytest.mark.parametrize("which", (0, 1))
def test_tables_beyond_one_scan_tile(big_tracks, which):
    """10 241 and 6 143 checkpoints, 7 000 N blocks: every plane of both running tables is scanned in several tiles of the device
    scan, the planes 16-byte aligned (stride 6 144) or not (10 242; 7 001).  40 000 random rows and rows cut around the tiles'
    edges against the running-count model, every 500th row counted from its own letters; 2 000 windows and 100 ragged rows
    against the letters of their windows.  (The row counts are what the time allows: the letters of 10 M bases and their six
    running counts cost what they cost, whatever the rows.)"""
    seq, facts = K.big_conditions(which)
    assert facts["stride"] == (10242, 6144)[which] and facts["stride"] % 4 == (2, 0)[which] and (len(seq.n_starts) + 1) % 2 == 1
    assert facts["rows over N block 2048"] > 100 and facts["rows over checkpoint 2048"] > 100
    track = big_tracks(which)
    assert (track.size, track.n_blocks, track.m_blocks) == (seq.size, K.BIG_N_BLOCKS, K.BIG_M_BLOCKS)
    whole = K.big_letters(which)
    starts, ends = K.big_composition_rows(which)
    zeros = np.zeros(len(starts), dtype=np.int32)
    want = K.big_composition_want(which)
    for i in range(0, len(starts), 500):
        s, e = max(int(starts[i]), 0), min(int(ends[i]), seq.size)
        assert want[i].tolist() == K.counts_of_letters(whole[s:e]), i
    assert (want > 0).any(axis=0).all() and int(want[:, :5].sum(axis=1).max()) == seq.size
    got = counts_host([track], zeros, starts, ends, True)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), [(int(starts[i]), int(ends[i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    assert np.array_equal(counts_dev([track], zeros, starts, ends, True), want)
    unmasked = want[::7].copy()
    unmasked[:, 5] = 0  # (without do_mask the letters are these in upper case)
    assert np.array_equal(counts_host([track], zeros[::7], starts[::7], ends[::7], False), unmasked)
    # letters
    rng = np.random.default_rng(340 + which)
    n, width = 2000, 100
    at = rng.integers(-50, seq.size - 49, n)
    at[:4] = (-50, -1, seq.size - 99, seq.size - 50)
    want = np.stack([K.window_row([seq], 0, int(a), width, True, ord("-")) for a in at])
    got = bases_host([track], zeros[:n], at, True, ord("-"), width=width)
    assert np.array_equal(got.reshape(n, width), want)
    assert np.array_equal(bases_dev([track], zeros[:n], at, True, ord("-"), width=width).reshape(n, width), want)
    lengths = K.log_uniform(rng, 1, 3 * M.TILE + 1, 100) - 1
    at = rng.integers(-50, seq.size - 49, 100)
    at[:2], lengths[:2] = (seq.size - 3 * M.TILE + 9, 17), (3 * M.TILE, 3 * M.TILE)
    for do_mask in (True, False):
        want = K.window_bases([seq], zeros[:100], at, lengths, do_mask, ord("."))
        assert np.array_equal(bases_host([track], zeros[:100], at, do_mask, ord("."), lengths=lengths), want), do_mask
        assert np.array_equal(bases_dev([track], zeros[:100], at, do_mask, ord("."), lengths=lengths, lead=7), want), do_mask


def test_host_forms_go_through_more_than_one_slab(big_tracks):
    """bxmi_twobit_bases in slabs of 2^26 output bytes -- 17 rows of 2^22 + 3 bases, then ragged rows of 0 to 2^23 + 9, a slab
    ending inside a row both times -- and bxmi_twobit_composition in slabs of 2^22 rows; the letters wanted are slices of the
    whole sequence's"""
    from bxmi import sequence

    seq, track, whole = K.big_sequence(0), big_tracks(0), K.big_letters(0)
    width, n = (1 << 22) + 3, 17
    assert n * width > K.TB_SLAB and K.TB_SLAB % width != 0
    starts = np.arange(n, dtype=np.int32) * 37 - 5
    want = np.full((n, width), ord("-"), dtype=np.uint8)
    for i, s in enumerate(starts.tolist()):
        want[i, max(-s, 0):] = whole[max(s, 0):s + width]
    got = sequence.matrix([track], np.zeros(n, dtype=np.int32), starts, width, pad=b"-")
    assert got.shape == want.shape and np.array_equal(got, want)
    big = 1 << 23
    lengths = np.array([5, big + 1, 0, 1, big - 7, 3, big + 2, 0, big, 1000, big + 9, 2, big - 1, big + 5, big, 77, big + 3, 4, big - 2, 999], dtype=np.int64)
    assert lengths.sum() > K.TB_SLAB + (1 << 22) and K.TB_SLAB not in np.cumsum(lengths)
    starts = (np.arange(len(lengths), dtype=np.int32) * 53) % 1100 - 5
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    want = np.full(int(offsets[-1]), ord("."), dtype=np.uint8)
    for i, (s, m) in enumerate(zip(starts.tolist(), lengths.tolist())):
        want[offsets[i] + max(-s, 0):offsets[i + 1]] = whole[max(s, 0):s + m] & ~np.uint8(0x20)
    got = bases_host([track], np.zeros(len(lengths), dtype=np.int32), starts, False, ord("."), lengths=lengths)
    assert np.array_equal(got, want)
    del got, want
    # base counts: 2^22 + 1001 rows drawn from those of test_tables_beyond_one_scan_tile, whose counts the model has (the running
    # counts of 10 M letters are made once); the rows on both sides of the slab's edge have three different, known answers
    n = K.TB_COMP_SLAB + 1001
    pool_starts, pool_ends = K.big_composition_rows(0)
    idx = np.random.default_rng(350).integers(0, len(pool_starts), n)
    edge = K.TB_COMP_SLAB
    idx[edge - 1:edge + 2] = (len(pool_starts) - 3, len(pool_starts) - 2, len(pool_starts) - 1)
    starts, ends, want = pool_starts[idx], pool_ends[idx], K.big_composition_want(0)[idx]
    assert len(np.unique(idx)) > len(pool_starts) // 2
    # (0, size), (size - 3, size + 100) and (0, the end of N block 2048): three different answers, each counted from its letters
    cut = int(seq.n_starts[2048] + seq.n_sizes[2048])
    known = [K.counts_of_letters(whole), K.counts_of_letters(whole[seq.size - 3:]), K.counts_of_letters(whole[:cut])]
    assert list(zip(starts[edge - 1:edge + 2].tolist(), ends[edge - 1:edge + 2].tolist())) == [(0, seq.size), (seq.size - 3, seq.size + 100), (0, cut)]
    assert want[edge - 1:edge + 2].tolist() == known and len({tuple(k) for k in known}) == 3 and all(sum(k) > 0 for k in known) and (want[edge - 1] > 0).all()
    got = counts_host([track], np.zeros(n, dtype=np.int32), starts, ends, True)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_sequence_at_the_top_of_int32():
    """2^31 - 1 bases (twobit_cases.TopSequence): positions, running sizes and running counts next to the top of int32 -- the T
    count of the whole sequence is beyond 2^30, its masked count 14 000 below 2^31 -- in rows at the sequence's end, across it,
    and across the edges of an N block of 2^28 bases and of a mask block of nearly everything"""
    top = K.top_sequence()
    with on_device([top.seq]) as tracks:  # (512 MiB of device memory: given back whatever happens)
        check_top_sequence(top, tracks[0])


def check_top_sequence(top, track):
    from bxmi import sequence

    size, half = top.size, 1 << 30
    assert (track.size, track.n_blocks, track.m_blocks) == (size, len(top.seq.n_starts), len(top.seq.m_starts)) and size == 2 ** 31 - 1
    # letters: windows of 100 (the pad belongs to the matrix form) and of TILE + 1
    at = [size - 100, size - 1, size, size - 50, size - 99, K.TOP_N[0] - 50, K.TOP_N[1] - 50, K.TOP_N[0] - 100, K.TOP_N[1], K.TOP_MASK[0] - 50, K.TOP_MASK[1] - 50,
          half - 2048 - 50, half - 50, half + 2048 - 50, size - 8192 - 50, size - 4097 - 40, -50, 4096 - 50, 0]
    zeros = np.zeros(len(at), dtype=np.int32)
    for width in (100, M.TILE + 1):
        starts = [a - (width - 100) // 2 for a in at[3:]] + at[:3]
        for do_mask in (True, False):
            want = np.stack([top.row(s, width, do_mask, ord("-")) for s in starts])
            if width == 100:  # the last three rows: up to the size, its last base and pad, pad only
                assert not (want[-3] == ord("-")).any() and want[-2, 0] != ord("-") and (want[-2, 1:] == ord("-")).all() and (want[-1] == ord("-")).all()
            got = bases_host([track], zeros, starts, do_mask, ord("-"), width=width).reshape(len(at), width)
            assert np.array_equal(got, want), (width, do_mask, [starts[i] for i in np.flatnonzero((got != want).any(axis=1))])
            assert np.array_equal(bases_dev([track], zeros, starts, do_mask, ord("-"), width=width).reshape(len(at), width), want), (width, do_mask)
    # the clipped regions of the Python layer: rows that end at the size, the last base, nothing
    starts, ends = [size - 3000, size - 1, size, half - 10, -5, K.TOP_MASK[1] - 7], [size, size, size, half + 10, 12, K.TOP_MASK[1] + 7]
    data, offsets = sequence.sequences([track], [0] * len(starts), starts, ends)
    assert np.diff(offsets).tolist() == [3000, 1, 0, 20, 12, 14]
    assert np.array_equal(data, np.concatenate([top.letters(max(s, 0), e) for s, e in zip(starts, ends)]))
    # base counts
    starts = [0, 1, K.TOP_N[0] - 3, half - 10, half - 3000, half, half - 1, size - 1, size - 1, size, size - 8192, 0, K.TOP_MASK[0] - 1, -7]
    ends = [size, size - 1, K.TOP_N[1] + 3, half + 10, half + 3000, half + 1, half, size, size, size, size, half, K.TOP_MASK[1] + 1, size]
    for do_mask in (True, False):
        want = top.composition(starts, ends, do_mask)
        assert want[0, 3] > half and want[0, :5].sum() == size and (want[0, 5] > 2 ** 31 - 20000) == do_mask and want.max() < 2 ** 31
        assert want[7].sum() == 1 + do_mask and want[9].sum() == 0 and want[2].tolist()[:5] == [0, 0, 0, 6, 1 << 28]
        got = counts_host([track], [0] * len(starts), starts, ends, do_mask)
        assert np.array_equal(got, want), (do_mask, got.tolist(), want.tolist())
        assert np.array_equal(counts_dev([track], [0] * len(starts), starts, ends, do_mask), want), (do_mask, "device form")


# ------------------------------------------------------------ device entry points on torch tensors --
def test_dev_forms_on_torch_tensors():
    """matrix_dev / sequences_dev / composition_dev on torch tensors -- input slices that start 4 bytes into their allocation,
    torch's current stream and a stream of the caller's, matrix_dev into a tensor sliced one byte off a 16-byte boundary with
    sentinels before and after it, rows the device form cannot refuse, an empty batch -- in a process of its own: torch brings its
    own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import twobit_model as M
from bxmi import sequence

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

seqs = M.structural_sequences()
model = M.Letters(seqs)
dev = [sequence.TwoBitTrack(s) for s in seqs]
side = torch.cuda.Stream()

track_of, starts, ends = M.composition_case()
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
assert all(x.data_ptr() % 16 for x in d)
for do_mask in (True, False):
    want = model.composition(track_of, starts, ends, do_mask)
    got = sequence.composition_dev(dev, *d, do_mask=do_mask)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), do_mask
    with torch.cuda.stream(side):
        got = sequence.composition_dev(dev, *d, do_mask=do_mask)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want), (do_mask, "side stream")
    # the rows as letters: clipped as `get` clips them
    lengths = [max(min(e, seqs[t].size if t >= 0 else 0) - max(s, 0), 0) for t, s, e in zip(track_of, starts, ends)]
    want_bytes, want_offsets = model.bases(track_of, [max(s, 0) for s in starts], lengths, do_mask)
    data, offsets = sequence.sequences_dev(dev, *d, do_mask=do_mask)
    torch.cuda.synchronize()
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and np.array_equal(offsets.cpu().numpy(), want_offsets)
    assert np.array_equal(data.cpu().numpy(), want_bytes), do_mask
    # on a stream that is not torch's current one: the tensors the call makes for itself outlive it on that stream
    data, offsets = sequence.sequences_dev(dev, *d, do_mask=do_mask, stream=side.cuda_stream)
    churn = [torch.zeros(len(track_of), dtype=torch.int32, device="cuda") for _ in range(4)]  # (what could take a freed block)
    side.synchronize()
    assert np.array_equal(offsets.cpu().numpy(), want_offsets) and np.array_equal(data.cpu().numpy(), want_bytes), (do_mask, "side stream")

for width in (37, M.TILE + 1):
    track_of_m, starts_m = M.matrix_case(width)
    want_m = model.matrix(track_of_m, starts_m, width, True, ord("-"))
    rows = [dev_i32(track_of_m, 1), dev_i32(starts_m, 2)]
    got = sequence.matrix_dev(dev, *rows, width, pad=b"-")
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want_m), width
    n = len(track_of_m)
    for lead in (1, 16):  # one byte off a 16-byte boundary; on one
        whole = torch.full((lead + n * width + 5,), 0xEE, dtype=torch.uint8, device="cuda")
        out = whole[lead:lead + n * width].view(n, width)
        assert (out.data_ptr() % 16 != 0) == (lead != 16)
        torch.cuda.synchronize()
        res = sequence.matrix_dev(dev, *rows, width, pad=b"-", stream=side.cuda_stream, out=out)
        side.synchronize()
        assert res is out and np.array_equal(out.cpu().numpy(), want_m), (width, lead)
        edge = whole.cpu().numpy()
        assert (edge[:lead] == 0xEE).all() and (edge[lead + n * width:] == 0xEE).all()

# entries the device form cannot refuse are rows of pad / of zeros: a track index beyond the list
odd_t, odd_s = dev_i32(np.array([len(dev), 1, -3]), 0), dev_i32(np.array([3, 3, 3]), 0)
odd = sequence.matrix_dev(dev, odd_t, odd_s, 6, pad=b"#", stream=side.cuda_stream)
side.synchronize()
assert [r.tobytes() for r in odd.cpu().numpy()] == [b"######", model.row(1, 3, 6).tobytes(), b"######"]
zero = sequence.composition_dev(dev, odd_t, odd_s, dev_i32(np.array([9, 9, 9]), 0)).cpu().numpy()
assert zero[0].tolist() == [0] * 6 and zero[2].tolist() == [0] * 6 and zero[1].sum() > 0
data, offsets = sequence.sequences_dev(dev, d[0][:0], d[1][:0], d[2][:0], stream=side.cuda_stream)
assert tuple(data.shape) == (0,) and offsets.tolist() == [0]
assert tuple(sequence.matrix_dev(dev, d[0][:0], d[1][:0], 5).shape) == (0, 5)
assert tuple(sequence.composition_dev(dev, d[0][:0], d[1][:0], d[2][:0]).shape) == (0, 6)
for t in dev:
    t.close()
print("twobit dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "twobit dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
