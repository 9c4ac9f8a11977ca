"""
2bit sequence and base counts on the device (bxmi_twobit_*, bxmi.sequence, bx.seq.twobit.TwoBitFile, bxmi.cli.twobit_intervals_to_fasta)
against the strings recorded from the reference's bx.seq.twobit (tests/golden/twobit) and, beyond them, against
tests/twobit_model.py -- itself pinned to those recordings by tests/test_twobit_model_golden.py.  Every comparison is of bytes.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

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
