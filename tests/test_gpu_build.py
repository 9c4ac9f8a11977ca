"""
2bit tracks built on the device from letters (bxmi_twobit_create_letters, bxmi_twobit_create_letters_dev, bxmi_twobit_create_nib,
bxmi_twobit_arrays; TwoBitTrack.from_letters / from_letters_dev / from_nib / arrays, TwoBitSet.from_fasta / from_nib / open, the
bx.seq.fasta and bx.seq.nib drop-ins, the command lines) against tests/build_model.py -- pinned to the reference's own FASTA / 2bit
pairs by tests/test_build_model_golden.py -- on the seeded cases of tests/build_cases.py, which tests/test_build_kernel_host.py runs
through the kernels' text on the host, and against the answers recorded from the reference's FastaFile.get and NibFile.get
(tests/golden/seqfile).  Integer work: every comparison is exact.
"""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as BC
import build_model as B
import twobit_cases as TC
import twobit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQFILE = os.path.join(ROOT, "tests", "golden", "seqfile")
# the _dev entry point this file drives by its C name (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_create_letters_dev",)


def arrays_equal(track, built, key):
    got = track.arrays()
    assert (track.size, track.n_blocks, track.m_blocks) == (built.seq.size, len(built.seq.n_starts), len(built.seq.m_starts)), key
    assert B.same_arrays(got, built.seq) and len(got.packed) == len(built.seq.packed), key
    return got


class DeviceLetters:
    """the letters in device memory, `misalign` bytes past an aligned address; freed on leaving"""

    def __init__(self, a, misalign=0):
        from bxmi import _ffi

        room = np.full(len(a) + misalign + 16, 0x5A, dtype=np.uint8)
        room[misalign:misalign + len(a)] = a
        self.held = _ffi.DeviceArray.from_numpy(room)
        self.ptr, self.size = self.held.ptr + misalign, len(a)
        assert self.ptr % 16 == misalign % 16

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.held.free()

    def create(self, other):
        """bxmi_twobit_create_letters_dev by its C name, on the null stream -> (rc, the handle)"""
        from bxmi import _ffi

        h = C.c_void_p(12345)
        return _ffi.load().bxmi_twobit_create_letters_dev(self.ptr, self.size, other, C.byref(h), None), h

    def track(self, other="N"):
        from bxmi import sequence

        return sequence.TwoBitTrack._built("bxmi_twobit_create_letters_dev", self.ptr, self.size, sequence._other(other), stream=(None,))


@pytest.fixture(scope="module")
def letter_cases():
    return [(name, a, B.from_letters(a)) for name, a in BC.letter_cases() + BC.other_cases()]


# ------------------------------------------------------------ 1. every case through all three entry points --
def test_host_letters_equal_the_model(letter_cases):
    from bxmi import sequence

    for name, a, built in letter_cases:
        track = sequence.TwoBitTrack.from_letters(a, other="N")
        arrays_equal(track, built, name)
        track.close()
    track = sequence.TwoBitTrack.from_letters("ACGTNnacgt")
    assert M.letters(track.arrays()).tobytes() == b"ACGTNnacgt" and sequence.TwoBitTrack.from_letters(b"ACGTNnacgt").arrays().m_starts.tolist() == [5]


def test_device_letters_equal_the_model_at_any_alignment(letter_cases):
    from bxmi import _ffi

    for name, a, built in letter_cases:
        for misalign in ((0, 1, 8, 15) if name in ("size_17", "size_%d" % (BC.T + 1), "random_411", "several_tiles") else (0,)):
            with DeviceLetters(a, misalign) as letters:
                track = letters.track()
                first = arrays_equal(track, built, (name, misalign))
                again = letters.track()  # the same on every run
                assert B.same_arrays(again.arrays(), first), name
                track.close(), again.close()
    with DeviceLetters(np.frombuffer(b"ACnnGT", dtype=np.uint8)) as letters:
        rc, h = letters.create(0)
        assert rc == _ffi.OK and h.value
        n, m = C.c_int64(), C.c_int64()
        _ffi.call("bxmi_twobit_info", h, None, C.byref(n), C.byref(m))
        assert (n.value, m.value) == (1, 1)
        _ffi.call("bxmi_twobit_destroy", h)


def test_nibbles_equal_the_model():
    from bxmi import sequence

    for name, data, size in BC.nib_cases() + BC.nib_other_cases():
        track = sequence.TwoBitTrack.from_nib(data, size, other="N")
        arrays_equal(track, B.from_nib(data, size), name)
        track.close()


def test_arrays_of_a_file_track_are_its_inputs():
    from bxmi import sequence, twobit

    for name, seq in twobit.read_file(os.path.join(M.GOLDEN, "multi.2bit")).items():
        track = sequence.TwoBitTrack(seq)
        assert B.same_arrays(track.arrays(), seq), name
        track.close()


def test_empty_track():
    from bxmi import sequence

    with DeviceLetters(np.zeros(0, np.uint8)) as letters:
        tracks = (sequence.TwoBitTrack.from_letters(b""), sequence.TwoBitTrack.from_nib(b"", 0), letters.track())
    for track in tracks:
        assert (track.size, track.n_blocks, track.m_blocks) == (0, 0, 0)
        assert sequence.strings([track], [0], [0], [10]) == [""] and not sequence.composition([track], [0], [0], [10]).any()
        track.close()


# ------------------------------------------------------------ 2. every sequence call gives the same on a built track --
def test_round_trip_against_tracks_from_the_arrays(letter_cases):
    from bxmi import kmers, sequence

    rng = np.random.default_rng(440)
    picked = [c for c in letter_cases if c[0] in ("size_%d" % (2 * BC.T + 1), "random_412", "every_second_n", "n_inside_lower_case", "three_tiles_N", "iupac",
                                                  "ends_and_single_mask", "size_5")]
    assert len(picked) == 8
    for name, a, built in picked:
        size = len(a)
        mine, theirs = sequence.TwoBitTrack.from_letters(a, other="N"), sequence.TwoBitTrack(built.seq)
        starts = np.concatenate([[0, -3, size - 1, 0], rng.integers(0, size, size=40)]).astype(np.int32)
        ends = np.concatenate([[size, 5, size + 4, 0], starts[4:] + rng.integers(0, 300, size=40)]).astype(np.int32)
        strands = (np.arange(len(starts)) % 2).astype(np.int8)
        rows = [0] * len(starts)
        for do_mask in (True, False):
            for s in (None, strands):
                got, want = sequence.sequences([mine], rows, starts, ends, do_mask, s), sequence.sequences([theirs], rows, starts, ends, do_mask, s)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, do_mask)
                assert np.array_equal(sequence.composition([mine], rows, starts, ends, do_mask, s), sequence.composition([theirs], rows, starts, ends, do_mask, s)), name
        whole = sequence.sequences([mine], [0], [0], [size])[0]  # and the letters themselves come back, an other symbol as N / n
        want = np.where(B._OTHER[a], np.where(B._LOWER[a], ord("n"), ord("N")), a)
        assert np.array_equal(whole, want), name
        k = (kmers.counts([mine], rows, starts, ends, 3, strands=strands), kmers.counts([theirs], rows, starts, ends, 3, strands=strands))
        assert np.array_equal(k[0], k[1]) and k[0].shape == (len(starts), 64), name
        mine.close(), theirs.close()


# ------------------------------------------------------------ 4. the recordings: drop-ins, get_batch, the command lines --
def manifest():
    with open(os.path.join(SEQFILE, "manifest.json")) as f:
        return json.load(f)["files"]


def open_recorded(name, contig, revcomp):
    import bx.seq.fasta
    import bx.seq.nib

    if name.endswith(".nib"):
        return bx.seq.nib.NibFile(open(os.path.join(SEQFILE, name), "rb"), revcomp)
    return bx.seq.fasta.FastaFile(open(os.path.join(SEQFILE, name)), revcomp, contig=contig)


def test_recorded_gets_through_the_drop_ins():
    checked = 0
    files = manifest()
    assert sorted(files) == sorted(["test.fa", "test2.fa", "testN.fa", "testMask.fa", "test.nib", "edges_be.nib", "random_be.nib"])
    for name, entry in files.items():
        strings = np.load(os.path.join(SEQFILE, entry["strings"])).tobytes().decode("ascii")
        lengths = {contig: (record_name, length) for contig, record_name, length in entry["records"]}
        groups = {}
        for contig, revcomp, start, length, first, past in entry["entries"]:
            groups.setdefault((contig, revcomp), []).append((start, length, strings[first:past]))
        assert {r for _, r in groups} == {False, "-5'", "-3'"}
        for (contig, revcomp), rows in groups.items():
            seq = open_recorded(name, contig, revcomp)
            assert seq.length == lengths[contig][1] and (name.endswith(".nib") or seq.name == lengths[contig][0])
            got = seq.get_batch([r[0] for r in rows], [r[1] for r in rows])  # ONE device call
            assert got == [r[2] for r in rows], (name, contig, revcomp)
            assert seq.get(*rows[3][:2]) == rows[3][2] and seq.get(0, 0) == ""
            if not name.endswith(".nib"):
                assert seq.text[:10] == seq.raw_fetch(0, 10)
            checked += len(rows)
            seq.close()
    assert checked == sum(len(e["entries"]) for e in files.values()) > 700


def test_sets_from_fasta_nib_and_open():
    from bxmi import sequence

    want = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, "testMask.2bit"))
    for got in (sequence.TwoBitSet.from_fasta(os.path.join(M.GOLDEN, "testMask.fa")), sequence.TwoBitSet.open(os.path.join(M.GOLDEN, "testMask.fa")),
                sequence.TwoBitSet.open(os.path.join(M.GOLDEN, "testMask.2bit"))):
        assert got.chroms == want.chroms and got.sizes == want.sizes
        for name in want.chroms:
            assert B.same_arrays(got.tracks[name].arrays(), want.tracks[name].arrays()), name
        got.close()
    want.close()
    nibs = sequence.TwoBitSet.open(SEQFILE)  # a directory of nib files
    assert nibs.chroms == ["edges_be", "random_be", "test"] and nibs.sizes["test"] == 379
    one = sequence.TwoBitSet.open(os.path.join(SEQFILE, "test.nib"))
    mule = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, "test.2bit"))
    assert one.chroms == ["test"] and one.strings(["test"], [0], [379]) == nibs.strings(["test"], [0], [379]) == mule.strings(["mule"], [0], [379])
    nibs.close(), one.close(), mule.close()


def test_twobit_command_lines_take_a_fasta_file(tmp_path):
    """the four twobit_* tools print for test.fa what they print for test.2bit"""
    from bxmi.cli import twobit_intervals_to_fasta, twobit_kmer_counts, twobit_pwm_hits, twobit_pwm_scores

    bed = "# regions\n" + "".join("mule\t%d\t%d\tr\t0\t%s\n" % r for r in ((0, 379, "+"), (100, 160, "-"), (370, 400, "+"), (5, 5, "+"))) + "horse\t1\t9\tr\t0\t+\n"
    matrix = tmp_path / "matrix.txt"
    matrix.write_text("ACGT\n1.0 -1.0 0.5 -0.5\n-2.0 1.5 0.25 0.0\n0.5 0.5 -1.0 1.0\n")
    runs = ((twobit_intervals_to_fasta, []), (twobit_intervals_to_fasta, ["-c", "-s"]), (twobit_intervals_to_fasta, ["-u", "-s"]),
            (twobit_kmer_counts, ["2", "-i"]), (twobit_pwm_scores, [str(matrix), "-s"]), (twobit_pwm_hits, [str(matrix), "1.0", "-r"]))
    for cli, args in runs:
        printed = []
        for path in (os.path.join(M.GOLDEN, "test.2bit"), os.path.join(M.GOLDEN, "test.fa")):
            out = io.StringIO()
            cli.main([path] + args, stdin=io.StringIO(bed), out=out)
            printed.append(out.getvalue())
        assert printed[0] == printed[1] and len(printed[0]) > 100, (cli.__name__, args)


def wrapped(text):
    return "".join(text[c:c + 50] + "\n" for c in range(0, len(text), 50))


def test_nib_command_lines(tmp_path):
    from bxmi import fasta
    from bxmi.cli import nib_chrom_intervals_to_fasta, nib_intervals_to_fasta

    mule = fasta.read_file(os.path.join(SEQFILE, "test.fa"))["mule"].tobytes().decode()
    ranges = ((0, 379), (100, 151), (7, 7), (378, 379), (33, 150))
    range_file = tmp_path / "ranges.txt"
    range_file.write_text("".join("%d %d\n" % r for r in ranges))
    out = io.StringIO()
    nib_intervals_to_fasta.main([str(range_file), os.path.join(SEQFILE, "test.nib")], out=out)
    assert out.getvalue() == "".join("> %d %d\n" % r + wrapped(mule[r[0]:r[1]]) for r in ranges)
    out = io.StringIO()
    rows = [("test", 5, 70), ("edges_be", 0, 75), ("test", 300, 379), ("random_be", 1, 2)]
    nib_chrom_intervals_to_fasta.main([SEQFILE], stdin=io.StringIO("".join("%s %d %d\n" % r for r in rows)), out=out)
    files = manifest()
    whole = {}
    for name in ("edges_be", "random_be"):
        strings = np.load(os.path.join(SEQFILE, name + ".nib.strings.npy")).tobytes().decode()
        whole[name] = next(strings[e[4]:e[5]] for e in files[name + ".nib"]["entries"] if e[1] is False and e[2] == 0 and e[3] == files[name + ".nib"]["records"][0][2])
    whole["test"] = mule
    assert out.getvalue() == "".join("> %s %d %d\n" % r + wrapped(whole[r[0]][r[1]:r[2]]) for r in rows)
    # a range outside the sequence: the reference's AssertionError for the first such line, before any output
    range_file.write_text("0 10\n370 380\n5 2\n")
    out = io.StringIO()
    with pytest.raises(AssertionError, match=r"Interval beyond end of sequence \(370\.\.380 > 379\)"):
        nib_intervals_to_fasta.main([str(range_file), os.path.join(SEQFILE, "test.nib")], out=out)
    assert out.getvalue() == ""


# ------------------------------------------------------------ 5. refusals --
def test_other_symbols_are_refused_by_position():
    from bxmi import _ffi, sequence

    lib = _ffi.load()
    for name, a in BC.other_cases():
        built = B.from_letters(a)
        word = "position %d holds byte 0x%02X" % (built.first_other, built.other_value)
        with pytest.raises(_ffi.BxmiError) as err:
            sequence.TwoBitTrack.from_letters(a)
        assert err.value.code == _ffi.EINVAL and word in str(err.value), (name, str(err.value))
        for misalign in (0, 3):
            with DeviceLetters(a, misalign) as letters:
                rc, h = letters.create(0)
            assert rc == _ffi.EINVAL and h.value is None and word.encode() in lib.bxmi_last_error(), name  # the code, the position, no handle
        h = C.c_void_p(12345)
        assert lib.bxmi_twobit_create_letters(_ffi.ptr(a), len(a), 0, C.byref(h)) == _ffi.EINVAL and h.value is None
    for name, data, size in BC.nib_other_cases():
        built = B.from_nib(data, size)
        h = C.c_void_p(12345)
        assert lib.bxmi_twobit_create_nib(_ffi.ptr(data), size, 0, C.byref(h)) == _ffi.EINVAL and h.value is None
        assert b"position %d holds nibble 0x%X (code %d)" % (built.first_other, built.other_value, built.other_value & 7) in lib.bxmi_last_error(), name
    # the pad nibble behind an odd size is no symbol
    track = sequence.TwoBitTrack.from_nib(np.array([0x01, 0x2F], dtype=np.uint8), 3)
    assert M.letters(track.arrays()).tobytes() == b"TCA"
    track.close()
    with pytest.raises(ValueError):
        sequence.TwoBitTrack.from_letters(b"ACGT", other="n")


# ------------------------------------------------------------ 3. and 6. torch tensors: letters that never leave the device; the top of int32 --
def test_from_letters_dev_on_torch_tensors():
    """TwoBitTrack.from_letters_dev on torch tensors, in a process of its own (torch brings its own HIP runtime, which the rest of the
    suite keeps out of the test process): the tensor matrix_dev returns, with no host copy in between, and again after an edit on
    the device; a misaligned slice; a stream of the caller's; a refusal.  Then size = 2^31 - 1: a torch-filled tensor, runs planted
    at 0, across 2^30 and through the last tile up to size; the block arrays, and the letters read back on twobit_cases.TOP_WINDOWS.
    The only large case."""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import os
import build_cases as BC
import build_model as B
import twobit_cases as TC
import twobit_model as M
from bxmi import _ffi, sequence

def arrays_equal(track, built, key):
    got = track.arrays()
    assert (track.size, track.n_blocks, track.m_blocks) == (built.seq.size, len(built.seq.n_starts), len(built.seq.m_starts)), key
    assert B.same_arrays(got, built.seq), key

genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, "multi.2bit"))
names = genome.chroms
rng = np.random.default_rng(441)
track_of = rng.integers(0, len(names), size=37).astype(np.int32)
starts = np.array([rng.integers(-5, max(genome.sizes[names[t]], 1)) for t in track_of], dtype=np.int32)
width = 113
on_device = genome.matrix_dev(torch.from_numpy(track_of).cuda(), torch.from_numpy(starts).cuda(), width)
track = sequence.TwoBitTrack.from_letters_dev(on_device)  # (no copy in between: the tensor as matrix_dev returned it)
built = B.from_letters(genome.matrix(track_of, starts, width).reshape(-1))
assert built.first_other is None and built.seq.size == 37 * width and len(built.seq.m_starts) > 0 and len(built.seq.n_starts) > 0
arrays_equal(track, built, "matrix_dev")
on_device[5, 7:20] = ord("n")  # edited on the device and built again
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
edited = sequence.TwoBitTrack.from_letters_dev(on_device, stream=side.cuda_stream)
arrays_equal(edited, B.from_letters(on_device.cpu().numpy().reshape(-1)), "edited")
flat = on_device.reshape(-1)[3:2000]
assert flat.data_ptr() % 16 == 3
odd = sequence.TwoBitTrack.from_letters_dev(flat)
arrays_equal(odd, B.from_letters(flat.cpu().numpy()), "misaligned")
flat[1000] = ord("R")
try:
    sequence.TwoBitTrack.from_letters_dev(flat)
    raise SystemExit("not refused")
except _ffi.BxmiError as e:
    assert e.code == _ffi.EINVAL and "position 1000 holds byte 0x52" in str(e), str(e)
arrays_equal(sequence.TwoBitTrack.from_letters_dev(flat, other="N"), B.from_letters(flat.cpu().numpy()), "other")
for bad in (on_device.cpu(), on_device.to(torch.int8), on_device[:, ::2]):
    try:
        sequence.TwoBitTrack.from_letters_dev(bad)
        raise SystemExit("accepted")
    except ValueError:
        pass
for t in (track, edited, odd):
    t.close()
genome.close()
del on_device, flat

size = TC.TOP_SIZE
pattern = np.frombuffer(b"ACGTTGCAGATTACAC" * 256, dtype=np.uint8)  # 4096 letters
letters = torch.from_numpy(pattern.copy()).cuda().repeat(1 << 19)[:size]
half = 1 << 30
n_runs = [(0, 100), (half - 500, half + 700), (size - 3 * BC.T - 5, size - 2 * BC.T - 1)]
m_runs = [(half - 500, half + 700), (size - BC.T - 77, size)]
for a, b in n_runs[::2]:
    letters[a:b] = ord("N")
letters[half - 500:half + 700] = ord("n")
letters[m_runs[1][0]:size] |= 0x20
track = sequence.TwoBitTrack.from_letters_dev(letters)
assert (track.size, track.n_blocks, track.m_blocks) == (size, 3, 2)
blocks = [np.zeros(k, dtype=np.int32) for k in (3, 3, 2, 2)]
_ffi.call("bxmi_twobit_arrays", track._h, None, *[_ffi.ptr(b) for b in blocks])  # (the packed bytes, 512 MiB, stay where they are)
assert [(s, s + n) for s, n in zip(blocks[0].tolist(), blocks[1].tolist())] == n_runs
assert [(s, s + n) for s, n in zip(blocks[2].tolist(), blocks[3].tolist())] == m_runs
windows = TC.TOP_WINDOWS + ((n_runs[2][0] - 10, n_runs[2][1] + 10),)
got, offsets = sequence.sequences([track], [0] * len(windows), [w[0] for w in windows], [w[1] for w in windows])
for k, (a, b) in enumerate(windows):
    assert np.array_equal(got[offsets[k]:offsets[k + 1]], letters[a:b].cpu().numpy()), (a, b)
counts = sequence.composition([track], [0], [0], [size])[0]
assert counts[4] == 100 + 1200 + (BC.T + 4) and counts[5] == 1200 + BC.T + 77 and counts[:5].sum() == size
track.close()
print("build dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "build dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])
