"""
Strand-aware 2bit rows on the device (bxmi_twobit_bases_strand*, bxmi_twobit_composition_strand*, bxmi_twobit_kmer_counts_strand*,
the `strands` keyword of bxmi.sequence and bxmi.kmers, TwoBitSet, the -s flag of both command lines) against the answers recorded
from the reference's ``get(s, e).translate(DNA_COMP)[::-1]`` and its count_ngrams over that string (tests/golden/strand) and, beyond
them, against tests/strand_model.py -- itself pinned to those recordings by tests/test_strand_model_golden.py -- on the seeded cases
of tests/strand_cases.py, which tests/test_strand_kernel_host.py runs through the kernels' text on the host.  Integer work: every
comparison is exact.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_cases as KC
import kmer_model as K
import strand_cases as SC
import strand_model as S
import twobit_cases as TC
import twobit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_bases_strand_dev", "bxmi_twobit_composition_strand_dev", "bxmi_twobit_kmer_counts_strand_dev")
GARBAGE = 0x5A5A5A5A
SENTINEL = -286331154  # 0xEEEEEEEE


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def i8(strands):
    return None if strands is None else np.ascontiguousarray(strands, dtype=np.int8)


class Rows:
    """track_of, start, strand and the offsets of a batch in device memory; freed on leaving"""

    def __init__(self, track_of, starts, strands, offsets, extra=()):
        from bxmi import _ffi as ffi

        self.held = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts) + tuple(extra)]
        self.strand = ffi.DeviceArray.from_numpy(i8(strands)) if strands is not None and len(strands) else None
        self.offsets = ffi.DeviceArray.from_numpy(offsets) if offsets is not None else None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.held + [self.strand, self.offsets]:
            if a is not None:
                a.free()

    def ptr(self, which):
        a = {"strand": self.strand, "offsets": self.offsets}.get(which) if isinstance(which, str) else self.held[which]
        return a.ptr if a is not None else None


def between_sentinels(cells, dtype, lead, tail, fill):
    """a device allocation of lead + cells + tail elements: sentinels around garbage -> (the array, check(): the body after the
    call, the sentinels verified)"""
    from bxmi import _ffi as ffi

    sentinel = SENTINEL if dtype == np.int32 else 0xEE
    filled = np.full(lead + cells + tail, sentinel, dtype=dtype)
    filled[lead:lead + cells] = fill
    out = ffi.DeviceArray.from_numpy(filled)

    def check():
        ffi.call("bxmi_synchronize", None)
        got = out.to_numpy(dtype)
        out.free()
        assert (got[:lead] == sentinel).all() and (got[lead + cells:] == sentinel).all(), "written outside the output"
        return got[lead:lead + cells]

    return out, check


class OnDevice:
    """one form of the library as a device of the check functions of strand_cases: the host forms (outputs pre-filled with garbage)
    or the _dev entry points (outputs between sentinels).  strands None goes to the unstranded entry point.  `force` goes through
    bxmi_twobit_kmer_force, `slack` to the _dev form alone; the slabs, the grid and the alignment of the host forms are the library's
    own; `misalign` moves the _dev form's output off a 16-byte boundary."""

    def __init__(self, held, dev):
        self.held, self.dev = held, dev

    def bases(self, seqs, track_of, starts, strands, lengths=None, width=0, do_mask=True, pad=ord("N"), misalign=0, slab=0):
        from bxmi import _ffi as ffi

        tracks = self.held.tracks_of(seqs)
        n = len(track_of)
        offsets = None if lengths is None else offsets_of(lengths)
        total = n * width if offsets is None else int(offsets[-1])
        stranded = strands is not None
        name = "bxmi_twobit_bases_strand" if stranded else "bxmi_twobit_bases"
        if not self.dev:
            t, s, m = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32), i8(strands)
            out = np.full(total, 0x5A, dtype=np.uint8)
            ffi.call(name, ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), *((ffi.ptr(m),) if stranded else ()), n, width, ffi.ptr(offsets), total,
                     int(do_mask), pad, ffi.ptr(out))
            return out
        with Rows(track_of, starts, strands, offsets) as rows:
            out, check = between_sentinels(total, np.uint8, 16 + misalign, 9, 0x5A)
            ffi.call(name + "_dev", ffi.handles(tracks), len(tracks), rows.ptr(0), rows.ptr(1), *((rows.ptr("strand"),) if stranded else ()), n, width,
                     rows.ptr("offsets"), total, int(do_mask), pad, out.ptr + 16 + misalign, None)
            return check()

    def composition(self, seqs, track_of, starts, ends, strands, do_mask=True):
        from bxmi import _ffi as ffi

        tracks = self.held.tracks_of(seqs)
        n = len(track_of)
        stranded = strands is not None
        name = "bxmi_twobit_composition_strand" if stranded else "bxmi_twobit_composition"
        if not self.dev:
            t, s, e, m = (np.ascontiguousarray(a, dtype=np.int32) for a in (track_of, starts, ends)) + (i8(strands),) if False else (
                np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32), np.ascontiguousarray(ends, dtype=np.int32),
                i8(strands))
            out = np.full((n, 6), GARBAGE, dtype=np.int32)
            ffi.call(name, ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), *((ffi.ptr(m),) if stranded else ()), ffi.ptr(e), n, int(do_mask),
                     ffi.ptr(out))
            return out
        with Rows(track_of, starts, strands, None, extra=(ends,)) as rows:
            out, check = between_sentinels(6 * n, np.int32, 4, 6, GARBAGE)
            ffi.call(name + "_dev", ffi.handles(tracks), len(tracks), rows.ptr(0), rows.ptr(1), *((rows.ptr("strand"),) if stranded else ()), rows.ptr(2), n,
                     int(do_mask), out.ptr + 16, None)
            return check().reshape(n, 6)

    def counts(self, seqs, track_of, starts, strands, k, radix, digits, lengths=None, width=0, do_mask=True, force=0, slack=0, grid=0, slab_rows=0):
        from bxmi import _ffi as ffi

        tracks = self.held.tracks_of(seqs)
        n, bins = len(track_of), radix ** k
        offsets = None if lengths is None else offsets_of(lengths)
        total = n * width if offsets is None else int(offsets[-1]) + (slack if self.dev else 0)
        stranded = strands is not None
        name = "bxmi_twobit_kmer_counts_strand" if stranded else "bxmi_twobit_kmer_counts"
        d8 = np.ascontiguousarray(digits, dtype=np.int8)
        ffi.call("bxmi_twobit_kmer_force", force)
        try:
            if not self.dev:
                t, s, m = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32), i8(strands)
                out = np.full((n, bins), GARBAGE, dtype=np.int32)
                ffi.call(name, ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), *((ffi.ptr(m),) if stranded else ()), n, width, ffi.ptr(offsets),
                         total, int(do_mask), k, radix, ffi.ptr(d8), ffi.ptr(out))
                return out
            with Rows(track_of, starts, strands, offsets) as rows:
                out, check = between_sentinels(n * bins, np.int32, 5, 7, GARBAGE)
                ffi.call(name + "_dev", ffi.handles(tracks), len(tracks), rows.ptr(0), rows.ptr(1), *((rows.ptr("strand"),) if stranded else ()), n, width,
                         rows.ptr("offsets"), total, int(do_mask), k, radix, ffi.ptr(d8), out.ptr + 20, None)
                return check().reshape(n, bins)
        finally:
            ffi.call("bxmi_twobit_kmer_force", 0)


class Held:
    """the tracks that the cases of a test put on the device, each once, all closed again whatever the test does"""

    def __init__(self):
        self.tracks = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for _, track in self.tracks.values():
            track.close()

    def tracks_of(self, seqs):
        from bxmi import sequence

        for s in seqs:
            if id(s) not in self.tracks:
                self.tracks[id(s)] = (s, sequence.TwoBitTrack(s))
        return [self.tracks[id(s)][1] for s in seqs]


def both_forms(held):
    return [OnDevice(held, False), OnDevice(held, True)]


# ------------------------------------------------------------ every recording, through every layer --
@pytest.mark.parametrize("name", M.FILES)
def test_recorded_letters_and_base_counts(name):
    """all recorded regions of a file as ONE ragged minus batch per do_mask setting through TwoBitSet, the module functions, the host
    form and the _dev form: the reference's reverse-complemented strings, and the base counts of their characters"""
    from bxmi import sequence

    checked = 0
    with Held() as held:
        for do_mask in (True, False):
            seqs, track_of, starts, ends, want = S.recorded_rows(name, do_mask)
            lengths = [e - s for s, e in zip(starts, ends)]
            minus = ["-"] * len(want)
            counted = [[w.upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in w)] for w in want]
            genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
            tracks = list(genome.tracks.values())
            assert genome.strings(track_of, starts, ends, strands=minus) == want, (name, do_mask)
            assert sequence.strings(tracks, track_of, starts, ends, do_mask, [1] * len(want)) == want
            assert genome.composition(track_of, starts, ends, strands=minus).tolist() == counted
            assert sequence.composition(tracks, track_of, starts, ends, do_mask, strands=[True] * len(want)).tolist() == counted
            assert genome.strings(track_of, starts, ends, strands=["+"] * len(want)) == genome.strings(track_of, starts, ends)
            genome.close()
            for dev in both_forms(held):
                got = dev.bases(seqs, track_of, starts, [1] * len(want), lengths=lengths, do_mask=do_mask)
                assert got.tobytes().decode() == "".join(want), (name, do_mask, dev.dev)
                assert dev.composition(seqs, track_of, starts, ends, [1] * len(want), do_mask).tolist() == counted
            checked += len(want)
    assert checked == len(S.manifest()["files"][name]["strings"])


@pytest.mark.parametrize("name", M.FILES)
def test_recorded_counts(name):
    """the recorded regions as one ragged minus batch per do_mask setting, mapping and k, through TwoBitSet and the module functions
    with drop_last (which shortens a minus region at its start), the host form and the _dev form: the reference's own counts"""
    from bxmi import kmers, sequence

    checked = 0
    with Held() as held:
        for do_mask in (True, False):
            genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
            tracks = list(genome.tracks.values())
            for mapping, k, seqs, track_of, starts, ends, want in S.recorded_batches(name, do_mask):
                alphabet, case_sensitive = K.ALPHABETS[mapping]
                letters, radix = K.MAPPINGS[mapping]
                minus = ["-"] * len(want)
                got = genome.kmer_counts(track_of, starts, ends, k, alphabet, case_sensitive, drop_last=True, strands=minus)
                assert got.dtype == np.int32 and np.array_equal(got, want), (name, do_mask, mapping, k)
                assert np.array_equal(kmers.counts(tracks, track_of, starts, ends, k, alphabet, case_sensitive, do_mask, True, [1] * len(want)), want)
                digits = K.digits8(K.table_of(letters))
                lengths = [max(e - s - 1, 0) for s, e in zip(starts, ends)]
                first = [s + 1 if e > s else s for s, e in zip(starts, ends)]
                for dev in both_forms(held):
                    got = dev.counts(seqs, track_of, first, [1] * len(want), k, radix, digits, lengths=lengths, do_mask=do_mask, slack=3 * K.TILE + 1)
                    assert np.array_equal(got, want), (name, do_mask, mapping, k, dev.dev)
                checked += len(want)
            genome.close()
    assert checked == len(S.manifest()["files"][name]["entries"])


# ------------------------------------------------------------ the seeded cases of tests/strand_cases.py --
def test_ragged_rows_of_either_strand():
    with Held() as held:
        SC.check_letters(both_forms(held), SC.letters_ragged_case(), where="ragged")


@pytest.mark.parametrize("width", (1, 37, M.TILE + 1))
def test_matrix_rows_of_either_strand(width):
    from bxmi import sequence

    case = SC.letters_matrix_case(width)
    with Held() as held:
        SC.check_letters(both_forms(held), case, where="width %d" % width)
        tracks = held.tracks_of(case["seqs"])
        want, _ = SC.want_letters(case, True, ord("-"))
        got = sequence.matrix(tracks, case["track_of"], case["starts"], width, b"-", True, ["-" if m else "+" for m in case["strands"]])
        assert got.shape == (len(case["starts"]), width) and np.array_equal(got.reshape(-1), want)


def test_one_base_blocks_at_the_ends_of_a_minus_row():
    with Held() as held:
        SC.check_letters(both_forms(held), SC.letters_edge_case(), where="edges")


def test_base_counts_of_either_strand():
    with Held() as held:
        SC.check_composition(both_forms(held), SC.composition_case(), where="composition")


@pytest.mark.parametrize("k", (1, 2, 7))
def test_windows_across_words_runs_tiles_and_segments(k):
    with Held() as held:
        SC.check_counts(both_forms(held), SC.boundary_case(k), where="boundary k=%d" % k)


@pytest.mark.parametrize("table", ("ry", "no_g", "shared"))
def test_digit_tables_closed_under_complement_and_not(table):
    with Held() as held:
        SC.check_counts(both_forms(held), SC.boundary_case(3, table), where=table)


def test_both_ways_of_accumulating_windows_of_one_width_and_a_palindrome():
    with Held() as held:
        SC.check_counts(both_forms(held), SC.plan_case(), where="plan")
        SC.check_counts(both_forms(held), SC.window_case(37, 3), where="width 37")
        SC.check_counts(both_forms(held), SC.palindrome_case(), where="palindrome")


def test_a_minus_row_of_more_tiles_than_the_grid_and_thousands_of_mixed_rows_in_a_tile():
    """one MINUS row of 1.5 x (compute units x 8) k-mer tiles: every workgroup adds to the same row of counts, some after two tiles;
    2 500 rows of 0 .. 3 bases, a random half minus, in one tile"""
    import ctypes as C

    from bxmi import _ffi

    dev, cus = C.c_int(0), C.c_int(0)
    _ffi.call("bxmi_get_device", C.byref(dev))
    _ffi.call("bxmi_device_info", dev.value, None, 0, C.byref(cus), None)
    fill = cus.value * 8
    tiles = fill + fill // 2
    assert cus.value > 0 and tiles > fill
    with Held() as held:
        SC.check_counts(both_forms(held), SC.long_row_case(tiles), where="one long minus row")
        many = SC.many_rows_case()
        assert len(many["starts"]) == 2500 and 1000 < sum(many["strands"]) < 1500
        SC.check_counts(both_forms(held), many, where="many rows")


# ------------------------------------------------------------ the Python layer --
def test_drop_last_bad_strands_and_nothing_to_do():
    from bxmi import kmers, sequence

    seqs = M.structural_sequences()
    model = S.Strand(seqs)
    table = KC.TABLES["dna"][0]
    with Held() as held:
        tracks = held.tracks_of(seqs)
        # drop_last on a minus row drops the window at the interval's START
        t, s, e, m = [0, 0, 1, 0, 0], [100, 100, 0, 50, -5], [140, 140, 41, 50, 3], ["-", "+", "-", "-", "-"]
        s_c, n_c = [100, 100, 0, 50, 0], [40, 40, 41, 0, 3]
        want = model.counts(t, s_c, n_c, m, 3, 4, table, drop_last=True)
        assert not np.array_equal(want[0], want[1]) and np.array_equal(want[0], model.counts([0], [101], [39], [1], 3, 4, table)[0])
        assert np.array_equal(kmers.counts(tracks, t, s, e, 3, "ACGT", False, True, True, m), want)
        want = model.counts([0, 0, 1], [100, 100, 3], [40, 40, 40], [1, 0, 1], 3, 4, table, drop_last=True)
        assert np.array_equal(kmers.count_matrix(tracks, [0, 0, 1], [100, 100, 3], 40, 3, "ACGT", False, True, True, [1, 0, 1]), want)
        assert not kmers.count_matrix(tracks, [0, 0], [100, 200], 1, 1, drop_last=True, strands="-+").any()
        # anything but "+", "-", bools, 0 and 1 is a ValueError, as is a wrong number of entries
        for bad in (["x", "+"], [2, 0], [0.5, 1], ["+"], [None, 1]):
            for call in (lambda: sequence.matrix(tracks, [0, 0], [5, 6], 4, strands=bad), lambda: sequence.strings(tracks, [0, 0], [5, 6], [9, 9], strands=bad),
                         lambda: sequence.composition(tracks, [0, 0], [5, 6], [9, 9], strands=bad), lambda: kmers.counts(tracks, [0, 0], [5, 6], [9, 9], 2, strands=bad),
                         lambda: kmers.count_matrix(tracks, [0, 0], [5, 6], 4, 2, strands=bad)):
                with pytest.raises(ValueError):
                    call()
        assert sequence.strings(tracks, [], [], [], strands=[]) == [] and sequence.matrix(tracks, [], [], 5, strands=[]).shape == (0, 5)
        assert sequence.composition(tracks, [], [], [], strands=[]).shape == (0, 6) and kmers.counts(tracks, [], [], [], 3, strands=[]).shape == (0, 64)
        assert sequence.strings(tracks, [0, 2, -1], [5, 0, 9], [5, 0, 30], strands="---") == ["", "", ""]


def test_folded_counts_do_not_depend_on_the_strand():
    """fold_reverse_complement(counts with strands) == fold_reverse_complement(counts without), case-folded ACGT"""
    from bxmi import kmers

    case = SC.boundary_case(2)
    ends = [s + n for s, n in zip(case["starts"], case["lengths"])]
    with Held() as held:
        tracks = held.tracks_of(case["seqs"])
        for k in (1, 2, 5):
            plus = kmers.counts(tracks, case["track_of"], case["starts"], ends, k, "ACGT", False)
            minus = kmers.counts(tracks, case["track_of"], case["starts"], ends, k, "ACGT", False, strands=[1] * len(ends))
            assert plus.sum() > 1000 and not np.array_equal(plus, minus)
            assert np.array_equal(kmers.fold_reverse_complement(minus, k), kmers.fold_reverse_complement(plus, k))
            assert np.array_equal(minus, plus[:, kmers.strand_columns(k, "ACGT", False)])


# ------------------------------------------------------------ the top of int32 --
def test_a_minus_row_at_the_top_of_int32():
    """twobit_cases.TopSequence, 2^31 - 1 bases (512 MiB of device memory: given back whatever happens): minus rows whose positions
    reach 2^31 - 2, cross the size and begin at it -- start + (len - 1 - j) beyond int32 -- and the base counts of the whole sequence,
    whose T count is beyond 2^30"""
    top = TC.top_sequence()
    size = top.size
    rows = [(size - 100, 100), (size - 100, 300), (size - 1, 9), (size, 50), ((1 << 30) - 2500, 1000), (size - 8192 - 40, 100), (-50, 100),
            (size - M.TILE - 7, M.TILE + 40)]
    starts, lengths = [r[0] for r in rows], [r[1] for r in rows]
    assert starts[0] + lengths[0] - 1 == 2 ** 31 - 2 and max(s + n for s, n in rows) > 2 ** 31
    minus = [1] * len(rows)

    def want_row(s, n, do_mask, pad):
        plus = top.row(s, n, do_mask, 0)
        return np.where(plus != 0, S.COMPLEMENT[plus], pad).astype(np.uint8)[::-1]

    with Held() as held:
        devices = both_forms(held)
        for do_mask in (True, False):
            want = np.concatenate([want_row(s, n, do_mask, ord("-")) for s, n in rows])
            plus = np.concatenate([top.row(s, n, do_mask, ord("-")) for s, n in rows])
            assert (want[:100] != ord("-")).all() and (want[100:300] == ord("-")).all() and (want[300:400] != ord("-")).all() and not np.array_equal(want, plus)
            for dev in devices:
                got = dev.bases([top.seq], [0] * len(rows), starts, minus, lengths=lengths, do_mask=do_mask, pad=ord("-"))
                assert np.array_equal(got, want), (do_mask, dev.dev, np.flatnonzero(got != want)[:10])
            table, radix = KC.TABLES["dna"]
            counts = np.array([K.count_text(want_row(s, n, do_mask, 0), 3, radix, table) for s, n in rows], dtype=np.int32)
            assert counts[0].sum() > 50 and counts[3].sum() == 0
            for dev in devices:
                got = dev.counts([top.seq], [0] * len(rows), starts, minus, 3, radix, K.digits8(table), lengths=lengths, do_mask=do_mask)
                assert np.array_equal(got, counts), (do_mask, dev.dev)
            # the int32-top rows of the base counts
            c_starts, c_ends = [0, 1, size - 1, size, -7, TC.TOP_N[0] - 3], [size, size - 1, size, size, size, TC.TOP_N[1] + 3]
            strand = [1, 0, 1, 1, 1, 1]
            base = top.composition(c_starts, c_ends, do_mask)
            swapped = np.where(np.array(strand, dtype=bool)[:, None], base[:, [3, 2, 1, 0, 4, 5]], base)
            assert base[0, 3] > 1 << 30 and swapped[0, 0] == base[0, 3] and swapped.max() < 2 ** 31
            for dev in devices:
                got = dev.composition([top.seq], [0] * len(c_starts), c_starts, c_ends, strand, do_mask)
                assert np.array_equal(got, swapped), (do_mask, dev.dev, got.tolist(), swapped.tolist())


# ------------------------------------------------------------ device entry points on torch tensors --
def test_dev_forms_on_torch_tensors():
    """matrix_dev / sequences_dev / composition_dev / counts_dev / count_matrix_dev with `strands` on torch tensors (int8, uint8 and
    bool), on torch's current stream and on a side stream, with `out` given, through TwoBitSet as well, in a process of its own:
    torch brings its own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import twobit_model as M
import kmer_cases as KC
import strand_model as S
from bxmi import kmers, sequence

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

def same(got, want):
    got = got.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)

seqs = M.structural_sequences()
model = S.Strand(seqs)
dev = [sequence.TwoBitTrack(s) for s in seqs]
side = torch.cuda.Stream()
table = KC.TABLES["dna"][0]

track_of, starts, lengths = M.ragged_case()
n = len(track_of)
minus = [(i * 7 + 1) % 3 != 0 for i in range(n)]
ends = [s + k for s, k in zip(starts, lengths)]
clip = [(max(s, 0), max(min(e, seqs[t].size if 0 <= t < len(seqs) else 0) - max(s, 0), 0)) for t, s, e in zip(track_of, starts, ends)]
s_c, n_c = [c[0] for c in clip], [c[1] for c in clip]
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
strand_tensors = [torch.tensor(minus, dtype=torch.bool, device="cuda"), torch.tensor(minus, dtype=torch.int8, device="cuda"),
                  torch.tensor([7] + [int(m) * 200 for m in minus], dtype=torch.uint8, device="cuda")[1:]]  # (any non-zero entry is minus)
for do_mask in (True, False):
    want, want_off = model.bases(track_of, s_c, n_c, minus, do_mask)
    plus, _ = model.bases(track_of, s_c, n_c, None, do_mask)
    assert not np.array_equal(want, plus)
    for which, st in enumerate(strand_tensors):
        got, off = sequence.sequences_dev(dev, *d, do_mask=do_mask, strands=st)
        torch.cuda.synchronize()
        assert same(got, want) and same(off, want_off), (do_mask, which)
    got, off = sequence.sequences_dev(dev, *d, do_mask=do_mask, stream=side.cuda_stream, strands=strand_tensors[0])
    side.synchronize()
    assert same(got, want), (do_mask, "side stream")
    got, _ = sequence.sequences_dev(dev, *d, do_mask=do_mask)
    torch.cuda.synchronize()
    assert same(got, plus)
    want_c = model.composition(track_of, starts, ends, minus, do_mask)
    got = sequence.composition_dev(dev, *d, do_mask=do_mask, stream=side.cuda_stream, strands=strand_tensors[1])
    side.synchronize()
    assert same(got, want_c) and not np.array_equal(want_c, model.composition(track_of, starts, ends, None, do_mask))
    for k, drop_last in ((2, False), (3, True), (6, False)):
        want_k = model.counts(track_of, s_c, n_c, minus, k, 4, table, do_mask, drop_last)
        assert want_k.sum() > 1000
        got = kmers.counts_dev(dev, *d, k, case_sensitive=False, do_mask=do_mask, drop_last=drop_last, strands=strand_tensors[2])
        torch.cuda.synchronize()
        assert same(got, want_k), (do_mask, k)
        out = torch.full(want_k.shape, 77, dtype=torch.int32, device="cuda")
        res = kmers.counts_dev(dev, *d, k, case_sensitive=False, do_mask=do_mask, drop_last=drop_last, stream=side.cuda_stream, out=out, strands=strand_tensors[0])
        side.synchronize()
        assert res is out and same(out, want_k), (do_mask, k, "out given, side stream")

for width in (37, M.TILE + 1):
    track_of_m, starts_m = M.matrix_case(width)
    m = [i % 2 == 0 for i in range(len(track_of_m))]
    st = torch.tensor(m, dtype=torch.bool, device="cuda")
    rows = [dev_i32(track_of_m, 1), dev_i32(starts_m, 2)]
    want = model.matrix(track_of_m, starts_m, width, m, True, ord("A"))
    # `out` one byte off a 16-byte boundary, sentinels before and after it
    whole = torch.full((len(m) * width + 40,), 0xEE, dtype=torch.uint8, device="cuda")
    out = whole[17:17 + len(m) * width].view(len(m), width)
    res = sequence.matrix_dev(dev, *rows, width, b"A", stream=side.cuda_stream, out=out, strands=st)
    side.synchronize()
    assert res is out and same(out, want) and bool((whole[:17] == 0xEE).all()) and bool((whole[17 + len(m) * width:] == 0xEE).all()), width
    got = sequence.matrix_dev(dev, *rows, width, b"A", strands=st)
    torch.cuda.synchronize()
    assert same(got, want), width
    for drop_last in (False, True):
        want_k = model.counts(track_of_m, starts_m, [width] * len(m), m, 3, 4, table, True, drop_last)
        out = torch.full(want_k.shape, 5, dtype=torch.int32, device="cuda")
        res = kmers.count_matrix_dev(dev, *rows, width, 3, case_sensitive=False, drop_last=drop_last, stream=side.cuda_stream, out=out, strands=st)
        side.synchronize()
        assert res is out and same(out, want_k), (width, drop_last)
for bad in (torch.zeros(len(m), dtype=torch.int32, device="cuda"), torch.zeros(len(m) + 1, dtype=torch.int8, device="cuda"), torch.zeros(len(m), dtype=torch.int8), [0] * len(m)):
    try:
        sequence.matrix_dev(dev, *rows, width, strands=bad)
        raise SystemExit("wrong strands were accepted")
    except ValueError:
        pass

# through TwoBitSet; entries the device forms cannot refuse are rows of pad or of zeros
genome = sequence.TwoBitSet({"blocks": seqs[0], "odd": seqs[1]}, do_mask=True)
t2, s2, e2 = dev_i32(np.array([0, 1, 5, -1]), 0), dev_i32(np.array([100, 0, 3, 3]), 0), dev_i32(np.array([400, 41, 30, 30]), 0)
st = torch.tensor([1, 1, 1, 0], dtype=torch.int8, device="cuda")
two = S.Strand(seqs[:2])
got = genome.kmer_counts_dev(t2, s2, e2, 2, strands=st)
torch.cuda.synchronize()
assert same(got, two.counts([0, 1, -1, -1], [100, 0, 0, 0], [300, 41, 0, 0], [1, 1, 1, 0], 2, 4, KC.TABLES["acgt"][0], True))
got = genome.kmer_count_matrix_dev(t2, s2, 6, 2, strands=st)
torch.cuda.synchronize()
assert same(got, two.counts([0, 1, -1, -1], [100, 0, 3, 3], [6] * 4, [1, 1, 1, 0], 2, 4, KC.TABLES["acgt"][0], True))
got = genome.matrix_dev(t2, s2, 6, strands=st)
torch.cuda.synchronize()
assert same(got, two.matrix([0, 1, -1, -1], [100, 0, 3, 3], 6, [1, 1, 1, 0]))
got, _ = genome.sequences_dev(t2, s2, e2, strands=st)
torch.cuda.synchronize()
assert same(got, two.bases([0, 1, -1, -1], [100, 0, 0, 0], [300, 41, 0, 0], [1, 1, 1, 0])[0])
got = genome.composition_dev(t2, s2, e2, strands=st)
torch.cuda.synchronize()
assert same(got, two.composition([0, 1, -1, -1], [100, 0, 3, 3], [400, 41, 30, 30], [1, 1, 1, 0]))
got = kmers.counts_dev(dev, d[0][:0], d[1][:0], d[2][:0], 3, stream=side.cuda_stream, strands=strand_tensors[1][:0])
assert tuple(got.shape) == (0, 64)
genome.close()
for t in dev:
    t.close()
print("strand dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "strand dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ------------------------------------------------------------ the command lines --
def test_command_lines_with_the_strand_flag(tmp_path):
    """a BED with "+", "-", "." and a missing strand column: -s prints the model's minus rows for "-" alone, the strand as a fourth
    field; without -s the same BED prints what it always printed"""
    from bxmi import kmers
    from bxmi.cli import twobit_intervals_to_fasta as fasta
    from bxmi.cli import twobit_kmer_counts as kmer_cli

    name = "multi.2bit"
    seqs = M.read(name)
    names = list(seqs)
    rows = [("ckpt", 990, 1100, "-"), ("odd", 0, 41, "+"), ("ckpt", 2565, 2600, "-"), ("odd", 3, 41, "."), ("ckpt", 0, 70, None), ("chrNone", 7, 9, "-"),
            ("odd", 38, 41, "-"), ("empty", 0, 5, "-")]
    bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r[:3] if r[3] is None else "%s\t%d\t%d\tname\t0\t%s\n" % r for r in rows)
    strands = [r[3] if r[3] in ("+", "-") else "+" for r in rows]
    minus = [s == "-" for s in strands]
    track_of = [names.index(r[0]) if r[0] in names else -1 for r in rows]
    sizes = [seqs[n].size for n in names]
    s_c = [max(r[1], 0) for r in rows]
    n_c = [max(min(r[2], sizes[t] if t >= 0 else 0) - s, 0) for r, t, s in zip(rows, track_of, s_c)]
    model = S.Strand([seqs[n] for n in names])
    path = os.path.join(M.GOLDEN, name)
    for flags, do_mask in (([], True), (["-u"], False)):
        data, offsets = model.bases(track_of, s_c, n_c, minus, do_mask)
        texts = [data[a:b].tobytes().decode() for a, b in zip(offsets[:-1], offsets[1:])]
        plain = [t.tobytes().decode() for t in (model.row(t, s, n, False, do_mask) for t, s, n in zip(track_of, s_c, n_c))]
        assert texts[0] == S.reverse_complement_str(plain[0]) != plain[0] and len(texts[0]) > 100 and texts[3] == plain[3] and texts[4] == plain[4]
        out = io.StringIO()
        fasta.main([path, "-s"] + flags, stdin=io.StringIO(bed), out=out)
        want = "".join("> %s %d %d %s\n" % (r[0], r[1], r[2], st) + "".join(t[c:c + 50] + "\n" for c in range(0, len(t), 50)) for r, st, t in zip(rows, strands, texts))
        assert out.getvalue() == want, flags
        out = io.StringIO()
        fasta.main([path] + flags, stdin=io.StringIO(bed), out=out)
        assert out.getvalue() == "".join("> %s %d %d\n" % r[:3] + "".join(t[c:c + 50] + "\n" for c in range(0, len(t), 50)) for r, t in zip(rows, plain)), flags
        out = io.StringIO()
        fasta.main([path, "-c", "-s"] + flags, stdin=io.StringIO(bed), out=out)
        counted = [[t.upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in t)] for t in texts]
        assert out.getvalue() == "".join("\t".join([r[0], str(r[1]), str(r[2]), st] + [str(x) for x in c]) + "\n" for r, st, c in zip(rows, strands, counted)), flags
        assert counted[0] != [plain[0].upper().count(c) for c in "ACGTN"] + [sum(ch.islower() for ch in plain[0])]
        for more, table in (([], "acgt"), (["-i"], "dna"), (["-c", "-i"], "dna")):
            want = model.counts(track_of, s_c, n_c, minus, 2, 4, KC.TABLES[table][0], do_mask)
            assert not np.array_equal(want, K.Counts(model.letters).counts(track_of, s_c, n_c, 2, 4, KC.TABLES[table][0], do_mask)) or "-c" in more
            labels = kmers.words(2)
            if "-c" in more:
                keep = kmers.canonical_columns(2)
                want, labels = kmers.fold_reverse_complement(want, 2)[:, keep], [labels[i] for i in keep]
            out = io.StringIO()
            kmer_cli.main([path, "2", "-s"] + flags + more, stdin=io.StringIO(bed), out=out)
            text = "\t".join(["#chrom", "start", "end", "strand"] + labels) + "\n"
            text += "".join("\t".join([r[0], str(r[1]), str(r[2]), st] + [str(c) for c in line]) + "\n" for r, st, line in zip(rows, strands, want.tolist()))
            assert out.getvalue() == text and want.any(), (flags, more)
        saved = tmp_path / "out.npy"
        kmer_cli.main([path, "-o", str(saved), "2", "-s"] + flags, stdin=io.StringIO(bed), out=io.StringIO())
        assert np.array_equal(np.load(saved), model.counts(track_of, s_c, n_c, minus, 2, 4, KC.TABLES["acgt"][0], do_mask)), flags
