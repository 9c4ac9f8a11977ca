"""
K-mer counts over 2bit rows on the device (bxmi_twobit_kmer_counts*, bxmi.kmers, TwoBitSet.kmer_counts / kmer_count_matrix,
bxmi.cli.twobit_kmer_counts) against the answers recorded from the reference's count_ngrams(mapping.translate(...))
(tests/golden/kmers; every row shortened by one base, the reference's loop) and, beyond them, against tests/kmer_model.py -- itself
pinned to those recordings by tests/test_kmer_model_golden.py -- on the seeded cases of tests/kmer_cases.py, which
tests/test_kmer_kernel_host.py runs through the kernel's text on the host.  Integer counts: every comparison is exact.
"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_cases as KC
import kmer_model as K
import twobit_cases as TC
import twobit_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the _dev entry points this file drives by their C names (tests/test_device_entry_points_abi.py)
DEV_ENTRY_POINTS = ("bxmi_twobit_kmer_counts_dev",)
GARBAGE = 0x5A5A5A5A
SENTINEL = -286331154  # 0xEEEEEEEE


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def counts_host(tracks, track_of, starts, k, radix, digits, lengths=None, width=0, do_mask=True):
    """bxmi_twobit_kmer_counts with the rows as they are (no clipping), `counts` filled with garbage first -> int32 [n, radix ** k]"""
    from bxmi import _ffi as ffi

    t, s = np.ascontiguousarray(track_of, dtype=np.int32), np.ascontiguousarray(starts, dtype=np.int32)
    offsets = None if lengths is None else offsets_of(lengths)
    total = len(t) * width if offsets is None else int(offsets[-1])
    out = np.full((len(t), radix ** k), GARBAGE, dtype=np.int32)
    ffi.call("bxmi_twobit_kmer_counts", ffi.handles(tracks), len(tracks), ffi.ptr(t), ffi.ptr(s), len(t), width, ffi.ptr(offsets), total, int(do_mask), k, radix,
             ffi.ptr(np.ascontiguousarray(digits, dtype=np.int8)), ffi.ptr(out))
    return out


def counts_dev(tracks, track_of, starts, k, radix, digits, lengths=None, width=0, do_mask=True, lead=5, tail=7, slack=0):
    """bxmi_twobit_kmer_counts_dev on arrays in device memory, on the null stream, `counts` `lead` counters into an allocation of
    sentinels, which must still be there on both sides afterwards, the counters themselves garbage before the call; `slack`: how far
    beyond row_off[n] the `total` given lies (ragged form)"""
    from bxmi import _ffi as ffi

    n = len(track_of)
    offsets = None if lengths is None else offsets_of(lengths)
    total = n * width if offsets is None else int(offsets[-1]) + slack
    rows = [ffi.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=np.int32)) for a in (track_of, starts)]
    rows += [ffi.DeviceArray.from_numpy(offsets)] if offsets is not None else []
    cells = n * radix ** k
    filled = np.full(lead + cells + tail, SENTINEL, dtype=np.int32)
    filled[lead:lead + cells] = GARBAGE
    out = ffi.DeviceArray.from_numpy(filled)
    ffi.call("bxmi_twobit_kmer_counts_dev", ffi.handles(tracks), len(tracks), rows[0].ptr, rows[1].ptr, n, width, rows[2].ptr if offsets is not None else None,
             total, int(do_mask), k, radix, ffi.ptr(np.ascontiguousarray(digits, dtype=np.int8)), out.ptr + 4 * lead, None)
    ffi.call("bxmi_synchronize", None)
    got = out.to_numpy(np.int32)
    for a in rows + [out]:
        a.free()
    assert (got[:lead] == SENTINEL).all() and (got[lead + cells:] == SENTINEL).all(), "written outside the counts"
    return got[lead:lead + cells].reshape(n, radix ** k)


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


class OnDevice:
    """one form of the library, host arrays or the _dev entry point, as a device of kmer_cases.check; `force` goes through
    bxmi_twobit_kmer_force, `slack` to the _dev form alone (the host form asks that `total` is where the offsets end); the grid and
    the slabs are the library's own"""

    def __init__(self, held, dev):
        self.held, self.dev = held, dev

    def counts(self, seqs, track_of, starts, k, radix, digits, lengths=None, width=0, do_mask=True, force=0, slack=0, grid=0, slab_rows=0):
        from bxmi import _ffi as ffi

        tracks = self.held.tracks_of(seqs)
        ffi.call("bxmi_twobit_kmer_force", force)
        try:
            if self.dev:
                return counts_dev(tracks, track_of, starts, k, radix, digits, lengths=lengths, width=width, do_mask=do_mask, slack=slack if lengths is not None else 0)
            return counts_host(tracks, track_of, starts, k, radix, digits, lengths=lengths, width=width, do_mask=do_mask)
        finally:
            ffi.call("bxmi_twobit_kmer_force", 0)


def both_forms(held):
    return [OnDevice(held, False), OnDevice(held, True)]


# ------------------------------------------------------------ every recorded case --
@pytest.mark.parametrize("name", M.FILES)
def test_recorded_counts(name):
    """the recorded regions of a file as one ragged batch per do_mask setting, mapping and k, through TwoBitSet and the module
    functions (which clip as `get` and drop the last base), the host form and the _dev form: the reference's own counts"""
    from bxmi import kmers, sequence

    checked = 0
    for do_mask in (True, False):
        genome = sequence.TwoBitSet.from_file(os.path.join(M.GOLDEN, name), do_mask=do_mask)
        tracks = list(genome.tracks.values())
        for mapping, k, seqs, track_of, starts, ends, want in K.recorded_batches(name, do_mask):
            alphabet, case_sensitive = K.ALPHABETS[mapping]
            letters, radix = K.MAPPINGS[mapping]
            got = genome.kmer_counts(track_of, starts, ends, k, alphabet, case_sensitive, drop_last=True)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, do_mask, mapping, k)
            assert np.array_equal(kmers.counts(tracks, track_of, starts, ends, k, alphabet, case_sensitive, do_mask, drop_last=True), want)
            digits = K.digits8(K.table_of(letters))
            lengths = [max(e - s - 1, 0) for s, e in zip(starts, ends)]
            assert np.array_equal(counts_host(tracks, track_of, starts, k, radix, digits, lengths=lengths, do_mask=do_mask), want)
            assert np.array_equal(counts_dev(tracks, track_of, starts, k, radix, digits, lengths=lengths, do_mask=do_mask, slack=3 * K.TILE + 1), want)
            # every window, the last one included: the model without drop_last
            every = K.Counts(seqs).counts(track_of, starts, [e - s for s, e in zip(starts, ends)], k, radix, K.table_of(letters), do_mask)
            assert np.array_equal(genome.kmer_counts(track_of, starts, ends, k, alphabet, case_sensitive), every)
            checked += len(want)
        genome.close()
    assert checked == len(K.manifest()["files"][name]["entries"])


# ------------------------------------------------------------ the seeded cases of tests/kmer_cases.py --
@pytest.mark.parametrize("k", (1, 2, 7))
def test_windows_across_words_runs_tiles_and_segments(k):
    with Held() as held:
        KC.check(both_forms(held), KC.boundary_case(k), where="boundary k=%d" % k)


@pytest.mark.parametrize("k", (1, 2, 7))
def test_one_base_blocks_at_every_offset_of_a_window(k):
    with Held() as held:
        KC.check(both_forms(held), KC.block_edge_case(k), where="edge k=%d" % k)


def test_the_stretch_of_one_base_blocks_and_the_structural_rows():
    with Held() as held:
        KC.check(both_forms(held), KC.stretch_case(2, "acgt"), where="stretch")
        KC.check(both_forms(held), KC.stretch_case(3, "dna"), where="stretch dna")


@pytest.mark.parametrize("width,k", ((1, 1), (37, 3), (K.TILE + 1, 2)))
def test_windows_of_one_width(width, k):
    from bxmi import kmers

    case = KC.window_case(width, k)
    with Held() as held:
        KC.check(both_forms(held), case, where="width %d" % width)
        got = kmers.count_matrix(held.tracks_of(case["seqs"]), case["track_of"], case["starts"], width, k, "ACGT", case_sensitive=False)
        assert np.array_equal(got, KC.want_of(case, True))


@pytest.mark.parametrize("table", ("no_g", "ry", "shared", "ry_folded"))
def test_digit_tables(table):
    """an upper-case letter without a digit, two letters on one digit, radix 2, 3 and 4"""
    with Held() as held:
        KC.check(both_forms(held), KC.boundary_case(3, table), where=table)


@pytest.mark.parametrize("k,table", ((7, "dna"), (14, "ry_folded"), (6, "dna"), (12, "ry"), (13, "ry"), (8, "no_g")))
def test_bins_at_the_maximum_and_around_the_lds_limit(k, table):
    with Held() as held:
        KC.check(both_forms(held), KC.bins_case(k, table), where="bins %s^%d" % (table, k))


def test_both_ways_of_accumulating_agree():
    """segments on both sides of the plan's cut-off, the plan's choice and either way forced: equal counts"""
    with Held() as held:
        KC.check(both_forms(held), KC.plan_case(), where="plan")


def test_a_row_of_more_tiles_than_the_grid_and_thousands_of_rows_in_a_tile():
    """the grid is at most compute units x 8 workgroups, each walking every gridDim.x-th tile: one row of half as many tiles again
    -- every workgroup adds to the same row of counts, some after two tiles -- with a `total` several grid fills beyond it"""
    import ctypes as C

    from bxmi import _ffi

    dev, cus = C.c_int(0), C.c_int(0)
    _ffi.call("bxmi_get_device", C.byref(dev))
    _ffi.call("bxmi_device_info", dev.value, None, 0, C.byref(cus), None)
    fill = cus.value * 8
    tiles = fill + fill // 2
    assert cus.value > 0 and tiles > fill
    with Held() as held:
        KC.check(both_forms(held), KC.long_row_case(tiles), where="one long row")
        KC.check(both_forms(held), KC.many_rows_case(), where="many rows")


def test_nothing_to_do_and_bad_arguments():
    from bxmi import _ffi as ffi
    from bxmi import kmers

    with Held() as held:
        tracks = held.tracks_of(M.structural_sequences())
        assert kmers.counts(tracks, [], [], [], 3).shape == (0, 64)
        assert kmers.count_matrix(tracks, [], [], 5, 2).shape == (0, 16)
        got = kmers.counts(tracks, [0, 2, -1, 0, 0], [5, 0, 9, 30, 40], [5, 0, 30, 31, 20], 2)
        assert got.shape == (5, 16) and not got.any()  # empty, the size-0 sequence, no track, shorter than k, reversed
        assert not kmers.count_matrix(tracks, [0, 0], [100, 200], 1, 1, drop_last=True).any()
        for call in (lambda: kmers.count_matrix(tracks, [0], [0], 0, 2), lambda: kmers.count_matrix(tracks, [len(tracks)], [0], 4, 2),
                     lambda: kmers.counts(tracks, [0, len(tracks)], [0, 0], [4, 4], 2)):
            with pytest.raises(ffi.BxmiError) as e:
                call()
            assert e.value.code == ffi.EINVAL
        with pytest.raises(ValueError):
            kmers.counts(tracks, [0], [0], [9], 8)


# ------------------------------------------------------------ the top of int32 --
def test_counts_at_the_top_of_int32():
    """twobit_cases.TopSequence, 2^31 - 1 bases (512 MiB of device memory: given back whatever happens): rows over TOP_WINDOWS, rows
    that end at the size, cross it and begin at it, a row across the middle window's edge.  Positions, the packed words and the
    blocks' edges next to the top of int32; k = 3 under the case-folded mapping, k = 7 (straight to HBM) under the upper-case one"""
    top = TC.top_sequence()
    rows = [(a, b - a) for a, b in TC.TOP_WINDOWS] + [(top.size - 100, 300), (top.size, 50), (top.size - 1, 9), ((1 << 30) - 2500, 1000),
                                                      (top.size - 8192 - 40, 100)]
    starts, lengths = [r[0] for r in rows], [r[1] for r in rows]
    assert max(starts) == top.size and max(s + n for s, n in rows) > 2 ** 31
    with Held() as held:
        tracks = held.tracks_of([top.seq])
        for k, name in ((3, "dna"), (7, "acgt")):
            table, radix = KC.TABLES[name]
            for do_mask in (True, False):
                want = np.array([K.count_text(top.row(s, n, do_mask, 0), k, radix, table) for s, n in rows], dtype=np.int32)
                assert want[:3].sum(axis=1).min() > 0 or (name == "acgt" and do_mask)  # (the middle window lies in the large mask block)
                assert want[0].sum() > 1000 and want[4].sum() == 0
                for form in (counts_host, counts_dev):
                    got = form(tracks, [0] * len(rows), starts, k, radix, K.digits8(table), lengths=lengths, do_mask=do_mask)
                    assert np.array_equal(got, want), (k, name, do_mask, form.__name__, np.flatnonzero((got != want).any(axis=1)))


# ------------------------------------------------------------ device entry points on torch tensors --
def test_dev_forms_on_torch_tensors():
    """counts_dev / count_matrix_dev on torch tensors, on torch's current stream and on a stream of the caller's (also while the
    current stream is busy, so that the offsets are late), with `out` given, through TwoBitSet as well, in a process of its own:
    torch brings its own HIP runtime, which the rest of the suite keeps out of the test process"""
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import twobit_model as M
import kmer_model as K
import kmer_cases as KC
from bxmi import kmers, sequence

def dev_i32(a, pad):
    return torch.from_numpy(np.concatenate([[7] * pad, a]).astype(np.int32)).cuda()[pad:]

def same(got, want):
    got = got.cpu().numpy()
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)

seqs = M.structural_sequences()
model = K.Counts(seqs)
dev = [sequence.TwoBitTrack(s) for s in seqs]
side = torch.cuda.Stream()
busy = torch.zeros(1 << 27, dtype=torch.float32, device="cuda")
table = KC.TABLES["dna"][0]

track_of, starts, lengths = M.ragged_case()
ends = [s + n for s, n in zip(starts, lengths)]
clip = [(max(s, 0), max(min(e, seqs[t].size if 0 <= t < len(seqs) else 0) - max(s, 0), 0)) for t, s, e in zip(track_of, starts, ends)]
s_c, n_c = [c[0] for c in clip], [c[1] for c in clip]
d = [dev_i32(track_of, 1), dev_i32(starts, 3), dev_i32(ends, 1)]
for do_mask in (True, False):
    for k, drop_last in ((2, False), (3, True), (6, False)):
        want = model.counts(track_of, s_c, n_c, k, 4, table, do_mask, drop_last)
        assert want.sum() > 1000
        got = kmers.counts_dev(dev, *d, k, case_sensitive=False, do_mask=do_mask, drop_last=drop_last)
        torch.cuda.synchronize()
        assert got.is_cuda and same(got, want), (do_mask, k)
        got = kmers.counts_dev(dev, *d, k, case_sensitive=False, do_mask=do_mask, drop_last=drop_last, stream=side.cuda_stream)
        churn = [torch.zeros(len(track_of) + 1, dtype=torch.int64, device="cuda") for _ in range(4)]  # (what could take a freed block)
        side.synchronize()
        assert same(got, want), (do_mask, k, "side stream")
    # torch's current stream is busy when the offsets are queued behind it: the side stream must wait for them, on the device
    want = model.counts(track_of, s_c, n_c, 4, 4, table, do_mask)
    for _ in range(20):
        busy.add_(1)
    out = torch.full(want.shape, 77, dtype=torch.int32, device="cuda")
    res = kmers.counts_dev(dev, *d, 4, case_sensitive=False, do_mask=do_mask, stream=side.cuda_stream, out=out)
    side.synchronize()
    assert res is out and same(out, want), (do_mask, "out given, side stream, busy")
    with torch.cuda.stream(side):
        got = kmers.counts_dev(dev, *d, 4, {"A": 0, "G": 0, "C": 1, "T": 1}, do_mask=do_mask)
    side.synchronize()
    assert same(got, model.counts(track_of, s_c, n_c, 4, 2, KC.TABLES["ry"][0], do_mask))

for width in (37, K.TILE + 1):
    track_of_m, starts_m = M.matrix_case(width)
    want = model.counts(track_of_m, starts_m, [width] * len(starts_m), 3, 4, table, True)
    rows = [dev_i32(track_of_m, 1), dev_i32(starts_m, 2)]
    got = kmers.count_matrix_dev(dev, *rows, width, 3, case_sensitive=False, stream=side.cuda_stream)
    side.synchronize()
    assert same(got, want), width
    out = torch.full(want.shape, 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        res = kmers.count_matrix_dev(dev, *rows, width, 3, case_sensitive=False, out=out)
    side.synchronize()
    assert res is out and same(out, want), width
    got = kmers.count_matrix_dev(dev, *rows, width, 3, case_sensitive=False, drop_last=True)
    torch.cuda.synchronize()
    assert same(got, model.counts(track_of_m, starts_m, [width] * len(starts_m), 3, 4, table, True, True)), width
for bad in (torch.zeros(want.shape, dtype=torch.int64, device="cuda"), torch.zeros((3, 64), dtype=torch.int32, device="cuda")):
    try:
        kmers.count_matrix_dev(dev, *rows, width, 3, out=bad)
        raise SystemExit("a wrong `out` was accepted")
    except ValueError:
        pass

# through TwoBitSet; entries the device forms cannot refuse are rows of zeros
genome = sequence.TwoBitSet({"blocks": seqs[0], "odd": seqs[1]}, do_mask=True)
t2, s2, e2 = dev_i32(np.array([0, 1, 5, -1]), 0), dev_i32(np.array([100, 0, 3, 3]), 0), dev_i32(np.array([400, 41, 30, 30]), 0)
want = K.Counts(seqs[:2]).counts([0, 1, -1, -1], [100, 0, 0, 0], [300, 41, 0, 0], 2, 4, KC.TABLES["acgt"][0], True)
got = genome.kmer_counts_dev(t2, s2, e2, 2)
torch.cuda.synchronize()
assert same(got, want) and want[:2].any() and not want[2:].any()
got = genome.kmer_count_matrix_dev(t2, s2, 6, 2)
torch.cuda.synchronize()
assert same(got, K.Counts(seqs[:2]).counts([0, 1, -1, -1], [100, 0, 3, 3], [6] * 4, 2, 4, KC.TABLES["acgt"][0], True))
folded = kmers.fold_reverse_complement(got, 2)
assert folded.is_cuda and np.array_equal(folded.cpu().numpy(), kmers.fold_reverse_complement(got.cpu().numpy(), 2))
got = kmers.counts_dev(dev, d[0][:0], d[1][:0], d[2][:0], 3, stream=side.cuda_stream)
assert tuple(got.shape) == (0, 64)
genome.close()
for t in dev:
    t.close()
print("kmer dev ok")
'''
    p = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "bx-python_amd"), os.path.join(ROOT, "tests")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "kmer dev ok" in p.stdout, (p.stdout[-1000:], p.stderr[-3000:])


# ------------------------------------------------------------ the command line --
def test_command_line_prints_the_models_lines(tmp_path):
    from bxmi import kmers
    from bxmi.cli import twobit_kmer_counts as cli

    name = "multi.2bit"
    seqs = M.read(name)
    names = list(seqs)
    rows = [("ckpt", 990, 1030), ("odd", 0, 41), ("ckpt", 2565, 2600), ("empty", 0, 5), ("chrNone", 7, 9), ("odd", 38, 41), ("ckpt", 0, 2579)]
    bed = "# regions\n" + "".join("%s\t%d\t%d\n" % r for r in rows)
    track_of = [names.index(c) if c in names else -1 for c, _, _ in rows]
    model = K.Counts([seqs[n] for n in names])
    sizes = [seqs[n].size for n in names]
    s_c = [max(r[1], 0) for r in rows]
    n_c = [max(min(r[2], sizes[t] if t >= 0 else 0) - s, 0) for r, t, s in zip(rows, track_of, s_c)]
    for flags, do_mask, table in (([], True, "acgt"), (["-u"], False, "acgt"), (["-i"], True, "dna"), (["-c", "-i"], True, "dna")):
        want = model.counts(track_of, s_c, n_c, 2, 4, KC.TABLES[table][0], do_mask)
        labels = kmers.words(2)
        if "-c" in flags:
            keep = kmers.canonical_columns(2)
            want, labels = kmers.fold_reverse_complement(want, 2)[:, keep], [labels[i] for i in keep]
            assert want.shape[1] == 10 and want.sum() == model.counts(track_of, s_c, n_c, 2, 4, KC.TABLES[table][0], do_mask).sum()
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), "2"] + flags, stdin=io.StringIO(bed), out=out)
        text = "\t".join(["#chrom", "start", "end"] + labels) + "\n"
        text += "".join("\t".join([r[0], str(r[1]), str(r[2])] + [str(c) for c in line]) + "\n" for r, line in zip(rows, want.tolist()))
        assert out.getvalue() == text and want.any(), flags
        path = tmp_path / "out.npy"
        out = io.StringIO()
        cli.main([os.path.join(M.GOLDEN, name), "-o", str(path), "2"] + flags, stdin=io.StringIO(bed), out=out)
        assert out.getvalue() == "" and np.array_equal(np.load(path), want), flags
