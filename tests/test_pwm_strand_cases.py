"""CPU-only: the model of tests/pwm_strand_model.py agrees with a scalar transcription of the reference's loop on the string that the
strand contract of include/bxmi.h spells out letter by letter; the seeded cases of tests/pwm_strand_cases.py hold what they promise;
every stand-in "device" -- the model with one deliberate change a wrong kernel could make -- FAILS the case made for it; and the
reverse-complement matrix on the plus string, mirrored, is the minus plane bit for bit exactly where every partial sum is exact."""
import numpy as np
import pytest

import pwm_cases as PC
import pwm_hits_cases as H
import pwm_model as P
import pwm_strand_cases as C
import pwm_strand_model as PS
import strand_model as S
from test_pwm_cases import scalar_score


def strand_letter(letters, t, start, length, k, do_mask):
    """letter k of the string of a MINUS row by the contract as written: the complement of the letter at p = start + (length - 1 - k);
    0 (no column in any alphabet) where p is outside [0, size) or the row names no track"""
    if not 0 <= t < len(letters.seqs):
        return 0
    whole = letters.of(t, do_mask)
    p = start + (length - 1 - k)
    return int(S.COMPLEMENT[whole[p]]) if 0 <= p < len(whole) else 0


class Device:
    """the model as a device of pwm_strand_cases.check; `change`: one deliberate error
      descending      (a) the -r route: the same terms added in descending matrix row
      no_complement   (b) the row reversed, its letters not complemented
      halo_past_end   (c) the halo of a minus segment taken beyond the row's END, not before its start
      first_genomic   (d) of equal best scores the first GENOMIC offset: the last of the strand's string
      class_xor       (e) N or a masked letter complemented as a code: the letter CLASS ^ 2
      col_before      (f) letter_col applied before the complement: the plus letter's column, then mirrored as a reverse-complement
                          matrix mirrors its columns"""

    def __init__(self, change=None):
        self.change = change
        self.inner = PC.Model(descending=change == "descending", last_wins=change == "first_genomic")

    def texts(self, seqs, track_of, starts, lengths, strands, do_mask, extra=0):
        letters = PC.letters_of(seqs).letters
        minus = S.as_minus(strands, len(track_of))
        out = []
        for t, s, n, m in zip(track_of, starts, lengths, minus):
            t, s, n = int(t), int(s), int(n)
            row = letters.row(t, s, n, do_mask, 0)
            if not m:
                out.append(np.concatenate([row, np.zeros(extra, dtype=np.uint8)]))
            elif self.change == "no_complement":
                out.append(row[::-1])
            elif self.change == "class_xor":
                cls = np.array([P.LETTERS.find(chr(c)) for c in row[::-1]], dtype=np.int64)
                swapped = np.where(cls >= 0, cls ^ 2, -1)
                out.append(np.array([ord(P.LETTERS[c]) if 0 <= c < len(P.LETTERS) else 0 for c in swapped], dtype=np.uint8))
            elif extra:  # (halo_past_end: the letters beyond the row's end follow the strand's string)
                out.append(np.concatenate([S.reverse_complement(row), S.COMPLEMENT[letters.row(t, s + n, extra, do_mask, 0)]]))
            else:
                out.append(S.reverse_complement(row))
        return out

    def planes(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True):
        n = len(track_of)
        lengths = [width] * n if lengths is None else lengths
        strands = [0] * n if strands is None else strands
        if self.change == "col_before":
            mats = [self.mirrored(m) for m in mats]
        if self.change == "halo_past_end":
            extra = max(m.width for m in mats) - 1
            rows = self.texts(seqs, track_of, starts, lengths, strands, do_mask, extra)
            acc, ok, ext = self.inner.planes(seqs, mats, track_of, starts, [len(r) for r in rows], do_mask=do_mask, texts=rows)
            keep = np.concatenate([np.arange(a, a + int(k)) for a, k in zip(ext[:-1], lengths)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
            minus = np.repeat(S.as_minus(strands, n), np.asarray(lengths, dtype=np.int64))
            acc, ok = acc[:, keep], ok[:, keep]
            real = PS.MODEL.planes(seqs, mats, track_of, starts, strands, lengths, do_mask=do_mask)
            return np.where(minus, acc, real[0]), np.where(minus, ok, real[1]), real[2]
        rows = self.texts(seqs, track_of, starts, lengths, strands, do_mask)
        return self.inner.planes(seqs, mats, track_of, starts, lengths, do_mask=do_mask, texts=rows)

    @staticmethod
    def mirrored(mat):
        out = P.Matrix(mat.alphabet, mat.rows)
        there = mat.char_to_index[S.COMPLEMENT]  # the column of every letter's complement
        out.char_to_index = np.where(there >= 0, mat.values.shape[1] - 1 - there, -1).astype(np.int16)
        return out

    def scores(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, **_):
        acc, ok, _ = self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask)
        return np.where(ok, acc, P.NAN)

    def best(self, seqs, mats, track_of, starts, strands, lengths=None, width=0, do_mask=True, **_):
        return self.inner.best_of_planes(*self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask))

    def hits(self, seqs, mats, track_of, starts, strands, thresholds, lengths=None, width=0, do_mask=True, **_):
        acc, ok, offsets = self.planes(seqs, mats, track_of, starts, strands, lengths, width, do_mask)
        return H.expected(np.where(ok, acc, P.NAN), offsets, thresholds, ok)


def small_cases():
    return dict(short=C.short_rows_case(), boundary=C.boundary_case(), edges=C.edge_case(), matrix37=C.matrix_form_case(37), lanes=C.lane_case(),
                long=C.long_row_case(5), many=C.many_rows_case(), palindrome=C.palindrome_case(), extremes=C.extremes_case(), small_top=C.small_top_case(),
                **{name: C.set_case(name, 10 if name == "mats_max" else 30, 20_000, 400 if name == "mats_max" else 1500) for name in C.SETS})


@pytest.mark.parametrize("name", ["short", "boundary", "edges", "matrix37", "lanes", "long", "many", "palindrome", "extremes", "small_top"] + list(C.SETS))
def test_model_is_the_scalar_loop_on_the_contracts_string(name):
    """the model's planes against the reference's loop, one float32 at a time, over letters taken position by position as the
    contract states them, on sampled offsets of minus rows; and the model passes its own case as a device"""
    case = small_cases()[name]
    lengths, width, n = C.rows_of(case)
    lengths = [width] * n if lengths is None else lengths
    offsets = H.offsets_of(lengths)
    letters = PC.letters_of(case["seqs"]).letters
    rng = np.random.default_rng(650)
    for do_mask in case.get("do_masks", (True, False)):
        acc, ok, _, _, _ = C.want_of(case, do_mask)
        got = np.where(ok, acc, P.NAN)
        minus_rows = [i for i in range(n) if case["strands"][i] and lengths[i] > 0]
        checked = 0
        for _ in range(400):
            i = minus_rows[int(rng.integers(len(minus_rows)))]
            m = int(rng.integers(len(case["mats"])))
            j = int(rng.integers(lengths[i]))
            mat = case["mats"][m]
            text = [strand_letter(letters, int(case["track_of"][i]), int(case["starts"][i]), int(lengths[i]), k, do_mask)
                    for k in range(j, min(j + mat.width, int(lengths[i])))]
            want = scalar_score(mat, [0] * j + text, j) if j + mat.width <= lengths[i] else P.NAN
            e = int(offsets[i]) + j
            assert P.bits(got[m, e]) == P.bits(want) or (np.isnan(got[m, e]) and np.isnan(want) and P.bits(want) != P.NAN_BITS), (name, do_mask, i, m, j)
            checked += not np.isnan(want)
        assert checked > 0, name
    C.check([Device()], case)


def test_cases_are_what_their_names_say():
    short = C.short_rows_case()
    for w in (1, 4, 20, P.WIDTH_MAX):
        assert {w - 1, w, w + 1} <= {n for n, m in zip(short["lengths"], short["strands"]) if m}
    assert {0, 1, 15, 16, 17, 33} <= set(short["lengths"])
    b = C.boundary_case()
    t, s, n, m = b["track_of"], b["starts"], b["lengths"], b["strands"]
    assert any(a < 0 and k for a, k in zip(s, m)) and any(q == -1 and k for q, k in zip(t, m))       # a minus row below 0; one without a track
    size = b["seqs"][0].size
    assert any(q == 0 and a + c > size and k for q, a, c, k in zip(t, s, n, m))                        # one reaching past the size
    assert m[:6] == [1, 0, 1, 0, 1, 0] and sum(n) % 4 == 1
    # the first W - 1 GENOMIC positions of a minus row are its unscoreable tail, and the letters below its start are not read:
    # the three-tile row starts at 4000, where the sequence has plain bases on both sides
    acc, ok, offsets, _, _ = C.want_of(b, False)
    three = b["cross"] + 1
    assert n[three] == 2 * P.TILE + 300 and m[three] == 1
    widest = [k for k, mat in enumerate(b["mats"]) if mat.width == P.WIDTH_MAX][0]
    row = ok[widest, offsets[three]:offsets[three + 1]]
    assert row[:n[three] - P.WIDTH_MAX + 1].any() and not row[n[three] - P.WIDTH_MAX + 1:].any()
    many = C.many_rows_case()
    assert len(many["strands"]) == 2500 and sum(many["lengths"]) <= P.TILE and 0 < sum(many["strands"]) < 2500
    for name in C.SETS:
        case = C.set_case(name, 10 if name == "mats_max" else 30, 20_000, 400 if name == "mats_max" else 1500)
        assert 0 < sum(case["strands"]) < len(case["strands"])
    assert sum(mat.width for mat in C.set_case("lds_plus_4")["mats"]) * 4 > PC.LDS_VALUES and len(C.set_case("mats_max", 10, 20_000, 400)["mats"]) == P.MATS_MAX


STAND_INS = {
    "descending": ("lds_plus_4", "mats_max", "cols16_g_top"),
    "no_complement": ("short", "boundary", "palindrome"),
    "halo_past_end": ("boundary", "short", "small_top"),
    "first_genomic": ("lanes", "long"),
    "class_xor": ("edges", "cols16_mixed"),  # (under an upper-case alphabet every such letter lacks a column either way)
    "col_before": ("cols16_mixed", "matrix37", "lds_256x16"),
}


@pytest.mark.parametrize("change", sorted(STAND_INS))
def test_a_changed_device_fails_its_cases(change):
    cases = small_cases()
    for name in STAND_INS[change]:
        with pytest.raises(AssertionError):
            C.check([Device(change)], cases[name])


def test_column_mirroring_is_right_only_for_closed_alphabets():
    """(f) again: on ACGT the plus letter's column mirrored IS the complement's column, so only alphabets that are not closed under
    complement can tell"""
    C.check([Device("col_before")], C.short_rows_case())


def mirrored_minus_r(mat, row):
    """the route a user had before strand: the reverse-complement matrix on the PLUS string, element j <-> len - W - j"""
    plane = mat.reverse_complement().score(row)
    out = np.full(len(row), P.NAN, dtype=np.float32)
    k = len(row) - mat.width + 1
    if k > 0:
        out[:k] = plane[:k][::-1]
    return out


def test_minus_r_on_the_plus_string_is_the_same_only_where_sums_are_exact():
    rng = np.random.default_rng(660)
    case = C.set_case("lds_plus_4")
    seqs = case["seqs"]
    rows = [r for r in PC.letters_of(seqs).rows(case["track_of"], case["starts"], case["lengths"], False) if len(r) > 300][:6]
    whole = [P.Matrix("ACGT", rng.integers(-8, 9, (w, 4)).astype(np.float32)) for w in (3, 20, 256)]  # every partial sum an integer below 2^24
    same = differ = scored = 0
    for row in rows:
        for mat in whole:
            minus, route = PS.score(mat, row, True), mirrored_minus_r(mat, row)
            assert np.array_equal(P.bits(minus), P.bits(route))
            same += int((~np.isnan(minus)).sum())
        for mat in case["mats"][:3]:  # the seeded random matrices of mixed magnitudes, 256 rows each
            minus, route = PS.score(mat, row, True), mirrored_minus_r(mat, row)
            assert np.array_equal(np.isnan(minus), np.isnan(route))
            differ += int((P.bits(minus) != P.bits(route)).sum())
            scored += int((~np.isnan(minus)).sum())
    assert same > 1000 and scored > 1000 and differ >= scored // 4, (same, differ, scored)
    # (a) is that route: descending order on the strand's string is the reverse-complement matrix's ascending order on the plus string
    mat, row = case["mats"][0], rows[0]
    down, ok = PC.chain(mat.values, mat.char_to_index, S.reverse_complement(row), descending=True)
    assert np.array_equal(P.bits(np.where(ok, down, P.NAN)), P.bits(mirrored_minus_r(mat, row)))
