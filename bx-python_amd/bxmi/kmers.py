"""
The k-mer spectrum of the sequence of .2bit files on the MI355X: ``bx.intseq.ngramcount.count_ngrams`` (reference:
lib/bx/intseq/ngramcount.pyx:34-85) fed by ``bx.seqmapping`` (lib/bx/seqmapping.py:36-48 over ``CharToIntArrayMapping.translate``,
lib/bx/_seqmapping.pyx:24-67) for a whole array of regions per call, read straight from the packed bases
(``bxmi_twobit_kmer_counts*`` of include/bxmi.h; kernel: csrc/kmer.hpp).  In the reference's terms, per region,
``count_ngrams(mapping.translate(twobit[chrom].get(start, end)), k, radix)``.

``counts`` gives int32 [n, radix ** k]: how often each word of ``k`` letters occurs in every region, ``count_matrix`` the same for
windows of one width.  A word's column is ``sum(digit[t] * radix ** t)``, its FIRST letter least significant, as the reference's.
The ``alphabet`` says which letters have a digit: a string gives the digit order (``"ACGT"``: A=0, C=1, G=2, T=3, what
``bx.seqmapping.DNA`` gives them), a mapping letter -> digit is the general case and may put several letters on one digit
(``{"A": 0, "G": 0, "C": 1, "T": 1}``: purine/pyrimidine words, radix 2).  A window over a letter without a digit -- an N, with a
case-sensitive alphabet of upper-case letters also a soft-masked base -- is not counted.  ``case_sensitive=False`` gives lower case
the digit of upper case, as ``bx.seqmapping.DNA`` does.  Every window of a region is counted; the reference's loop stops one
window early (ngramcount.pyx:71), and ``drop_last=True`` reproduces that by shortening every region by one base.  The work is
integer: the counts are the reference's bit for bit.  The ``_dev`` forms take and return torch tensors on the caller's stream.

``strands`` (None: all plus; given as for ``bxmi.sequence``) counts the minus regions over their reverse complement, the string
``sequence.strings(..., strands=...)`` gives: the digits of the complemented letters in reverse order, under ANY alphabet.  With
``drop_last`` the last window of the STRAND's string is dropped, so a minus region is shortened at its start.

``index_of`` / ``word_of`` / ``words`` name the columns; ``fold_reverse_complement`` collapses the two strands;
``strand_columns`` gives, for an alphabet closed under complement, the column of every column's reverse-complement word.
"""
import numpy as np

from . import _ffi
from ._ffi import as_i32, call, ptr
from .sequence import _clip, _clip_dev, _record, _strands, _strands_dev
from .summary import _rows_i32

BINS_MAX = 16384          # KM_BINS_MAX of csrc/kmer.hpp
LETTERS = "TCAGtcag"      # the eight letters that can have a digit, in the order of the digits table: 4 * lower_case + code
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
_COMPLEMENT.update({a.lower(): b.lower() for a, b in list(_COMPLEMENT.items())})


def _letter_digits(alphabet):
    """{letter: digit} of an alphabet as given, and the letter that names each digit"""
    if isinstance(alphabet, str):
        if len(set(alphabet)) != len(alphabet):
            raise ValueError("the letters of an alphabet string must be distinct")
        given = {ch: d for d, ch in enumerate(alphabet)}
    else:
        given = {ch: int(d) for ch, d in dict(alphabet).items()}
    for ch, d in given.items():
        if ch in ("N", "n"):
            raise ValueError("N has no digit: an alphabet cannot give %r one" % ch)
        if not isinstance(ch, str) or len(ch) != 1 or ch not in LETTERS:
            raise ValueError("an alphabet holds letters of %s, not %r" % (LETTERS, ch))
        if d < 0:
            raise ValueError("the digit of %r is negative" % ch)
    if not given:
        raise ValueError("an alphabet holds at least one letter")
    return given


def digits_of(alphabet="ACGT", case_sensitive=True):
    """(int8 [8], radix): the digit of every letter of LETTERS, -1 for none, as bxmi_twobit_kmer_counts takes it; radix is the
    greatest digit + 1, at least 2, at most 4"""
    given = _letter_digits(alphabet)
    if not case_sensitive:  # lower case takes the digit of upper case
        given = {ch: d for ch, d in given.items() if ch.isupper()}
        given.update({ch.lower(): d for ch, d in list(given.items())})
    radix = max(max(given.values(), default=0) + 1, 2)
    if radix > 4:
        raise ValueError("radix %d: a digit is at most 3" % radix)
    table = np.array([given.get(ch, -1) for ch in LETTERS], dtype=np.int8)
    return table, radix


def _names(alphabet):
    """[the letter that names digit d] for an alphabet: the first letter given that digit"""
    given = _letter_digits(alphabet)
    radix = max(max(given.values()) + 1, 2)
    names = [None] * radix
    for ch, d in given.items():
        if d < radix and names[d] is None:
            names[d] = ch
    return names, given, radix


def bins_of(k, radix):
    k = int(k)
    if k < 1:
        raise ValueError("k = %d, must be at least 1" % k)
    if radix ** k > BINS_MAX:
        raise ValueError("%d ** %d words are more than the %d a call counts" % (radix, k, BINS_MAX))
    return radix ** k


def index_of(word, alphabet="ACGT"):
    """the column of a word: sum(digit[t] * radix ** t), the first letter least significant"""
    _, given, radix = _names(alphabet)
    index = 0
    for t, ch in enumerate(word):
        if ch not in given:
            raise ValueError("%r has no digit in this alphabet" % ch)
        index += given[ch] * radix ** t
    return index


def word_of(index, k, alphabet="ACGT"):
    """the word of a column; a digit several letters share is named by the first of them"""
    names, _, radix = _names(alphabet)
    index = int(index)
    if not 0 <= index < radix ** int(k):
        raise ValueError("index %d outside [0, %d ** %d)" % (index, radix, k))
    out = []
    for _ in range(int(k)):
        index, d = divmod(index, radix)
        if names[d] is None:
            raise ValueError("no letter of this alphabet has digit %d" % d)
        out.append(names[d])
    return "".join(out)


def words(k, alphabet="ACGT"):
    """the column labels: [word_of(i, k, alphabet) for every column i]"""
    names, _, radix = _names(alphabet)
    if None in names:
        raise ValueError("no letter of this alphabet has digit %d" % names.index(None))
    out = [""]
    for _ in range(int(k)):  # (a later letter is a more significant digit: it varies more slowly)
        out = [rest + ch for ch in names for rest in out]
    bins_of(k, radix)
    return out


def reverse_complement_columns(k, alphabet="ACGT"):
    """int64 [4 ** k]: the column of every column's reverse-complement word; radix 4 over A, C, G, T only"""
    names, given, radix = _names(alphabet)
    if radix != 4 or sorted(names, key=str) != ["A", "C", "G", "T"] or len(given) != 4:
        raise ValueError("the strands are folded for an alphabet of exactly A, C, G and T")
    comp = np.array([given[_COMPLEMENT[names[d]]] for d in range(4)], dtype=np.int64)
    k = int(k)
    index = np.arange(bins_of(k, 4), dtype=np.int64)
    out = np.zeros_like(index)
    for t in range(k):  # letter t of the word becomes letter k - 1 - t of its reverse complement
        out += comp[(index // 4 ** t) % 4] * 4 ** (k - 1 - t)
    return out


def strand_columns(k, alphabet="ACGT", case_sensitive=True):
    """int64 [radix ** k]: w -> index_of(reverse_complement(word_of(w))), for an alphabet closed under complement -- the
    complements of the letters of one digit all have one digit, and every digit is some letter's.  Then the counts of the minus
    strand are a gather of the plus strand's: minus[:, strand_columns(k)[w]] == plus[:, w], that is, minus == plus[:, rc] with rc
    its own inverse.  An alphabet that is not closed (a letter whose complement has no digit, or another one than its digit-mates')
    is a ValueError: no permutation of the columns gives its minus counts."""
    digits, radix = digits_of(alphabet, case_sensitive)
    comp = {}
    for ch, d in zip(LETTERS, digits.tolist()):
        if d < 0:
            continue
        c = int(digits[LETTERS.index(_COMPLEMENT[ch])])
        if c < 0 or comp.setdefault(d, c) != c:
            raise ValueError("the alphabet is not closed under complement at %r" % ch)
    if sorted(comp) != list(range(radix)):
        raise ValueError("no letter of this alphabet has digit %d" % min(set(range(radix)) - set(comp)))
    table = np.array([comp[d] for d in range(radix)], dtype=np.int64)
    k = int(k)
    index = np.arange(bins_of(k, radix), dtype=np.int64)
    out = np.zeros_like(index)
    for t in range(k):  # letter t of the word becomes letter k - 1 - t of its reverse complement
        out += table[(index // radix ** t) % radix] * radix ** (k - 1 - t)
    return out


def canonical_columns(k, alphabet="ACGT"):
    """the columns `fold_reverse_complement` keeps: those not above their reverse complement's"""
    rc = reverse_complement_columns(k, alphabet)
    return np.flatnonzero(np.arange(len(rc)) <= rc)


def fold_reverse_complement(counts, k, alphabet="ACGT"):
    """The strand-collapsed spectrum of `counts` [..., 4 ** k] (numpy or torch): the columns of a word and of its reverse complement
    are added into the smaller index of the two and the larger one is zero; a palindrome is kept once.  A new array of the same
    shape."""
    rc = reverse_complement_columns(k, alphabet)
    if counts.shape[-1] != len(rc):
        raise ValueError("counts has %d columns, 4 ** %d = %d words" % (counts.shape[-1], k, len(rc)))
    above = np.flatnonzero(rc < np.arange(len(rc)))  # (their partners are distinct: the map is an involution)
    if isinstance(counts, np.ndarray):
        out = counts.copy()
        out[..., rc[above]] += counts[..., above]
        out[..., above] = 0
        return out
    import torch

    out = counts.clone()
    hi, lo = torch.as_tensor(above, device=counts.device), torch.as_tensor(rc[above], device=counts.device)
    out[..., lo] += counts[..., hi]
    out[..., hi] = 0
    return out


def _offsets(lengths, drop_last):
    if drop_last:
        lengths = np.maximum(lengths - 1, 0)
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return offsets


def counts(tracks, track_of, starts, ends, k, alphabet="ACGT", case_sensitive=True, do_mask=True, drop_last=False, strands=None):
    """The words of regions [starts[i], ends[i]) of tracks[track_of[i]], clipped as `sequence.sequences` clips them -> int32
    [n, radix ** k].  An empty region, one shorter than k, or one on an unknown sequence gives zeros.  With drop_last every region
    loses its last base first: then row i equals the reference's count_ngrams(mapping.translate(seq.get(start, end)), k, radix)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s, e = _rows_i32("track_of, starts and ends", track_of, starts, ends)
    digits, radix = digits_of(alphabet, case_sensitive)
    bins = bins_of(k, radix)
    s64, lengths = _clip([tr.size for tr in tracks], t, s, e)
    offsets = _offsets(lengths, drop_last)
    out = np.empty((len(t), bins), dtype=np.int32)
    strand = _strands(strands, len(t))
    if strand is None:
        call("bxmi_twobit_kmer_counts", _ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), len(t), 0, ptr(offsets), int(offsets[-1]),
             int(bool(do_mask)), int(k), radix, ptr(digits), ptr(out))
        return out
    if drop_last:  # the last window of a minus region's string lies at the region's start
        s64 = s64 + ((strand != 0) & (lengths > 0))
    call("bxmi_twobit_kmer_counts_strand", _ffi.handles(tracks), len(tracks), ptr(t), ptr(as_i32(s64)), ptr(strand), len(t), 0, ptr(offsets),
         int(offsets[-1]), int(bool(do_mask)), int(k), radix, ptr(digits), ptr(out))
    return out


def count_matrix(tracks, track_of, starts, width, k, alphabet="ACGT", case_sensitive=True, do_mask=True, drop_last=False, strands=None):
    """The words of windows [starts[i], starts[i] + width) of tracks[track_of[i]] -> int32 [n, radix ** k]; a position outside the
    sequence has no digit, as has every position of a row that names no track.  width < 1 raises BxmiError (EINVAL)."""
    _ffi.require_gpu()
    tracks = list(tracks)
    t, s = _rows_i32("track_of and starts", track_of, starts)
    digits, radix = digits_of(alphabet, case_sensitive)
    bins = bins_of(k, radix)
    width = int(width)
    strand = _strands(strands, len(t))
    if drop_last and width == 1:  # (nothing is left of a window of one base)
        return np.zeros((len(t), bins), dtype=np.int32)
    shorter = drop_last and width > 1
    width -= 1 if shorter else 0
    out = np.empty((len(t), bins), dtype=np.int32)
    if strand is None:
        call("bxmi_twobit_kmer_counts", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), len(t), width, None, len(t) * max(width, 0),
             int(bool(do_mask)), int(k), radix, ptr(digits), ptr(out))
        return out
    if shorter:  # the last window of a minus row's string lies at the window's start
        s = as_i32(s.astype(np.int64) + (strand != 0))
    call("bxmi_twobit_kmer_counts_strand", _ffi.handles(tracks), len(tracks), ptr(t), ptr(s), ptr(strand), len(t), width, None, len(t) * max(width, 0),
         int(bool(do_mask)), int(k), radix, ptr(digits), ptr(out))
    return out


def _out_dev(out, n, bins, dev):
    """(`out` or a new int32 [n, bins] tensor, the tensors made here)"""
    import torch

    if out is None:
        out = torch.empty((n, bins), dtype=torch.int32, device=dev)
        return out, (out,)
    if out.dtype != torch.int32 or tuple(out.shape) != (n, bins) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous int32 [n, radix ** k] tensor on the device of the rows")
    return out, ()


def counts_dev(tracks, track_of, starts, ends, k, alphabet="ACGT", case_sensitive=True, do_mask=True, drop_last=False, stream=None, out=None,
               strands=None):
    """`counts` on device arrays: int32 torch tensors on the GPU in, the int32 [n, radix ** k] tensor out -- `out` if given
    (contiguous, on the rows' device), else a new one -- queued on torch's current stream (or `stream`).  The clipping and the
    offsets are torch's, on its current stream, and the host waits for NOTHING and reads nothing back: the kernel reads where the
    rows end from the offsets themselves and is given only a bound of it, n times the longest sequence.  When `stream` is not
    torch's current stream it is made to wait, on the device, for what the current stream has queued up to the offsets; the
    tensors made here are recorded as in use on it.  One 2bit call at a time, as `sequence.matrix_dev`."""
    import torch

    tracks = list(tracks)
    (track_of, starts, ends), n, dev, stream = _ffi.device_args("counts_dev", "counts", ("track_of", "starts", "ends"), (track_of, starts, ends), stream)
    digits, radix = digits_of(alphabet, case_sensitive)
    bins = bins_of(k, radix)
    first, offsets = _clip_dev(tracks, track_of, starts, ends, n, dev)
    strand = _strands_dev(strands, n, dev, "counts_dev")
    if drop_last and n:
        if strand is not None:  # the last window of a minus region's string lies at the region's start
            first = first + ((strand != 0) & (offsets[1:] > offsets[:-1])).to(first.dtype)
        torch.cumsum((offsets[1:] - offsets[:-1] - 1).clamp_(min=0), 0, out=offsets[1:])
    if stream != torch.cuda.current_stream(dev).cuda_stream:  # the kernel reads what torch's current stream is still writing
        torch.cuda.ExternalStream(stream, device=dev).wait_stream(torch.cuda.current_stream(dev))
    out, made = _out_dev(out, n, bins, dev)
    bound = n * max([tr.size for tr in tracks] + [0])
    if strand is None:
        call("bxmi_twobit_kmer_counts_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), n, 0, offsets.data_ptr(), bound,
             int(bool(do_mask)), int(k), radix, ptr(digits), out.data_ptr(), stream)
    else:
        call("bxmi_twobit_kmer_counts_strand_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), first.data_ptr(), strand.data_ptr(), n, 0,
             offsets.data_ptr(), bound, int(bool(do_mask)), int(k), radix, ptr(digits), out.data_ptr(), stream)
        made = made + ((strand,) if strand is not strands else ())
    if n:
        _record(stream, dev, (first, offsets) + made)
    return out


def count_matrix_dev(tracks, track_of, starts, width, k, alphabet="ACGT", case_sensitive=True, do_mask=True, drop_last=False, stream=None, out=None,
                     strands=None):
    """`count_matrix` on device arrays: the int32 [n, radix ** k] tensor (`out` if given), queued on torch's current stream (or
    `stream`), nothing is waited for."""
    tracks = list(tracks)
    (track_of, starts), n, dev, stream = _ffi.device_args("count_matrix_dev", "count_matrix", ("track_of", "starts"), (track_of, starts), stream)
    digits, radix = digits_of(alphabet, case_sensitive)
    bins = bins_of(k, radix)
    width = int(width)
    out, made = _out_dev(out, n, bins, dev)
    strand = _strands_dev(strands, n, dev, "count_matrix_dev")
    if drop_last and width == 1:
        return out.zero_()
    shorter = drop_last and width > 1
    width -= 1 if shorter else 0
    if strand is None:
        call("bxmi_twobit_kmer_counts_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), n, width, None, n * max(width, 0),
             int(bool(do_mask)), int(k), radix, ptr(digits), out.data_ptr(), stream)
    else:
        if shorter:  # the last window of a minus row's string lies at the window's start (torch's current stream, as counts_dev's offsets)
            import torch

            starts = starts + (strand != 0).to(starts.dtype)
            made = made + (starts,)
            if stream != torch.cuda.current_stream(dev).cuda_stream:
                torch.cuda.ExternalStream(stream, device=dev).wait_stream(torch.cuda.current_stream(dev))
        call("bxmi_twobit_kmer_counts_strand_dev", _ffi.handles(tracks), len(tracks), track_of.data_ptr(), starts.data_ptr(), strand.data_ptr(), n, width,
             None, n * max(width, 0), int(bool(do_mask)), int(k), radix, ptr(digits), out.data_ptr(), stream)
        made = made + ((strand,) if strand is not strands else ())
    if made and n:
        _record(stream, dev, made)
    return out
