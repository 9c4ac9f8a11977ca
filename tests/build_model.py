"""A numpy statement of the contract of bxmi_twobit_create_letters / _create_nib (include/bxmi.h): letters or nibbles -> the packed
bytes, the N blocks and the mask blocks of the 2bit track, and the lowest position of a symbol that is none of TCAGNtcagn.  The
rule is the one real files follow (tests/test_build_model_golden.py): maximal runs, code 0 under N, zero bits behind the last base."""
import collections

import numpy as np

from bxmi import twobit

TILE = 4096  # positions per workgroup of csrc/twobit_build.hpp (tests/test_build_abi.py checks it against its text)

# per ASCII byte: the code, N, lower case, other
_CODE = np.zeros(256, dtype=np.uint8)
_IS_N = np.ones(256, dtype=bool)
_LOWER = np.zeros(256, dtype=bool)
_OTHER = np.ones(256, dtype=bool)
for _code, _ch in enumerate("TCAG"):
    for _c in (_ch, _ch.lower()):
        _CODE[ord(_c)], _IS_N[ord(_c)], _OTHER[ord(_c)] = _code, False, False
_OTHER[[ord("N"), ord("n")]] = False
_LOWER[ord("a"):ord("z") + 1] = True

Built = collections.namedtuple("Built", "seq first_other other_value")


def runs(flag):
    """(starts, sizes) of the maximal runs of True"""
    edge = np.diff(np.concatenate([[0], flag.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    return starts.astype(np.uint32), (ends - starts).astype(np.uint32)


def _built(code, is_n, lower, other, values):
    size = len(code)
    code = np.where(is_n, 0, code).astype(np.uint8)
    padded = np.zeros((size + 3) // 4 * 4, dtype=np.uint8)
    padded[:size] = code
    quads = padded.reshape(-1, 4)
    packed = (quads[:, 0] << 6 | quads[:, 1] << 4 | quads[:, 2] << 2 | quads[:, 3]).astype(np.uint8)
    at = np.flatnonzero(other)
    first = int(at[0]) if len(at) else None
    return Built(twobit.Sequence(size, *runs(is_n), *runs(lower), packed), first, int(values[first]) if first is not None else None)


def as_letters(letters):
    if isinstance(letters, str):
        letters = letters.encode("latin-1")
    if isinstance(letters, (bytes, bytearray)):
        return np.frombuffer(bytes(letters), dtype=np.uint8)
    return np.asarray(letters, dtype=np.uint8)


def from_letters(letters):
    """Built of ASCII letters under other="N"; first_other (None without one) is what other="error" reports"""
    a = as_letters(letters)
    return _built(_CODE[a], _IS_N[a], _LOWER[a], _OTHER[a], a)


def nibbles_of(nibble_bytes, size):
    b = np.asarray(nibble_bytes, dtype=np.uint8)
    return np.stack([b >> 4, b & 15], axis=1).reshape(-1)[:size]


def from_nib(nibble_bytes, size):
    v = nibbles_of(nibble_bytes, size)
    c = v & 7
    return _built(np.where(c < 4, c, 0), c >= 4, (v & 8) != 0, c > 4, v)  # (other_value: the whole nibble)


def to_nib(letters):
    """the nibble bytes of a string over TCAGNtcagn (the reverse of the reference's _nib.pyx table), the last low nibble 0"""
    a = as_letters(letters)
    table = np.full(256, 255, dtype=np.uint8)
    for code, ch in enumerate("TCAGN"):
        table[ord(ch)], table[ord(ch.lower())] = code, code | 8
    v = table[a]
    assert (v != 255).all()
    v = np.concatenate([v, np.zeros(len(v) & 1, dtype=np.uint8)])
    return (v[0::2] << 4 | v[1::2]).astype(np.uint8)


def same_arrays(got, want):
    """what two twobit.Sequence must agree in"""
    return (int(got.size) == int(want.size) and all(np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(w, dtype=np.int64))
                                                     for g, w in zip(got[1:5], want[1:5]))
            and np.array_equal(np.asarray(got.packed, dtype=np.uint8)[:(want.size + 3) // 4], np.asarray(want.packed, dtype=np.uint8)))
