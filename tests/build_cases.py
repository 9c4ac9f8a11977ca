"""Seeded cases for the builders of 2bit tracks from letters (csrc/twobit_build.hpp), shared by the kernels compiled for the host
(tests/test_build_kernel_host.py) and the device (tests/test_gpu_build.py).  Every case is a few thousand letters: T is the
builder's tile, 16 a thread's share of it, 1024 a wave's.  The expected arrays come from tests/build_model.py."""
import numpy as np

import build_model as B

T = B.TILE
THREAD, WAVE = 16, 1024
SCAN_TILE = 2048  # of csrc/primitives.hpp: entries per workgroup of the device scan
SIZES = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T + 1)
BOUNDS = (THREAD, 3 * THREAD, WAVE, 3 * WAVE, T, 2 * T)  # thread, wave and tile boundaries, the first and a later one of each
TEN = np.frombuffer(b"TCAGNtcagn", dtype=np.uint8)
RANDOM_SEEDS = (411, 412, 413)


def plain(rng, size):
    """upper-case ACGT"""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=size)].copy()


def plant(a, kind, lo, hi):
    """[lo, hi) of `a` becomes N ("N"), lower case ("mask") or n ("n")"""
    if kind in ("N", "n"):
        a[lo:hi] = ord("N")
    if kind in ("mask", "n"):
        a[lo:hi] |= 0x20


def random_ten(rng, size):
    """letters over all ten, in runs of 1 to about 40 of one kind so that blocks of every short length occur"""
    out = plain(rng, size)
    at = 0
    while at < size:
        step = int(rng.integers(1, 41))
        kind = ("", "", "N", "mask", "n")[int(rng.integers(0, 5))]
        if kind:
            plant(out, kind, at, min(at + step, size))
        at += step
    return out


# how a run lies at a boundary b: [b + lo, b + hi)
SHAPES = {"ends_at": (-5, 0), "starts_at": (0, 5), "straddles_by_one_before": (-1, 3), "straddles_by_one_after": (-3, 1), "one_base_each_side": (-1, 1)}


def letter_cases():
    """[(name, uint8 letters)]: none holds a symbol outside the ten letters"""
    rng = np.random.default_rng(410)
    cases = [("size_%d" % size, random_ten(rng, size)) for size in SIZES]
    for shape, (lo, hi) in SHAPES.items():
        for kind in ("N", "mask", "n"):
            a = plain(rng, 3 * T)
            for b in BOUNDS:
                plant(a, kind, b + lo, b + hi)
            cases.append(("%s_%s" % (shape, kind), a))
    for kind in ("N", "mask", "n"):
        a = plain(rng, 2 * T + 33)
        plant(a, kind, 0, 3)                 # a run at position 0
        plant(a, kind, len(a) - 4, len(a))   # a run that ends at size
        for p in (7, 15, 16, 31, 32, 1023, 1024, T - 1, T, 2 * T + 30):  # runs of length 1, at the edges of threads, waves and tiles too
            plant(a, kind, p, p + 1)
        cases.append(("ends_and_single_%s" % kind, a))
        a = plain(rng, 3 * T + 100)
        plant(a, kind, T - 7, 2 * T + 9)     # one run over three tiles
        cases.append(("three_tiles_%s" % kind, a))
        a = plain(rng, T + 17)
        plant(a, kind, 0, len(a))
        cases.append(("all_%s" % kind, a))
    a = plain(rng, 200)
    plant(a, "mask", 10, 60)
    plant(a, "n", 10, 13)      # n at the edges of lower case, and inside it
    plant(a, "n", 30, 34)
    plant(a, "n", 57, 60)
    plant(a, "mask", 100, 150)
    plant(a, "N", 98, 103)     # upper-case N before, inside and behind lower case: the mask run is cut, the N run is not
    plant(a, "N", 120, 122)
    plant(a, "N", 148, 153)
    plant(a, "n", 160, 170)    # n with upper case around it
    cases.append(("n_inside_lower_case", a))
    for kind in ("N", "mask", "n"):  # every second base: size / 2 blocks, the most a tile can hold, through two tiles and more than two scan tiles
        a = plain(rng, 2 * T + 1)
        a[0::2] = np.where(kind == "mask", a[0::2] | 0x20, ord("N") | (0x20 if kind == "n" else 0)).astype(np.uint8)
        assert (len(a) + 1) // 2 > 2 * SCAN_TILE
        cases.append(("every_second_%s" % kind, a))
    for seed in RANDOM_SEEDS:
        r = np.random.default_rng(seed)
        cases.append(("random_%d" % seed, TEN[r.integers(0, 10, size=2 * T + 1 + seed % 7)].copy()))
    return cases


def other_cases():
    """[(name, uint8 letters)]: each holds symbols outside the ten letters; the model names the lowest"""
    rng = np.random.default_rng(420)
    cases = []
    a = random_ten(rng, 3 * T + 5)
    for p, v in ((2 * T + 77, ord("R")), (T + 3, ord("y")), (T + 2000, 0x00), (len(a) - 1, 0xFF)):  # several, in different tiles: the lowest is y's
        a[p] = v
    cases.append(("several_tiles", a))
    a = random_ten(rng, T + 9)
    a[-1] = ord("X")
    cases.append(("last_position", a))
    a = random_ten(rng, 70)
    a[0] = 0x00
    cases.append(("byte_00_first", a))
    a = random_ten(rng, 70)
    a[33] = 0xFF
    cases.append(("byte_FF", a))
    a = plain(rng, 100)
    a[10:14] = np.frombuffer(b"RYrk", dtype=np.uint8)      # IUPAC, upper and lower case, next to each other
    a[20:23] = np.frombuffer(b"aWc", dtype=np.uint8)       # an upper-case one that cuts a mask run
    a[30:33] = np.frombuffer(b"NmN", dtype=np.uint8)       # a lower-case one inside an N run
    a[40:44] = np.frombuffer(b"-*. ", dtype=np.uint8)      # what is no letter at all
    a[50:52] = np.frombuffer(b"@[", dtype=np.uint8)        # the bytes around A-Z
    a[52:54] = np.frombuffer(b"`{", dtype=np.uint8)        # ... and around a-z: not lower case
    a[60] = ord("T") | 0x80                                # (bit 7 must not be ignored)
    cases.append(("iupac", a))
    return cases


def nib_cases():
    """[(name, nibble bytes, size)]: the letter cases as nibbles (a few of them), and nibbles as they are"""
    cases = []
    for name, a in letter_cases():
        if name.startswith(("size_", "random_", "ends_and_single_", "every_second_n", "three_tiles_n", "one_base_each_side_")) or name == "n_inside_lower_case":
            cases.append((name, B.to_nib(a), len(a)))
    return cases


def nib_other_cases():
    rng = np.random.default_rng(430)
    cases = []
    v = rng.integers(0, 16, size=2 * T + 3).astype(np.uint8)  # every nibble value: codes 5-7 with and without the mask bit
    cases.append(("every_value", v, len(v)))
    v = B.nibbles_of(B.to_nib(random_ten(rng, T + 6)), T + 6).copy()
    v[T + 5] = 7
    cases.append(("code_7_last", v, len(v)))
    v = B.nibbles_of(B.to_nib(random_ten(rng, 3 * T)), 3 * T).copy()
    v[2 * T + 1], v[T - 1], v[T + 500] = 5, 0xE, 0xD  # in different tiles: the lowest is the masked 6
    cases.append(("several_tiles", v, len(v)))
    out = []
    for name, v, size in cases:
        v = np.concatenate([v, np.zeros(size & 1, dtype=np.uint8)])
        out.append((name, (v[0::2] << 4 | v[1::2]).astype(np.uint8), size))
    odd = out[0]
    out.append(("pad_nibble_is_other", np.concatenate([odd[1][:-1], [odd[1][-1] | 0x0F]]).astype(np.uint8), odd[2]))  # the nibble past an odd size counts for nothing
    return out
