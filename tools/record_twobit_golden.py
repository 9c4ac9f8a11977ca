#!/usr/bin/env python
"""
Record what the reference's bx.seq.twobit answers for the cases of tests/golden/twobit (run where a built reference is at hand; the
engine is not involved).  Per .2bit file a fixed list of cases -- ``TwoBitSequence.get(start, end)`` and ``seq[a:b:step]`` -- each
with ``do_mask`` True and False: the strings go, one after another, into <file>.mask.npy and <file>.nomask.npy (uint8), and
manifest.json lists every case with its span in that array, or, where the reference raises, the exception's type and message.

The cases: all 16 start and end phases of a packed byte on phases.2bit; on blocks.2bit (and swap.2bit) regions chosen by the tile,
chunk and checkpoint constants, which are read out of bx-python_amd/csrc/twobit.hpp; clipped regions (start < 0, end > size);
regions where the reference raises; slices with open, negative and strided bounds.

The small files come from tools/write_twobit_fixture.py (written first where missing).

Building the one extension the reference needs, out of its tree (a writable copy of its lib/, Cython, nothing else):

    from setuptools import setup, Extension
    from Cython.Build import cythonize
    exts = [Extension("bx.seq._twobit", ["lib/bx/seq/_twobit.pyx"])]
    setup(name="bxseq", package_dir={"": "lib"}, ext_modules=cythonize(exts, language_level=3), script_args=["build_ext", "--inplace"])

(The reference's bx/seq/__init__.py imports bx.seq.core and through it bx.seq.nib's extension, which this tool has no use for: it
registers bare `bx` and `bx.seq` packages that only point at the reference's directories, so that bx.seq.twobit and bx.seq._twobit
are the only modules of the reference that run.)

usage: record_twobit_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR [REFERENCE_SEQ_TESTS_DIR]]
(REFERENCE_SEQ_TESTS_DIR: default test_data/seq_tests beside REFERENCE_LIB_DIR)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)

import twobit_model as M  # noqa: E402
import write_twobit_fixture as W  # noqa: E402


def cases_for(name, sizes):
    """[(seq, op, args)] of a file whose sequences have `sizes`"""
    _, tile, chunk, ckpt = M.kernel_constants()
    out = []
    if name == "phases.2bit":
        out += [("phases", "get", [s, e]) for s in range(4, 8) for e in range(20, 24)]
        out += [("phases", "get", a) for a in ([5, 7], [4, 8], [0, 39], [38, 39], [9, 14], [19, 28], [-3, 50], [7, 7], [9, 2])]
        out += [("phases", "slice", a) for a in ([None, None, None], [-10, None, None], [None, 7, None], [5, 5, None], [3, 2, None], [0, 10, 2], [-100, 100, 1])]
    elif name in ("blocks.2bit", "swap.2bit"):
        size, st = sizes["blocks"], W.STRETCH_START
        regions = [[0, size], [0, tile], [1, tile + 1], [tile - 1, tile + 1], [tile, 2 * tile], [st - 3, st + 2 * (chunk + 5) + 3], [st, st + 2 * chunk],
                   [5000, 5000 + tile], [6000 - 5, 6000 + 2 * (chunk + 5) + 5], [ckpt, 2 * ckpt], [ckpt - 1, ckpt + 1], [ckpt, ckpt + 1], [0, ckpt],
                   [1000, 3 * ckpt + 5], list(W.BIG_N), [W.BIG_N[0] + 100, W.BIG_N[1] - 100], [W.BIG_N[0] - 10, W.BIG_N[1] + 10], [3150, 3175], [3090, 3310],
                   [3390, 3610], [3455, 3460], [90, 1500], [1590, 3000], [size - 10, size], [size - 1, size], [size - 40, size]]
        regions += [[-5, 10], [size - 3, size + 10], [-100, size + 100]]                  # clipped
        regions += [[10, 10], [20, 5], [size, size + 5], [-5, 0]]                         # the reference raises
        out += [("blocks", "get", r) for r in regions]
        out += [("blocks", "slice", a) for a in ([100, 140, None], [-30, None, None], [None, 130, None], [size, None, None], [7, 3, None], [0, 100, 3])]
    elif name == "multi.2bit":
        for seq, size in sizes.items():
            out += [(seq, "get", r) for r in ([0, size], [0, 1], [size - 1, size], [-4, size + 4], [3, 38])]
            out += [(seq, "slice", [None, None, None]), (seq, "slice", [0, 0, None])]
        n = sizes["ckpt"]
        out += [("ckpt", "get", r) for r in ([ckpt - 1, ckpt + 1], [ckpt, 2 * ckpt], [2 * ckpt - 1, n], [2 * ckpt, n], [990, 1110], [2565, n])]
    else:  # the reference's own files
        rng = np.random.default_rng(len(name))
        for seq, size in sizes.items():
            out += [(seq, "get", r) for r in ([0, size], [1, 33], [17, 18], [size - 5, size + 5], [-2, 3], [size, size + 1])]
            out += [(seq, "get", sorted(rng.integers(0, size + 1, size=2).tolist())) for _ in range(10)]
            out += [(seq, "slice", [None, None, None]), (seq, "slice", [-7, -2, None])]
    return out


def main(argv):
    if not argv:
        sys.exit(__doc__)
    lib = os.path.abspath(argv[0])
    golden = argv[1] if len(argv) > 1 else M.GOLDEN
    seq_tests = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(lib), "test_data", "seq_tests")
    W.main([golden, seq_tests])
    import types

    for pkg, where in (("bx", os.path.join(lib, "bx")), ("bx.seq", os.path.join(lib, "bx", "seq"))):
        module = types.ModuleType(pkg)
        module.__path__ = [where]
        sys.modules[pkg] = module
    from bx.seq.twobit import TwoBitFile

    files = {}
    for name in M.FILES:
        path = os.path.join(golden, name)
        strings = {"mask": bytearray(), "nomask": bytearray()}
        cases = []
        with open(path, "rb") as f:
            tbf = TwoBitFile(f)
            sizes = {seq: len(tbf[seq]) for seq in tbf}
        for do_mask in (True, False):
            key = "mask" if do_mask else "nomask"
            with open(path, "rb") as f:
                tbf = TwoBitFile(f, do_mask=do_mask)
                for seq, op, args in cases_for(name, sizes):
                    case = {"seq": seq, "op": op, "args": args, "mask": do_mask}
                    try:
                        text = tbf[seq].get(*args) if op == "get" else tbf[seq][slice(*args)]
                        case["span"] = [len(strings[key]), len(strings[key]) + len(text)]
                        strings[key] += text.encode("ascii")
                    except (Exception, AssertionError) as e:
                        case["error"] = [type(e).__name__, str(e)]
                    cases.append(case)
        for key, data in strings.items():
            np.save(os.path.join(golden, "%s.%s.npy" % (name, key)), np.frombuffer(bytes(data), dtype=np.uint8))
        files[name] = {"sizes": sizes, "strings": {key: "%s.%s.npy" % (name, key) for key in strings}, "cases": cases}
        print("%s: %d cases, %d raised" % (name, len(cases), sum("error" in c for c in cases)))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        json.dump({"stretch_start": W.STRETCH_START, "files": files}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
