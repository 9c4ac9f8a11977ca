#!/usr/bin/env python
"""
Record what the reference's FastaFile.get and NibFile.get answer (run where the reference is at hand; the engine is not involved):
for every record of test.fa, test2.fa (three records, "> apple"-style headers), testN.fa, testMask.fa and test.nib of the reference's
test_data/seq_tests, and of the two nib files of tools/write_nib_fixture.py (big-endian, odd length), under revcomp in False, "-5'"
and "-3'", the strings of a list of (start, length) pairs: length 0 at both ends, odd and even starts, the whole sequence, the last
base, the first, and seeded pairs.

Written to tests/golden/seqfile: the input files themselves, <file>.strings.npy (uint8: the strings one after another) and
manifest.json, which lists per file "records" -- each [contig, name, length] -- and "entries" -- each [contig, revcomp, start, length,
the first byte, past the last byte].  Data only, a few KiB.

The reference's _nib extension is built in a temporary directory that is removed at the end; nothing of it is kept.

usage: record_seqfile_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import write_nib_fixture  # noqa: E402

GOLDEN = write_nib_fixture.GOLDEN
COPIED = ("test.fa", "test2.fa", "testN.fa", "testMask.fa", "test.nib")
REVCOMPS = (False, "-5'", "-3'")

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
setup(name="bxnib", ext_modules=cythonize([Extension("_nib", ["_nib.pyx"])], language_level=3), script_args=["build_ext", "--inplace"])
"""


def build_extension(lib):
    work = tempfile.mkdtemp(prefix="bxnib")
    shutil.copy(os.path.join(lib, "bx", "seq", "_nib.pyx"), work)
    with open(os.path.join(work, "setup.py"), "w") as f:
        f.write(SETUP)
    subprocess.check_call([sys.executable, "setup.py"], cwd=work, stdout=subprocess.DEVNULL)
    return work


def ranges_of(length, rng):
    """(start, length) pairs inside a sequence of `length` bases"""
    out = [(0, 0), (length, 0), (0, length)]
    if length >= 1:
        out += [(length - 1, 1), (0, 1)]
    if length >= 8:
        out += [(1, 1), (1, 4), (2, 5), (3, length - 3), (4, length - 5), (length // 2, length - length // 2), (length - 7, 6)]
        for _ in range(6):
            start = int(rng.integers(0, length))
            out.append((start, int(rng.integers(0, length - start + 1))))
    return out


def compact(manifest):
    one = lambda x: json.dumps(x, sort_keys=True)  # noqa: E731
    files = []
    for k, v in sorted(manifest["files"].items()):
        files.append('  %s: {"strings": %s, "records": %s, "entries": [\n%s\n  ]}'
                     % (one(k), one(v["strings"]), one(v["records"]), ",\n".join(" " + one(e) for e in v["entries"])))
    return '{"files": {\n' + ",\n".join(files) + "\n}}\n"


def main(argv):
    if not argv:
        sys.exit(__doc__)
    lib = os.path.abspath(argv[0])
    golden = argv[1] if len(argv) > 1 else GOLDEN
    os.makedirs(golden, exist_ok=True)
    for name in COPIED:
        shutil.copyfile(os.path.join(lib, "..", "test_data", "seq_tests", name), os.path.join(golden, name))
    write_nib_fixture.main([golden])
    built = build_extension(lib)
    for pkg, where in (("bx", [os.path.join(lib, "bx")]), ("bx.seq", [os.path.join(lib, "bx", "seq"), built])):
        module = types.ModuleType(pkg)
        module.__path__ = where
        sys.modules[pkg] = module
    from bx.seq.fasta import FastaFile
    from bx.seq.nib import NibFile

    rng = np.random.default_rng(20)
    manifest = {"files": {}}
    for name in COPIED + ("edges_be.nib", "random_be.nib"):
        path = os.path.join(golden, name)
        records, entries, texts, held = [], [], [], 0
        contig = 1
        while True:
            pairs = None
            for revcomp in REVCOMPS:
                if name.endswith(".nib"):
                    seq = NibFile(open(path, "rb"), revcomp)
                else:
                    try:
                        seq = FastaFile(open(path), revcomp, contig=contig)
                    except AssertionError:  # (no such contig: the file is done)
                        seq = None
                if seq is None:
                    break
                if pairs is None:
                    pairs = ranges_of(seq.length, rng)
                    records.append([contig, seq.name, seq.length])
                for start, length in pairs:
                    text = seq.get(start, length)
                    assert len(text) == length
                    entries.append([contig, revcomp, start, length, held, held + length])
                    texts.append(np.frombuffer(text.encode("ascii"), dtype=np.uint8))
                    held += length
                seq.file.close()
            if pairs is None or name.endswith(".nib"):
                break
            contig += 1
        np.save(os.path.join(golden, name + ".strings.npy"), np.concatenate(texts))
        manifest["files"][name] = {"strings": name + ".strings.npy", "records": records, "entries": entries}
        print("%s: %d records, %d entries, %d letters" % (name, len(records), len(entries), held))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write(compact(manifest))
    shutil.rmtree(built)


if __name__ == "__main__":
    main(sys.argv[1:])
