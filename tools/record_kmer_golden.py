#!/usr/bin/env python
"""
Record what the reference's bx.intseq.ngramcount.count_ngrams answers on the regions of tests/golden/twobit (run where the
reference is at hand; the engine is not involved): per recorded region of every file of twobit_model.FILES,
``count_ngrams(mapping.translate(seq.get(s, e)), k, radix)`` for k in 1, 2, 3, 6 under three mappings -- bx.seqmapping.DNA itself
(radix 4, case folded), a case-sensitive ACGT mapping and a purine/pyrimidine mapping (radix 2), the last two made with
CharToIntArrayMapping.set_mapping from tests/kmer_model.MAPPINGS.  The string is read by the reference's own TwoBitFile where the
case is a ``get`` (and must equal the recorded one), else it is the recorded string of the slice.  Written to tests/golden/kmers:
<file>.kmers.npy (int32 [2, pairs]: the non-zero counts of every answer one after another, row 0 the index, row 1 the count) and
manifest.json, which lists per file the entries, each [the index of the case in tests/golden/twobit/manifest.json, the mapping, k,
the first pair, past the last pair].  Cases are taken in file order, each with the (mapping, k) pairs its index selects, while the file stays
below the largest one of tests/golden/twobit.

count_ngrams prints from its inner loop, once per window (ngramcount.pyx:79,84): stdout is redirected while it runs.

The extensions the reference needs -- bx.intseq.ngramcount, bx._seqmapping, bx.seq._twobit -- are built here out of its tree, in a
temporary directory, from copies of the three .pyx files and of src/npy_capsule_as_void_ptr.h (Cython and a C compiler, nothing
else).  No __init__.py of the reference is run: bare packages are registered that only point at the reference's directories and
at the built extensions.

usage: record_kmer_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import kmer_model as K  # noqa: E402
import twobit_model as M  # noqa: E402

SETUP = """
import numpy
from setuptools import setup, Extension
from Cython.Build import cythonize
exts = [Extension(n, [n + ".pyx"], include_dirs=[numpy.get_include(), "."]) for n in ("ngramcount", "_seqmapping", "_twobit")]
setup(name="bxkmer", ext_modules=cythonize(exts, language_level=3), script_args=["build_ext", "--inplace"])
"""


def build_extensions(lib):
    work = tempfile.mkdtemp(prefix="bxkmer")
    for rel in ("bx/intseq/ngramcount.pyx", "bx/_seqmapping.pyx", "bx/seq/_twobit.pyx", "../src/npy_capsule_as_void_ptr.h"):
        shutil.copy(os.path.join(lib, rel), work)
    with open(os.path.join(work, "setup.py"), "w") as f:
        f.write(SETUP)
    subprocess.check_call([sys.executable, "setup.py"], cwd=work, stdout=subprocess.DEVNULL)
    return work


def compact(manifest):
    """the manifest as JSON, one line per entry"""
    one = lambda x: json.dumps(x, sort_keys=True)  # noqa: E731
    files = []
    for k, v in sorted(manifest["files"].items()):
        files.append('  %s: {"counts": %s, "entries": [\n%s\n  ]}' % (one(k), one(v["counts"]), ",\n".join(" " + one(e) for e in v["entries"])))
    return '{"files": {\n' + ",\n".join(files) + "\n}}\n"


def main(argv):
    if not argv:
        sys.exit(__doc__)
    lib = os.path.abspath(argv[0])
    golden = argv[1] if len(argv) > 1 else K.GOLDEN
    os.makedirs(golden, exist_ok=True)
    built = build_extensions(lib)
    for pkg, where in (("bx", [os.path.join(lib, "bx"), built]), ("bx.intseq", [os.path.join(lib, "bx", "intseq"), built]),
                       ("bx.seq", [os.path.join(lib, "bx", "seq"), built])):
        module = types.ModuleType(pkg)
        module.__path__ = where
        sys.modules[pkg] = module
    from bx.intseq.ngramcount import count_ngrams
    from bx.seq.twobit import TwoBitFile
    from bx.seqmapping import DNA, CharToIntArrayMapping

    mappings = {"dna": DNA}
    for name in ("acgt", "ry"):
        mappings[name] = CharToIntArrayMapping()
        for ch, d in K.MAPPINGS[name][0].items():
            mappings[name].set_mapping(ch, d)
    for name, (letters, _) in K.MAPPINGS.items():  # the model's tables are the reference's on the letters of a 2bit string
        probe = b"TCAGNtcagn"
        assert mappings[name].translate(probe).tolist() == K.table_of(letters)[np.frombuffer(probe, dtype=np.uint8)].tolist(), name
    names = sorted(K.MAPPINGS)

    limit = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN))
    budget = (limit - 256) // 8  # (index, count) pairs per file
    manifest = {"files": {}}
    for fixture in M.FILES:
        cases = M.recorded(fixture)
        handles = {do_mask: TwoBitFile(open(os.path.join(M.GOLDEN, fixture), "rb"), do_mask=do_mask) for do_mask in (True, False)}
        pairs, entries, used = [], [], 0
        for i, (case, text) in enumerate(cases):
            if text is None or len(text) > 2700:
                continue
            if case["op"] == "get":
                read = handles[case["mask"]][case["seq"]].get(*case["args"])
                assert read == text, (fixture, case)
                text = read
            for j in range(3):  # three (mapping, k) pairs per case, every pair over the cases of a file
                name, k = names[(i + j) % 3], K.KS[(i // 3 + j) % 4]
                radix = K.MAPPINGS[name][1]
                with contextlib.redirect_stdout(io.StringIO()):
                    answer = count_ngrams(mappings[name].translate(text.encode("ascii")), k, radix)
                assert answer.dtype == np.int32 and answer.shape == (radix ** k,)
                at = np.flatnonzero(answer)
                if used + len(at) > budget:
                    continue
                entries.append([i, name, k, used, used + len(at)])
                pairs.append(np.stack([at.astype(np.int32), answer[at]]))
                used += len(at)
        for h in handles.values():
            h.file.close()
        data = np.concatenate(pairs, axis=1) if pairs else np.zeros((2, 0), dtype=np.int32)
        path = os.path.join(golden, "%s.kmers.npy" % fixture)
        np.save(path, data)
        assert os.path.getsize(path) <= limit
        manifest["files"][fixture] = {"counts": "%s.kmers.npy" % fixture, "entries": entries}
        print("%s: %d entries, %d pairs, %d windows, (mapping, k) %d of 12" % (fixture, len(entries), used, int(data[1].sum()),
                                                                            len({(e[1], e[2]) for e in entries})))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write(compact(manifest))
    shutil.rmtree(built)


if __name__ == "__main__":
    main(sys.argv[1:])
