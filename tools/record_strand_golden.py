#!/usr/bin/env python
"""
Record what the reference's reverse complement answers on the regions of tests/golden/twobit (run where the reference is at hand;
the engine is not involved): per recorded region of every file of twobit_model.FILES, under both do_mask settings,

  letters   ``seq.get(s, e).translate(DNA_COMP)[::-1]`` -- SeqFile.reverse_complement (lib/bx/seq/seq.py:108-109) with DNA_COMP
            imported from the reference's bx.seq.seq.  The string is read by the reference's own TwoBitFile where the case is a
            ``get`` (and must equal the recorded one), else it is the recorded string of the slice.
  k-mers    ``count_ngrams(mapping.translate(that string), k, radix)`` for k in 1, 2, 3, 6 under the three mappings of
            tools/record_kmer_golden.py (tests/kmer_model.MAPPINGS), three (mapping, k) pairs per case, as non-zero pairs.

Written to tests/golden/strand: <file>.rc.npy (uint8: the strings one after another), <file>.rckmers.npy (int32 [2, pairs]: row 0
the index, row 1 the count) and manifest.json, which lists per file "strings" -- each [the index of the case in
tests/golden/twobit/manifest.json, the first byte, past the last byte] -- and "entries" -- each [the case, the mapping, k, the
first pair, past the last pair].  Data only; the counts of a file stay below the largest file of tests/golden/twobit, its strings (every one is kept) below 512 KiB.

The extensions the reference needs are built as tools/record_kmer_golden.py builds them, in a temporary directory that is removed
at the end; none of them is kept.

usage: record_strand_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import contextlib
import io
import json
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)

import kmer_model as K  # noqa: E402
import strand_model as S  # noqa: E402
import twobit_model as M  # noqa: E402
from record_kmer_golden import build_extensions  # noqa: E402


def compact(manifest):
    """the manifest as JSON, one line per entry"""
    one = lambda x: json.dumps(x, sort_keys=True)  # noqa: E731
    files = []
    for k, v in sorted(manifest["files"].items()):
        rows = lambda key: ",\n".join(" " + one(e) for e in v[key])  # noqa: E731
        files.append('  %s: {"letters": %s, "counts": %s, "strings": [\n%s\n  ], "entries": [\n%s\n  ]}'
                     % (one(k), one(v["letters"]), one(v["counts"]), rows("strings"), rows("entries")))
    return '{"files": {\n' + ",\n".join(files) + "\n}}\n"


def main(argv):
    if not argv:
        sys.exit(__doc__)
    lib = os.path.abspath(argv[0])
    golden = argv[1] if len(argv) > 1 else S.GOLDEN
    os.makedirs(golden, exist_ok=True)
    built = build_extensions(lib)
    for pkg, where in (("bx", [os.path.join(lib, "bx"), built]), ("bx.intseq", [os.path.join(lib, "bx", "intseq"), built]),
                       ("bx.seq", [os.path.join(lib, "bx", "seq"), built])):
        module = types.ModuleType(pkg)
        module.__path__ = where
        sys.modules[pkg] = module
    from bx.intseq.ngramcount import count_ngrams
    from bx.seq.seq import DNA_COMP
    from bx.seq.twobit import TwoBitFile
    from bx.seqmapping import DNA, CharToIntArrayMapping

    mappings = {"dna": DNA}
    for name in ("acgt", "ry"):
        mappings[name] = CharToIntArrayMapping()
        for ch, d in K.MAPPINGS[name][0].items():
            mappings[name].set_mapping(ch, d)
    names = sorted(K.MAPPINGS)

    limit = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN))
    budget = (limit - 256) // 8  # (index, count) pairs per file
    manifest = {"files": {}}
    for fixture in M.FILES:
        cases = M.recorded(fixture)
        handles = {do_mask: TwoBitFile(open(os.path.join(M.GOLDEN, fixture), "rb"), do_mask=do_mask) for do_mask in (True, False)}
        texts, strings, pairs, entries, used, held = [], [], [], [], 0, 0
        for i, (case, text) in enumerate(cases):
            if text is None:
                continue
            if case["op"] == "get":
                read = handles[case["mask"]][case["seq"]].get(*case["args"])
                assert read == text, (fixture, case)
                text = read
            rc = text.translate(DNA_COMP)[::-1]
            assert len(rc) == len(text)
            strings.append([i, held, held + len(rc)])
            texts.append(np.frombuffer(rc.encode("ascii"), dtype=np.uint8))
            held += len(rc)
            if len(rc) > 2700:
                continue
            for j in range(3):  # three (mapping, k) pairs per case, every pair over the cases of a file
                name, k = names[(i + j) % 3], K.KS[(i // 3 + j) % 4]
                radix = K.MAPPINGS[name][1]
                with contextlib.redirect_stdout(io.StringIO()):
                    answer = count_ngrams(mappings[name].translate(rc.encode("ascii")), k, radix)
                assert answer.dtype == np.int32 and answer.shape == (radix ** k,)
                at = np.flatnonzero(answer)
                if used + len(at) > budget:
                    continue
                entries.append([i, name, k, used, used + len(at)])
                pairs.append(np.stack([at.astype(np.int32), answer[at]]))
                used += len(at)
        for h in handles.values():
            h.file.close()
        letters = np.concatenate(texts) if texts else np.zeros(0, dtype=np.uint8)
        data = np.concatenate(pairs, axis=1) if pairs else np.zeros((2, 0), dtype=np.int32)
        for suffix, array, most in (("rc", letters, 1 << 19), ("rckmers", data, limit)):  # (every string is kept: both settings in one file)
            path = os.path.join(golden, "%s.%s.npy" % (fixture, suffix))
            np.save(path, array)
            assert os.path.getsize(path) <= most
        manifest["files"][fixture] = {"letters": "%s.rc.npy" % fixture, "counts": "%s.rckmers.npy" % fixture, "strings": strings, "entries": entries}
        print("%s: %d of %d strings, %d letters, %d entries, %d pairs" % (fixture, len(strings), sum(t is not None for _, t in cases), held,
                                                                        len(entries), used))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write(compact(manifest))
    shutil.rmtree(built)


if __name__ == "__main__":
    main(sys.argv[1:])
