#!/usr/bin/env python
"""
Record what the reference answers for a position weight matrix on the MINUS strand of the strings of tests/golden/twobit:
matrix.score_string(seq.get(s, e).translate(DNA_COMP)[::-1]) -- bx.motif.pwm.ScoringMatrix.score_string (lib/bx/motif/pwm.py:141-149
over _pwm.pyx:23-55) on SeqFile.reverse_complement's string (lib/bx/seq/seq.py:108-109), DNA_COMP the reference's own (seq.py:9-14).
Run where the reference is at hand; the engine is not involved.  The (region, matrix) pairs are exactly the entries of
tests/golden/pwm/manifest.json -- every recorded region under every matrix it was recorded with, both do_mask settings, the matrices
whose alphabets are not closed under complement (w20n, w4n, w1lc, w20lc) among them -- and the matrices are the recorded
tests/golden/pwm/mat.<name>.npy.  Written to tests/golden/pwm_strand: <file>.scores.npy (float32, the answers one after another) and
manifest.json, which lists per file the entries (the index of the case in tests/golden/twobit/manifest.json, the matrix, the span of
the answer) and how many of the plus entries were kept.  No file is larger than the largest one of tests/golden/pwm: whole entries are
kept in manifest order while they fit.

The one extension the reference needs, bx.motif._pwm, is built as tools/record_pwm_golden.py builds it: out of its tree, in a
temporary directory that is removed again.  bx.seq.seq is imported from the reference for DNA_COMP alone.

usage: record_pwm_strand_golden.py REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import importlib.util
import json
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)

import pwm_model as P  # noqa: E402
import record_pwm_golden as R  # noqa: E402
import twobit_model as M  # noqa: E402

GOLDEN = os.path.join(M.ROOT, "tests", "golden", "pwm_strand")


def dna_comp(lib):
    """the reference's DNA_COMP, from lib/bx/seq/seq.py run on its own (bx/seq/__init__.py is never run)"""
    spec = importlib.util.spec_from_file_location("bx_seq_seq", os.path.join(lib, "bx", "seq", "seq.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.DNA_COMP


def compact(manifest):
    one = lambda x: json.dumps(x, sort_keys=True)  # noqa: E731
    files = []
    for k, v in sorted(manifest["files"].items()):
        files.append('  %s: {"scores": %s, "kept": %s, "entries": [\n%s\n  ]}' % (one(k), one(v["scores"]), one(v["kept"]),
                                                                                  ",\n".join("    " + one(e) for e in v["entries"])))
    return '{"files": {\n' + ",\n".join(files) + "\n}}\n"


def main(argv):
    if not argv:
        sys.exit(__doc__)
    lib = os.path.abspath(argv[0])
    golden = argv[1] if len(argv) > 1 else GOLDEN
    os.makedirs(golden, exist_ok=True)
    built = R.build_extension(lib)
    for pkg, where in (("bx", [os.path.join(lib, "bx")]), ("bx.motif", [os.path.join(lib, "bx", "motif"), built])):
        module = types.ModuleType(pkg)
        module.__path__ = where
        sys.modules[pkg] = module
    from bx.motif.pwm import ScoringMatrix

    comp = dna_comp(lib)
    limit = max(os.path.getsize(os.path.join(P.GOLDEN, f)) for f in os.listdir(P.GOLDEN))
    budget = (limit - 128) // 4  # floats per file, behind the 128 bytes of an .npy header
    reference = {}
    for name, entry in P.manifest()["matrices"].items():
        rows = np.load(os.path.join(P.GOLDEN, entry["file"]))
        reference[name] = ScoringMatrix.from_rows(list(entry["alphabet"]), rows.tolist())
        assert reference[name].values.dtype == np.float32
    manifest = {"files": {}}
    for fixture in M.FILES:
        cases = M.recorded(fixture)
        plus = P.manifest()["files"][fixture]["entries"]
        data, entries, used = [], [], 0
        for e in plus:
            text = cases[e["case"]][1]
            if used + len(text) > budget:
                break  # (whole entries, in manifest order)
            answer = reference[e["matrix"]].score_string(text.translate(comp)[::-1])
            assert answer.dtype == np.float32 and len(answer) == len(text)
            entries.append({"case": e["case"], "matrix": e["matrix"], "span": [used, used + len(text)]})
            data.append(answer)
            used += len(text)
        scores = np.concatenate(data) if data else np.zeros(0, dtype=np.float32)
        np.save(os.path.join(golden, "%s.scores.npy" % fixture), scores)
        assert os.path.getsize(os.path.join(golden, "%s.scores.npy" % fixture)) <= limit
        manifest["files"][fixture] = {"scores": "%s.scores.npy" % fixture, "kept": [len(entries), len(plus)], "entries": entries}
        print("%s: kept %d of %d entries, %d scores, %d of them numbers, matrices %s" % (fixture, len(entries), len(plus), used, int((~np.isnan(scores)).sum()),
                                                                                        " ".join(sorted({e["matrix"] for e in entries}))))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write(compact(manifest))
    shutil.rmtree(built)


if __name__ == "__main__":
    main(sys.argv[1:])
