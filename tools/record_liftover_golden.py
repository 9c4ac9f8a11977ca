#!/usr/bin/env python
"""
Record what the reference's scripts/bnMapper.py answers for the cases of tests/golden/bnmapper (run where a built
reference is at hand; the engine is not involved).  Output lines are taken in the order of the input rows -- the
reference writes source chromosomes in set order.  The reference's own small case is stored as the files it wrote; of the
synthetic case (stored gzipped: syn.bed.gz, syn.chain.gz) manifest.json keeps, per option set, the number of output lines of
every input row and the SHA-256 of all lines in row order.

usage: record_liftover_golden.py BNMAPPER_PY REFERENCE_LIB_DIR [GOLDEN_DIR]
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
EPO = "epo_547_hs_mm_12way_mammals_65.chain"
# (expectation, input, alignment, options)
CASES = [
    ("hpeaks.default.bed4", "hpeaks.bed", EPO, []),
    ("hpeaks.default.bed12", "hpeaks.bed", EPO, ["-fBED12"]),
    ("hpeaks.g9.bed4", "hpeaks.bed", EPO, ["-g9"]),
    ("hpeaks.g3.bed4", "hpeaks.bed", EPO, ["-g3"]),
    ("hpeaks.g9_t0.67.bed4", "hpeaks.bed", EPO, ["-g9", "-t0.67"]),
    ("hpeaks.g9_t0.7.bed4", "hpeaks.bed", EPO, ["-g9", "-t0.7"]),
    ("hpeaks.k.bed4", "hpeaks.bed", EPO, ["-k"]),
    ("hpeaks.k.narrowPeak", "hpeaks.narrowPeak", EPO, ["-k", "-inarrowPeak", "-fnarrowPeak"]),
    ("hpeaks.g3.narrowPeak", "hpeaks.narrowPeak", EPO, ["-g3", "-inarrowPeak", "-fnarrowPeak"]),
    ("syn.default.bed4", "syn.bed.gz", "syn.chain.gz", []),
    ("syn.k.bed4", "syn.bed.gz", "syn.chain.gz", ["-k"]),
    ("syn.g5.bed4", "syn.bed.gz", "syn.chain.gz", ["-g5"]),
    ("syn.g0_k.bed4", "syn.bed.gz", "syn.chain.gz", ["-g0", "-k"]),
    ("syn.t0.5_k.bed4", "syn.bed.gz", "syn.chain.gz", ["-t0.5", "-k"]),
    ("syn.t0.9.bed4", "syn.bed.gz", "syn.chain.gz", ["-t0.9"]),
    ("syn.k.bed12", "syn.bed.gz", "syn.chain.gz", ["-fBED12", "-k"]),
]


def main(script, libdir, golden=os.path.join(HERE, "..", "tests", "golden", "bnmapper")):
    env = dict(os.environ, PYTHONPATH=libdir)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:  # (the reference drops a .pkl beside the alignment: work on copies)
        for name in sorted({c[1] for c in CASES} | {c[2] for c in CASES}):
            if name.endswith(".gz"):
                with gzip.open(os.path.join(golden, name), "rb") as src, open(os.path.join(tmp, name[:-3]), "wb") as dst:
                    dst.write(src.read())
            else:
                shutil.copy(os.path.join(golden, name), tmp)
        for expect, bed, chain, opts in CASES:
            raw = os.path.join(tmp, "out.txt")
            plain = [os.path.join(tmp, n[:-3] if n.endswith(".gz") else n) for n in (bed, chain)]
            subprocess.run([sys.executable, script, "-v", "silent", *opts, "-o", raw, *plain], check=True, env=env, stderr=subprocess.DEVNULL)
            row_of = {line.split()[3]: n for n, line in enumerate(open(plain[0]))}
            lines = open(raw).readlines()
            lines.sort(key=lambda l: row_of[l.split()[3]])  # stable: a feature's lines keep their order
            case = {"expected": expect, "input": bed, "alignment": chain, "options": opts, "lines": len(lines)}
            if expect.startswith("syn"):
                per_row = [0] * len(row_of)
                for l in lines:
                    per_row[row_of[l.split()[3]]] += 1
                case["lines_per_row"] = "".join(chr(48 + min(n, 74)) for n in per_row)  # one character per input row: '0' + count
                assert max(per_row) < 74
                case["sha256"] = hashlib.sha256("".join(lines).encode()).hexdigest()
            else:
                with open(os.path.join(golden, expect), "w") as f:
                    f.writelines(lines)
            manifest.append(case)
            print(expect, len(lines))
    with open(os.path.join(golden, "manifest.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in manifest) + "\n]\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
