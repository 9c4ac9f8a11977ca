"""
The checker of the liftover tests against the reference's own answers: tests/liftover_model.py, a per-row restatement of
scripts/bnMapper.py, reproduces every expectation recorded under tests/golden/bnmapper (tools/record_liftover_golden.py ran the
real script) exactly: the files that script wrote for its own small case; for the seeded synthetic case (gzipped inputs) the
number of output lines of every input row and the SHA-256 of all lines in row order.  Runs without a GPU; tests/test_gpu_liftover.py then holds the engine against the same files and, on
fresh inputs, against the model.
"""
import hashlib
import json
import os

import pytest

import liftover_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bnmapper")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def options_of(opts):
    """the script's options as keyword arguments of liftover_model.run"""
    kw = {}
    for o in opts:
        if o == "-k":
            kw["keep_split"] = True
        elif o.startswith("-g"):
            kw["gap"] = int(o[2:])
        elif o.startswith("-t"):
            kw["threshold"] = float(o[2:])
        elif o.startswith("-f"):
            kw["fmt"] = o[2:]
        elif o.startswith("-i"):
            kw["in_format"] = o[2:]
        else:
            raise ValueError(o)
    return kw


def assert_as_recorded(case, got):
    """got = {input row: its output lines} against what the reference wrote for this case"""
    feats = M.read_lines(os.path.join(GOLDEN, case["input"]))
    if "sha256" in case:
        counts = "".join(chr(48 + len(got.get(n, ()))) for n in range(len(feats)))
        wrong = [n for n in range(len(feats)) if counts[n] != case["lines_per_row"][n]]
        assert not wrong, ("rows with another number of output lines", wrong[:10], [got.get(n) for n in wrong[:3]])
        assert hashlib.sha256("".join(l for n in sorted(got) for l in got[n]).encode()).hexdigest() == case["sha256"]
        return
    row_of = {line.split()[3]: n for n, line in enumerate(feats)}
    want = {}
    for line in open(os.path.join(GOLDEN, case["expected"])):
        want.setdefault(row_of[line.split()[3]], []).append(line)
    assert sum(len(v) for v in want.values()) == case["lines"]
    assert got == want


@pytest.mark.parametrize("case", MANIFEST, ids=[c["expected"] for c in MANIFEST])
def test_model_reproduces_the_reference(case):
    got = M.run(os.path.join(GOLDEN, case["input"]), os.path.join(GOLDEN, case["alignment"]), **options_of(case["options"]))
    assert_as_recorded(case, got)


def _mapped(expected):
    """the input rows a recorded option set of the synthetic case maps"""
    case = [c for c in MANIFEST if c["expected"] == expected][0]
    return {n for n, ch in enumerate(case["lines_per_row"]) if ch != "0"}


def test_the_synthetic_case_is_as_hard_as_it_must_be():
    """From the recorded expectations, so that a weaker regenerated case cannot pass silently: of the features that meet a chain,
    at least 5 % each end as mapped, dropped as split, dropped by the gap rule (-g5) and dropped by the threshold (-t0.9); at
    least 20 meet only chains that yield nothing; at least a third of the chains lie on each query strand."""
    chains = M.load_chains(os.path.join(GOLDEN, "syn.chain.gz"))
    feats = [line.split() for line in M.read_lines(os.path.join(GOLDEN, "syn.bed.gz"))]
    meets = {n for n, f in enumerate(feats) if M.find(chains.get(f[0], []), int(f[1]), int(f[2]))}
    mapped, kept, g5, t09 = _mapped("syn.default.bed4"), _mapped("syn.k.bed4"), _mapped("syn.g5.bed4"), _mapped("syn.t0.9.bed4")
    assert mapped <= kept <= meets and g5 <= meets and t09 <= mapped  # (-g5 can also rescue a split feature: one of its chains drops out)
    n = len(meets)
    print("meet a chain %d, mapped %d, split %d, gap-dropped %d, threshold-dropped %d, yield nothing %d"
          % (n, len(mapped), len(kept - mapped), len(mapped - g5), len(mapped - t09), len(meets - kept)))
    assert len(mapped) >= 0.05 * n
    assert len(kept - mapped) >= 0.05 * n
    assert len(mapped - g5) >= 0.05 * n
    assert len(mapped - t09) >= 0.05 * n
    assert len(meets - kept) >= 20
    every = [c for cs in chains.values() for c in cs]
    minus = sum(c["minus"] for c in every)
    assert 3 * minus >= len(every) and 3 * (len(every) - minus) >= len(every)
    assert len(chains) == 2 and len(every) == 60 and len(feats) == 3000
