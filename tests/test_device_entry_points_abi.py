"""CPU-only: every device-pointer (`_dev`) entry point declared in include/bxmi.h is bound in _ffi, exported by libbxmi.so,
and named by its C name, as a string (an `_ffi.call("bxmi_..._dev", ...)` or an entry of a module-level tuple), in at least one
GPU test file -- so a new `_dev` entry point without a GPU test fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the other device-pointer entry point: the collective, covered by tests/test_gpu_intervals.py through bxmi.shard (by method, not
# by C name), so it is checked for its binding only
ALSO_DEVICE = ("bxmi_allreduce_i64",)


def declared_dev_names():
    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    return sorted(set(re.findall(r"\bint\s+(bxmi_\w+_dev)\s*\(", header)))


def gpu_test_sources():
    out = {}
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))):
        with open(p) as f:
            out[os.path.basename(p)] = f.read()
    return out


def test_header_declares_the_dev_entry_points():
    names = declared_dev_names()
    assert len(names) >= 16, names  # (a regex that stopped matching would make the tests below vacuous)
    for n in ("bxmi_ivl_find_dev", "bxmi_ivl_count_dev", "bxmi_bits_popcount_dev", "bxmi_bits_group_popcount_dev"):
        assert n in names, n


def test_dev_entry_points_bound_and_exported():
    from bxmi import _ffi

    lib = _ffi.load()
    for name in declared_dev_names() + list(ALSO_DEVICE):
        assert name in _ffi._SIGNATURES, name
        assert name in _ffi.EXPORTED, name
        assert hasattr(lib, name), name
        # the stream-ordered forms end in the stream (void *); the two introspection views have none
        if name not in ("bxmi_ivl_order_dev", "bxmi_bits_words_dev"):
            assert _ffi._SIGNATURES[name][-1] is _ffi.vp, name


def test_every_dev_entry_point_has_a_gpu_test():
    sources = gpu_test_sources()
    assert sources, "no tests/test_gpu_*.py"
    missing = [n for n in declared_dev_names() if not any(re.search(r"[\"']%s[\"']" % n, src) for src in sources.values())]
    assert not missing, "device entry points no GPU test names: %s" % missing
