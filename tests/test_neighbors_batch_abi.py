"""CPU-only: the batched neighbour entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so,
and the Python layers carry their batch methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bxmi_ivl_neighbors_batch", "bxmi_ivl_neighbors_batch_dev")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _ffi.EXPORTED, name
        assert hasattr(lib, name), name
    # host variant: handle, pos, nq, k, max_dist, dir, out, n_out, n_cand; the device variant adds the stream
    assert len(_ffi._SIGNATURES[NAMES[0]]) == 9 and len(_ffi._SIGNATURES[NAMES[1]]) == 10


def test_python_batch_methods_exist():
    from bx.intervals.intersection import IntervalTree
    from bxmi.intervals import IntervalIndex

    for m in ("before_batch", "after_batch", "neighbors_batch_dev"):
        assert callable(getattr(IntervalIndex, m, None)), m
    for m in ("before_many", "after_many", "upstream_many", "downstream_many"):
        assert callable(getattr(IntervalTree, m, None)), m
    assert IntervalTree().before_many([1, 2, 3]) == [[], [], []]  # an empty tree needs no device
