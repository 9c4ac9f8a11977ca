"""CPU-only: the liftover entry points are declared in include/bxmi.h, bound in _ffi and exported by libbxmi.so; the device
variant's signature ends in the stream; the Python layers and the command line import without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bxmi_chainmap_create", "bxmi_chainmap_destroy", "bxmi_chainmap_info", "bxmi_chainmap_map", "bxmi_chainmap_map_dev")


def test_declared_bound_and_exported():
    from bxmi import _ffi

    header = open(os.path.join(ROOT, "include", "bxmi.h")).read()
    lib = _ffi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _ffi.EXPORTED, name
        assert hasattr(lib, name), name
    host, dev = _ffi._SIGNATURES["bxmi_chainmap_map"], _ffi._SIGNATURES["bxmi_chainmap_map_dev"]
    assert dev[:-1] == host and dev[-1] is C.c_void_p  # the same arguments, then the stream
    decl = re.search(r"int bxmi_chainmap_map_dev\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl).strip().endswith("void *stream")
    assert len(re.findall(r",", decl)) + 1 == len(dev)
    for status in ("MAPPED 0", "NOCHAIN 1", "SPLIT 2", "BELOW 3", "EMPTY 4"):
        assert re.search(r"#define BXMI_LIFT_%s\b" % status, header), status


def test_python_layers_import():
    from bxmi import liftover
    from bxmi.chain import load_chains
    from bxmi.cli import bnMapper

    for m in ("from_file", "map", "map_dev", "map_ptrs", "info", "chroms"):
        assert callable(getattr(liftover.ChainMap, m, None)), m
    assert callable(bnMapper.main) and callable(load_chains)
    assert (liftover.MAPPED, liftover.NOCHAIN, liftover.SPLIT, liftover.BELOW, liftover.EMPTY) == (0, 1, 2, 3, 4)
    assert (liftover.UNIQUE, liftover.LONGEST, liftover.FIRST) == (0, 1, 2)


def test_chain_reader_matches_the_model(tmp_path):
    """bxmi.chain (arrays) and tests/liftover_model.py (per row) read the fixtures alike; .gz is read; no .pkl appears."""
    import gzip
    import shutil

    import numpy as np

    import liftover_model as M
    from bxmi.chain import load_chains

    golden = os.path.join(ROOT, "tests", "golden", "bnmapper")
    shutil.copy(os.path.join(golden, "syn.chain.gz"), tmp_path)
    with gzip.open(tmp_path / "syn.chain.gz", "rb") as src, open(tmp_path / "syn.chain", "wb") as dst:
        dst.write(src.read())
    shutil.copy(os.path.join(golden, "epo_547_hs_mm_12way_mammals_65.chain"), tmp_path)
    names = ("syn.chain", "syn.chain.gz", "epo_547_hs_mm_12way_mammals_65.chain")
    for name in names:
        tables, model = load_chains(str(tmp_path / name)), M.load_chains(str(tmp_path / name))
        assert list(tables) == list(model)
        for chrom, t in tables.items():
            assert len(t) == len(model[chrom])
            for c, mc in enumerate(model[chrom]):
                T, Q = t.block_table(c)
                assert T.tolist() == [list(x) for x in mc["T"]] and Q.tolist() == [list(x) for x in mc["Q"]]
                assert (int(t.t_start[c]), int(t.t_end[c]), int(t.q_start[c]), int(t.q_span[c]), bool(t.q_minus[c]), t.q_name[c], t.ids[c]) == (
                    mc["tS"], mc["tE"], mc["qS"], mc["Sz"], mc["minus"], mc["qName"], mc["id"])
            assert t.block_off.dtype == np.int64 and t.blk_t_start.dtype == np.int32
    assert sorted(os.listdir(tmp_path)) == sorted(names)
