"""CPU-only: bxmi.twobit reads the fixtures of tests/golden/twobit into the arrays tools/write_twobit_fixture.py put there -- either
byte order, the index in file order, sizes, N and mask blocks, packed bytes -- lazily by name or all at once, and refuses what the
reference refuses with its messages."""
import io
import os
import struct
import sys

import numpy as np
import pytest

import twobit_model as M

sys.path.insert(0, os.path.join(M.ROOT, "tools"))
import write_twobit_fixture as W  # noqa: E402

from bxmi import twobit  # noqa: E402


def path(name):
    return os.path.join(M.GOLDEN, name)


def test_blocks_fixture_holds_what_the_writer_put_there():
    name, codes, n_blocks, m_blocks = W.blocks_sequence(M.CHUNK)
    for file, order in (("blocks.2bit", ">"), ("swap.2bit", "<")):
        reader = twobit.TwoBitReader(path(file))
        assert (reader.byte_order, reader.version, reader.seq_count, reader.names) == (order, 0, 1, [name])
        seq = reader.load(name)
        assert seq.size == W.BLOCKS_SIZE == len(codes) and len(seq.packed) == (seq.size + 3) // 4
        assert np.array_equal(M.codes_of(seq), codes)
        assert list(zip(seq.n_starts.tolist(), seq.n_sizes.tolist())) == n_blocks
        assert list(zip(seq.m_starts.tolist(), seq.m_sizes.tolist())) == m_blocks
        assert seq.n_starts.dtype == np.uint32 and seq.packed.dtype == np.uint8
        assert reader.load(name) is seq  # kept
    # the fixture has what the issue asks of it
    n_end = [s + n for s, n in n_blocks]
    assert {s % 4 for s, _ in n_blocks[:16]} == {e % 4 for e in n_end[:16]} == {0, 1, 2, 3}
    assert len({(s % 4, (s + n) % 4) for s, n in n_blocks[:16]}) == 16 and len({(s % 4, (s + n) % 4) for s, n in m_blocks[1:17]}) == 16
    assert sum(n == 1 for _, n in n_blocks) == M.CHUNK + 5 and n_end[-1] == W.BLOCKS_SIZE
    under = np.concatenate([codes[s:s + n] for s, n in n_blocks])
    assert len(set(under.tolist())) == 4  # random, not zero, codes under the N blocks


def test_multi_in_file_order_and_lazily():
    reader = twobit.TwoBitReader(path("multi.2bit"))
    assert reader.names == ["odd", "empty", "ckpt"] and not reader._loaded
    assert reader.load("empty").size == 0 and len(reader.load("empty").packed) == 0 and list(reader._loaded) == ["empty"]
    seqs = reader.load_all()
    assert [s.size for s in seqs.values()] == [41, 0, 2579] and list(seqs) == reader.names
    assert seqs["odd"].size % 4 == 1 and 2 * M.CKPT < seqs["ckpt"].size < 3 * M.CKPT and seqs["ckpt"].size % 4
    assert seqs["ckpt"].n_starts.tolist() == [1000, 2040, 2570] and seqs["ckpt"].m_sizes.tolist() == [10, 10, 452]
    with pytest.raises(KeyError):
        reader.load("chrNone")


def test_sources_path_bytes_and_file_object():
    data = open(path("phases.2bit"), "rb").read()
    with open(path("phases.2bit"), "rb") as f:
        f.read(7)
        readers = [twobit.TwoBitReader(path("phases.2bit")), twobit.TwoBitReader(data), twobit.TwoBitReader(f)]
        for reader in readers:
            seq = reader.load("phases")
            assert (seq.size, seq.n_starts.tolist(), seq.n_sizes.tolist(), seq.m_starts.tolist(), seq.m_sizes.tolist()) == (39, [10], [3], [20], [7])
    assert list(twobit.read_file(path("test.2bit"))) == list(M.manifest()["files"]["test.2bit"]["sizes"])


def test_a_sequence_is_read_when_it_is_loaded_not_before():
    """a file object sees the header and the index at construction and one record per load; a path is not held open"""
    class Counting(io.BytesIO):
        bytes_read = 0

        def read(self, n=-1):
            got = super().read(n)
            self.bytes_read += len(got)
            return got

    data = open(path("multi.2bit"), "rb").read()
    f = Counting(data)
    reader = twobit.TwoBitReader(f)
    index_bytes = 16 + sum(1 + len(n) + 4 for n in reader.names)
    assert f.bytes_read == index_bytes
    odd = reader.load("odd")
    assert f.bytes_read == index_bytes + 4 + (4 + 8) * 2 + 4 + len(odd.packed) and len(odd.packed) == 11
    reader.load("odd")
    assert f.bytes_read == index_bytes + 32 + 11  # kept: not read again
    by_path = twobit.TwoBitReader(path("multi.2bit"))
    assert by_path._file is None and by_path.load("ckpt").size == 2579


def test_refusals_carry_the_references_messages():
    data = bytearray(open(path("phases.2bit"), "rb").read())
    with pytest.raises(Exception, match="^Not a NIB file$"):
        twobit.TwoBitReader(b"\x00\x01\x02\x03" + bytes(data[4:]))
    for order in (">", "<"):
        bad = struct.pack(order + "LL", twobit.MAGIC, 1) + bytes(data[8:])
        with pytest.raises(Exception, match="^File is version '1' but I only know about '0'$"):
            twobit.TwoBitReader(bad)
    with pytest.raises(ValueError, match="truncated"):
        twobit.TwoBitReader(bytes(data[:-3])).load("phases")
    for cut in (6, 16, 19, 24):  # inside the header, before the index, inside a name, inside an offset
        with pytest.raises(ValueError, match="truncated"):
            twobit.TwoBitReader(bytes(data[:cut]))
    with pytest.raises(Exception, match="^Not a NIB file$"):
        twobit.TwoBitReader(bytes(data[:3]))
    with pytest.raises(ValueError, match="truncated"):
        twobit.TwoBitReader(bytes(data[:40])).load("phases")  # inside the record's block lists
