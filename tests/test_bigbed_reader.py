"""CPU-only: bxmi.bigbed reads the fixtures of tests/golden/bigbed (written by tools/write_bigbed_fixture.py, read by the reference
when tools/record_bigbed_golden.py recorded them): byte-order and compressed twins give identical arrays, chromosomes that share a
block are split record by record, the `rest` strings round-trip, what is not a whole bigBed file raises ValueError, and every
public function of bxmi.bigwig still refuses these files."""
import os
import struct
import sys

import numpy as np
import pytest

from bed_cases import FILES, GOLDEN, ROOT, path_of

sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_twins_give_identical_arrays():
    from bxmi import bigbed

    a, b, c = (bigbed.read_items_file(path_of(n)) for n in ("genes.bb", "genes.z.bb", "genes.be.bb"))
    assert list(a) == list(b) == list(c) == ["chrA", "chrBB"]
    for chrom in a:
        for x, y, z in zip(a[chrom][:2], b[chrom][:2], c[chrom][:2]):
            assert x.dtype == np.int32 and x.tobytes() == y.tobytes() == z.tobytes()
        assert a[chrom][2] == b[chrom][2] == c[chrom][2]
    assert bigbed.chroms(path_of("genes.bb")) == bigbed.chroms(path_of("genes.be.bb")) == {"chrA": 2000, "chrBB": 400}
    with open(path_of("genes.be.bb"), "rb") as f:
        data = f.read()
    assert bigbed.byte_order(data) == ">" and bigbed.byte_order(open(path_of("genes.z.bb"), "rb").read(4)) == "<"
    assert bigbed.is_bigbed(path_of("genes.bb")) and bigbed.chroms(data=data) == {"chrA": 2000, "chrBB": 400}
    assert struct.unpack_from("<I", open(path_of("genes.z.bb"), "rb").read(64), 52)[0] > 0  # uncompress_buf_size: compressed
    for name, entry in FILES.items():
        assert bigbed.chroms(path_of(name)) == entry["chroms"] and bigbed.zoom_reductions(path_of(name)) == entry["reductions"]


def test_records_are_the_writers_and_shared_blocks_are_split():
    import write_bigbed_fixture as W
    from bxmi import bigbed

    for name in ("genes.bb", "hand.bb", "straddle.bb", "long.bb", "zoom.bb"):
        chroms, blocks, _, _, _ = W.FIXTURES[name]
        got = bigbed.read_items_file(path_of(name))
        assert any(len({r[0] for r in block}) > 1 for block in blocks) == (name in ("genes.bb", "hand.bb", "zoom.bb"))  # a block of two chromosomes
        for chrom_id, (chrom, _) in enumerate(chroms):
            mine = [r for block in blocks for r in block if r[0] == chrom_id]
            s, e, rest = got[chrom]
            assert s.tolist() == [r[1] for r in mine] and e.tolist() == [r[2] for r in mine] and rest == [r[3] for r in mine], (name, chrom)
    s, e, rest = bigbed.read_items_file(path_of("genes.bb"))["chrBB"]
    assert rest[2] == "" and rest[0] == "geneD\t100\t-"  # a record without further columns; tabs kept
    levels = bigbed.read_zoom_file(path_of("zoom.bb"))
    assert [r for r, _ in levels] == [16, 64] and [len(per["chrZ"].start) for _, per in levels] == [120, 60] and len(levels[0][1]["chrY"].start) == 9
    assert bigbed.read_zoom_file(path_of("genes.bb")) == []


def test_what_is_not_a_whole_bigbed_file_raises_value_error(tmp_path):
    from bxmi import bigbed

    with open(path_of("genes.bb"), "rb") as f:
        data = f.read()
    wig = os.path.join(GOLDEN, "..", "profile", "bg.bw")
    with pytest.raises(ValueError, match="a bigWig file, not a bigBed file"):
        bigbed.read_items_file(wig)
    with pytest.raises(ValueError, match="a bigWig file, not a bigBed file"):
        bigbed.chroms(wig)
    assert not bigbed.is_bigbed(wig)
    cases = {"bad magic": b"\x00\x01\x02\x03" + data[4:], "two bytes": data[:2], "half a header": data[:40], "no index": data[:len(data) - 40],
             "no data": data[:200], "text": b"chr1\t0\t10\n"}
    for what, blob in cases.items():
        path = tmp_path / "case.bb"
        path.write_bytes(blob)
        with pytest.raises(ValueError):
            bigbed.read_items_file(str(path))
        with pytest.raises(ValueError):
            bigbed.read_items_file(data=blob)
    with pytest.raises(ValueError, match="bad magic"):
        bigbed.chroms(data=cases["bad magic"])
    with open(path_of("genes.z.bb"), "rb") as f:
        packed = bytearray(f.read())
    first = struct.unpack_from("<Q", packed, struct.unpack_from("<Q", packed, 24)[0] + 48 + 4 + 16)[0]  # the first leaf entry's block
    packed[first + 4] ^= 0xFF
    with pytest.raises(ValueError):
        bigbed.read_items_file(data=bytes(packed))


def test_records_the_device_cannot_hold_and_unlisted_chromosomes_raise(tmp_path):
    import write_bigbed_fixture as W
    from bxmi import bigbed

    path = str(tmp_path / "far.bb")
    W.write_bigbed(path, [("chrA", 100)], [[(0, 5, 2 ** 31, "far")]])
    with pytest.raises(ValueError, match="beyond 2\\^31 - 1"):
        bigbed.read_items_file(path)
    W.write_bigbed(path, [("chrA", 100)], [[(0, 5, 2 ** 31 - 1, "near")]])
    assert bigbed.read_items_file(path)["chrA"][1].tolist() == [2 ** 31 - 1]
    W.write_bigbed(path, [("chrA", 100)], [[(0, 5, 9, "mine"), (3, 1, 2, "whose")]], compress=True)
    with pytest.raises(ValueError, match="chromosome id 3"):
        bigbed.read_items_file(path)


def test_bigwig_still_refuses_bigbed():
    from bxmi import bigwig

    for name in ("genes.bb", "genes.be.bb", "zoom.bb"):
        assert not bigwig.is_bigwig(path_of(name))
        for read in (bigwig.chroms, bigwig.read_spans_file, bigwig.zoom_reductions, bigwig.read_zoom_file):
            with pytest.raises(ValueError, match="a bigBed file, not a bigWig file"):
                read(path_of(name))
