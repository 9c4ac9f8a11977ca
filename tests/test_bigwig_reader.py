"""CPU-only: bxmi.bigwig against what the reference's BigWigFile.get_as_array returned for the same files (tests/golden/profile,
recorded by tools/record_profile_golden.py): spans filled into a NaN array in file order equal every recorded region exactly,
chromosome names and sizes match, both byte orders and all three block kinds are read, compressed or not."""
import os
import struct

import numpy as np
import pytest

import profile_model as M
from test_profile_model_golden import FILES, GOLDEN, MANIFEST, recorded_regions


def dense(path):
    from bxmi import bigwig

    sizes = bigwig.chroms(path)
    spans = bigwig.read_spans_file(path)
    assert list(spans) == list(sizes)
    for s, e, v in spans.values():
        assert s.dtype == np.int32 and e.dtype == np.int32 and v.dtype == np.float32 and len(s) == len(e) == len(v)
    # (the reference's own file has a 247 Mbp chromosome with data below 21 kbp: fill what the spans reach)
    return sizes, {c: M.fill_spans(min(sizes[c], int(spans[c][1].max()) if len(spans[c][1]) else 0), spans[c]) for c in sizes}


@pytest.mark.parametrize("name", sorted(FILES))
def test_spans_fill_to_the_recorded_arrays(name):
    sizes, tracks = dense(os.path.join(GOLDEN, name))
    assert {c: sizes[c] for c in FILES[name]["chroms"]} == FILES[name]["chroms"]
    for (chrom, s, e), want in recorded_regions(name):
        got = M.window(tracks[chrom], s, e - s)
        assert got.tobytes() == want.tobytes(), (name, chrom, s, e)


def test_fixtures_cover_kinds_orders_and_compression():
    """what the fixture files are for, read off their bytes"""
    from bxmi import bigwig

    seen = set()
    for name in FILES:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            data = f.read()
        h = bigwig._Header(data)
        for off, size in bigwig._leaf_blocks(data, h.unzoomed_index_offset):
            block = data[off:off + size]
            if h.uncompress_buf_size:
                import zlib

                block = zlib.decompress(block)
            seen.add((struct.unpack_from(h.order + "B", block, 20)[0], h.order, h.uncompress_buf_size > 0))
    for kind in (bigwig.BEDGRAPH, bigwig.VARIABLE_STEP, bigwig.FIXED_STEP):
        assert any(k == kind and z for k, _, z in seen) and any(k == kind and not z for k, _, z in seen), (kind, seen)
        assert any(k == kind and o == ">" for k, o, _ in seen) and any(k == kind and o == "<" for k, o, _ in seen), (kind, seen)


def test_byte_orders_give_the_same_spans():
    from bxmi import bigwig

    a = bigwig.read_spans_file(os.path.join(GOLDEN, "two.z.bw"))
    b = bigwig.read_spans_file(os.path.join(GOLDEN, "two.be.bw"))
    assert bigwig.chroms(os.path.join(GOLDEN, "two.z.bw")) == bigwig.chroms(os.path.join(GOLDEN, "two.be.bw")) == {"chrA": 100, "chrBB": 50}
    assert list(a) == list(b)
    for c in a:
        for x, y in zip(a[c], b[c]):
            assert x.tobytes() == y.tobytes()


def test_bad_magic_and_bigbed_raise_value_error(tmp_path):
    from bxmi import bigwig

    with open(os.path.join(GOLDEN, "bg.bw"), "rb") as f:
        data = f.read()
    bad = tmp_path / "bad.bw"
    bad.write_bytes(b"\x00\x01\x02\x03" + data[4:])
    bed = tmp_path / "bigbed.bb"
    bed.write_bytes(struct.pack("<I", 0x8789F2EB) + data[4:])
    short = tmp_path / "short.bw"
    short.write_bytes(data[:2])
    text = tmp_path / "scores.wig"
    text.write_text("fixedStep chrom=chr1 start=1 step=1\n1.0\n")
    for p in (bad, bed, short, text):
        assert not bigwig.is_bigwig(str(p))
        with pytest.raises(ValueError):
            bigwig.read_spans_file(str(p))
        with pytest.raises(ValueError):
            bigwig.chroms(str(p))
    with pytest.raises(ValueError, match="bigBed"):
        bigwig.chroms(str(bed))
    assert bigwig.is_bigwig(os.path.join(GOLDEN, "bg.bw")) and bigwig.is_bigwig(os.path.join(GOLDEN, "two.be.bw"))


@pytest.mark.parametrize("twin", MANIFEST["twins"], ids=lambda t: t["bigwig"])
def test_bigwig_and_wiggle_twins_give_the_same_track(twin):
    """test.bw was made from test.wig, bg.wig is written beside bg.bw: the recorder found each pair to be the same track (the
    bigWig through the reference's reader), so the project's two readers must agree span for span after filling"""
    from bxmi import wiggle

    assert twin["same"], "the recorder found different tracks; this test would have to say why"
    _, from_bigwig = dense(os.path.join(GOLDEN, twin["bigwig"]))
    spans = wiggle.read_spans_file(os.path.join(GOLDEN, twin["wiggle"]))
    assert set(spans) == set(from_bigwig)
    for c, (s, e, v) in spans.items():
        t = M.fill_spans(int(e.max()), (s, e, v))
        assert t.tobytes() == from_bigwig[c].tobytes(), c
