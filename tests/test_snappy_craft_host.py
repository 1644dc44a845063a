"""(CPU) The crafted snappy corpus of tests/snappy_craft.py is what it claims to be: the reference
decoder agrees with Google's decoder (pyarrow's codec) on every stream, valid or malformed; the
crafted Parquet files read back through pyarrow.parquet with the intended values; and every case
holds the feature it is named for (inspect / walk). The GPU half is tests/test_snappy_craft.py."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import snappy_craft as sc

VALID = sc.valid_cases()
MALFORMED = sc.malformed_cases()
SNAPPY = pa.Codec("snappy")


def test_builder_refuses_only_what_a_tag_cannot_express():
    for op in (sc.lit(b""), sc.lit(b"x" * 61, 0), sc.lit(b"x" * 257, 1), sc.copy(5, 3, 1), sc.copy(2048, 4, 1),
               sc.copy(5, 12, 1), sc.copy(65536, 4, 2), sc.copy(5, 65, 2), sc.copy(1 << 32, 4, 3), sc.copy(5, 0, 3)):
        with pytest.raises(ValueError):
            sc.encode_op(op)
    assert sc.encode_op(sc.lit(b"abcde", 4)) == b"\xfc\x04\x00\x00\x00abcde"
    assert sc.encode_op(sc.lit(b"x" * 60)) == b"\xec" + b"x" * 60
    assert sc.encode_op(sc.lit(b"x" * 60, 1)) == b"\xf0\x3b" + b"x" * 60
    assert sc.encode_op(sc.copy(0, 4, 3)) == b"\x0f\x00\x00\x00\x00"
    assert sc.varint(64, 3) == b"\xc0\x80\x00" and sc.varint(300) == b"\xac\x02"


def test_reference_reads_googles_encoder():
    rng = np.random.default_rng(5)
    raw = b"".join(bytes([65 + i % 7]) * int(rng.integers(1, 90)) + rng.integers(0, 256, size=int(rng.integers(0, 40)),
                   dtype=np.uint8).tobytes() for i in range(4000))
    comp = SNAPPY.compress(raw, asbytes=True)
    assert sc.decode(comp) == raw
    tags = sc.inspect(comp)
    # what the corpus adds: none of these come out of Google's encoder
    assert not any(t.kind == 3 or (t.kind == 0 and t.form > 2) for t in tags)
    assert len(raw) > 2 * sc.FRAG and sc._fast(tags)


@pytest.mark.parametrize("case", VALID, ids=[c.name for c in VALID])
def test_valid_case(case, tmp_path):
    assert len(case.out) <= 320 * 1024
    assert sc.decode(case.stream) == case.out
    assert SNAPPY.decompress(case.stream, decompressed_size=len(case.out), asbytes=True) == case.out
    tags = sc.inspect(case.stream)
    assert case.check(tags, case.stream), "the case lost the feature it is named for"
    # the serial expectation follows from the tags: a straddling tag or a copy reaching back across a
    # 64 KiB output boundary, and nothing else, sends a page to k_snappy_serial
    assert case.serial == (0 if sc._fast(tags) else 1)
    path = str(tmp_path / "c.parquet")
    sc.write_case(path, case)
    got = pq.read_table(path).column("v").to_numpy()
    assert got.tobytes() == case.out


def test_tiny_file(tmp_path):
    path = str(tmp_path / "t.parquet")
    want = sc.write_tiny(path)
    t = pq.read_table(path)
    assert t.column("v").to_numpy().tobytes() == want["v"]
    assert t.column("s").to_pylist() == want["s"]
    assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "SNAPPY"


@pytest.mark.parametrize("bad", MALFORMED, ids=[b.name for b in MALFORMED])
def test_malformed_case(bad, tmp_path):
    if bad.stream_ok:                      # only the page header disagrees: the stream itself is fine
        assert len(sc.decode(bad.stream)) != bad.usize
    else:
        with pytest.raises(ValueError):
            sc.decode(bad.stream)
        with pytest.raises(Exception):
            SNAPPY.decompress(bad.stream, decompressed_size=max(bad.usize, 64), asbytes=True)
    path = str(tmp_path / "m.parquet")
    sc.write_malformed(path, bad)
    with pytest.raises(Exception):
        pq.read_table(path)


def test_malformed_files_are_good_up_to_the_bad_page(tmp_path):
    """The same two-page layout with a good second page reads: the bad page alone fails a file."""
    good = sc.Bad("good", sc.build([sc.lit(bytes(range(16)))], 16), 16, True)
    path = str(tmp_path / "g.parquet")
    sc.write_malformed(path, good)
    assert pq.read_table(path).num_rows == 18
