"""ZSTD-compressed Parquet pages (k_zstd_page, delta_amd/csrc/dk_zstd.hip) against their uncompressed
or snappy twin: the same table written twice must decode to byte-identical columns, and to what
pyarrow reads back. Before this decoder existed every zstd file failed at prepare() with
"unsupported compression codec 6".

Malformed pages use only damage the sanitised host program (tests/test_zstd_host.py) has run clean.
"""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import zstd_inspect
from tests.test_delta_encodings import FIELDS, _arrow_leaf, _arrow_pylist, _pylist

pytestmark = pytest.mark.gpu
MAGIC = b"\x28\xb5\x2f\xfd"


@pytest.fixture(scope="module")
def engine():
    from delta_amd import kernel as K
    eng = K.GpuEngine(parquet_batch_size=1000)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def clean_table(tmp_path_factory):
    from delta_amd import synth
    d = str(tmp_path_factory.mktemp("clean"))
    synth.write_table(d, synth.TableSpec(n_adds=2_000, n_commits=2))
    return d


def _still_usable(engine, clean_table):
    from tests.parity_util import assert_same, oracle_scan, product_scan
    assert_same(product_scan(clean_table, engine=engine), oracle_scan(clean_table))


def _small_table(n=2000):
    rng = np.random.default_rng(5)
    s = ["row-%05d/%s" % (i, "abcdefghij"[: i % 11]) if i % 7 else None for i in range(n)]
    inner = pa.StructArray.from_arrays(
        [pa.array([i * 3 if i % 4 else None for i in range(n)], pa.int64()), pa.array(["x%d" % (i % 50) for i in range(n)], pa.string())],
        names=["a", "b"], mask=pa.array([i % 9 == 0 for i in range(n)]))
    m = pa.array([[("k%d" % j, "v%d-%d" % (i, j) if j % 2 else None) for j in range(i % 4)] if i % 13 else None for i in range(n)],
                 pa.map_(pa.string(), pa.string()))
    return pa.table({
        "l": pa.array(rng.integers(-1 << 40, 1 << 40, n), pa.int64()), "i": pa.array(np.arange(n, dtype=np.int32) % 300, pa.int32()),
        "s": pa.array(s, pa.string()), "d": pa.array(rng.standard_normal(n), pa.float64()),
        "b": pa.array([bool(i % 3) if i % 10 else None for i in range(n)], pa.bool_()), "st": inner, "m": m})


LEAVES = ["l", "i", "s", "d", "b", "st.a", "st.b", "m.key_value.key", "m.key_value.value"]


def _got(col):
    """A decoded non-repeated column as Python values: bytes, or the bit pattern of a fixed-width value."""
    if col.phys == 6:
        return _pylist(col, None)
    valid = col.row_def == col.max_def
    bits = col.fixed.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[col.width])
    return [int(bits[i]) if ok else None for i, ok in enumerate(valid)]


def _want(arr):
    t = arr.type
    if pa.types.is_integer(t):
        mask = (1 << t.bit_width) - 1
        return [None if v is None else v & mask for v in arr.to_pylist()]
    if pa.types.is_boolean(t):
        return [None if v is None else int(v) for v in arr.to_pylist()]
    return _arrow_pylist(arr)


def _compare(engine, paths, leaves, table=None):
    """Every file of `paths` decodes to the same columns as the first; non-repeated leaves also equal `table`."""
    from delta_amd import kernel as K
    ps = K.ParquetSet(engine, paths, leaves).decode()
    try:
        for leaf in leaves:
            a = ps.column(0, leaf)
            for k in range(1, len(paths)):
                b = ps.column(k, leaf)
                for f in FIELDS:
                    x, y = getattr(a, f), getattr(b, f)
                    assert (x is None) == (y is None), (leaf, f)
                    if x is not None:
                        np.testing.assert_array_equal(y, x, err_msg="%s %s file %d" % (leaf, f, k))
                if table is not None and a.max_rep == 0:
                    assert _got(b) == _want(_arrow_leaf(table, leaf)), leaf
    finally:
        ps.close() if hasattr(ps, "close") else None


def _codecs(path):
    md = pq.ParquetFile(path).metadata
    return {md.row_group(0).column(i).path_in_schema: md.row_group(0).column(i).compression for i in range(md.num_columns)}


@pytest.mark.parametrize("level", [1, 3, 19])
@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_twins(tmp_path, engine, version, dictionary, level):
    t = _small_table()
    kw = dict(use_dictionary=dictionary, data_page_version=version, write_statistics=False, data_page_size=16 << 10,
              row_group_size=1200)
    none, z = str(tmp_path / "none.parquet"), str(tmp_path / "zstd.parquet")
    pq.write_table(t, none, compression="none", **kw)
    pq.write_table(t, z, compression="zstd", compression_level=level, **kw)
    assert set(_codecs(z).values()) == {"ZSTD"}
    _compare(engine, [none, z], LEAVES, pq.read_table(z))


def _page_bodies(path, leaf):
    """zstd_inspect's tags of each row group's page body: these files hold one v1 data page per chunk and no
    dictionary page, so the body runs from the frame magic to the end of the chunk."""
    md = pq.ParquetFile(path).metadata
    out = []
    with open(path, "rb") as f:
        for g in range(md.num_row_groups):
            c = next(md.row_group(g).column(i) for i in range(md.num_columns) if md.row_group(g).column(i).path_in_schema == leaf)
            f.seek(c.data_page_offset)
            buf = f.read(c.total_compressed_size)
            out.append(zstd_inspect.inspect(buf[buf.index(MAGIC):]))
    return out


def _words(n, rng):
    words = ["".join(chr(c) for c in rng.integers(97, 123, rng.integers(2, 9))) for _ in range(300)]
    return [" ".join(words[int(rng.zipf(1.3)) % 300] for _ in range(12)) for _ in range(n)]


def test_large_page_has_many_blocks(tmp_path, engine):
    """One string page of ~330 KiB at level 19: several blocks per frame, Treeless literals, Repeat tables."""
    t = pa.table({"s": pa.array(["part-%05d-abcdef-%d.c000.snappy.parquet" % (i, i * 7919) for i in range(8000)], pa.string())})
    kw = dict(use_dictionary=False, write_statistics=False, data_page_size=8 << 20, data_page_version="1.0")
    none, z = str(tmp_path / "none.parquet"), str(tmp_path / "zstd.parquet")
    pq.write_table(t, none, compression="none", **kw)
    pq.write_table(t, z, compression="zstd", compression_level=19, **kw)
    tags = set().union(*_page_bodies(z, "s"))
    assert {"blocks:many", "lit:treeless", "block:compressed"} <= tags, sorted(tags)
    assert any(x.endswith(":repeat") for x in tags), sorted(tags)
    _compare(engine, [none, z], ["s"], pq.read_table(z))


@pytest.mark.parametrize("kind", ["incompressible", "constant", "empty", "one_row"])
def test_page_shapes(tmp_path, engine, kind):
    rng = np.random.default_rng(3)
    if kind == "incompressible":
        col, want = pa.array([rng.bytes(700) for _ in range(400)], pa.binary()), "block:raw"
    elif kind == "constant":
        col, want = pa.array([b"\x00" * 400_000], pa.binary()), "block:rle"
    elif kind == "empty":
        col, want = pa.array([""] * 3000, pa.string()), None
    else:
        col, want = pa.array(["only"], pa.string()), None
    t = pa.table({"s": col})
    kw = dict(use_dictionary=False, write_statistics=False, data_page_size=8 << 20, data_page_version="1.0")
    none, z = str(tmp_path / "none.parquet"), str(tmp_path / "zstd.parquet")
    pq.write_table(t, none, compression="none", **kw)
    pq.write_table(t, z, compression="zstd", **kw)
    if want:
        tags = set().union(*_page_bodies(z, "s"))
        assert want in tags, sorted(tags)
    _compare(engine, [none, z], ["s"], pq.read_table(z))


def test_mixed_codecs_in_one_file(tmp_path, engine):
    n = 3000
    t = pa.table({"a": pa.array(["alpha-%d" % (i % 97) for i in range(n)]), "b": pa.array(["beta-%d" % (i * 7) for i in range(n)]),
                  "c": pa.array(np.arange(n, dtype=np.int64))})
    kw = dict(use_dictionary=False, write_statistics=False)
    none, mix = str(tmp_path / "none.parquet"), str(tmp_path / "mix.parquet")
    pq.write_table(t, none, compression="none", **kw)
    pq.write_table(t, mix, compression={"a": "snappy", "b": "zstd", "c": "none"}, **kw)
    assert _codecs(mix) == {"a": "SNAPPY", "b": "ZSTD", "c": "UNCOMPRESSED"}
    _compare(engine, [none, mix], ["a", "b", "c"], pq.read_table(mix))


def test_scan_over_zstd_checkpoint(tmp_path, engine):
    """getScanFiles over a zstd checkpoint with a JSON tail: the selected rows and the 5 counters of its
    snappy twin."""
    from delta_amd import synth
    from tests.parity_util import product_scan
    got = {}
    for codec in ("snappy", "zstd"):
        d = str(tmp_path / codec)
        synth.write_table(d, synth.TableSpec(n_adds=4_000, n_commits=13, compression=codec))
        ck = [f for f in os.listdir(os.path.join(d, "_delta_log")) if f.endswith(".checkpoint.parquet")]
        assert ck, "the table has a checkpoint"
        assert set(_codecs(os.path.join(d, "_delta_log", ck[0])).values()) == {codec.upper()}
        got[codec] = product_scan(d, engine=engine)
    assert got["zstd"][0] == got["snappy"][0]
    assert got["zstd"][2] == got["snappy"][2], ("counters", got["zstd"][2], got["snappy"][2])
    assert [r[:-1] for r in got["zstd"][1]] == [r[:-1] for r in got["snappy"][1]]
    assert len(got["zstd"][1]) > 0


# ---- malformed pages ---------------------------------------------------------------------------------

def _read_error(engine, path, leaf):
    from delta_amd import kernel as K
    from delta_amd._lib import DkError
    with pytest.raises(DkError) as ei:
        K.ParquetSet(engine, [path], [leaf]).decode()
    return str(ei.value)


def _zstd_file(tmp_path, n=4000):
    rng = np.random.default_rng(2)
    p = str(tmp_path / "bad.parquet")
    pq.write_table(pa.table({"s": pa.array(_words(n, rng), pa.string())}), p, use_dictionary=False, compression="zstd",
                   write_statistics=False, data_page_size=8 << 20, data_page_version="1.0")
    md = pq.ParquetFile(p).metadata.row_group(0).column(0)
    with open(p, "rb") as f:
        f.seek(md.data_page_offset)
        buf = f.read(md.total_compressed_size)
    at = buf.find(MAGIC)
    return p, md.data_page_offset + at, len(buf) - at       # the frame's file offset and length


@pytest.mark.parametrize("damage", ["middle", "truncated", "magic", "dictionary_id"])
def test_malformed_frame(tmp_path, engine, clean_table, damage):
    if damage == "dictionary_id":
        # a 2-byte Frame_Content_Size (256 .. 65,791 bytes) has room for a window descriptor and a
        # 1-byte Dictionary_ID in its place
        p, at, n = _zstd_file(tmp_path, n=300)
        with open(p, "r+b") as f:
            f.seek(at + 4)
            assert f.read(1) == b"\x60", "single segment, 2-byte content size"
            f.seek(at + 4)
            f.write(bytes([0x01, 0x58, 0x07]))
        want = "unsupported encoding/codec"
    else:
        p, at, n = _zstd_file(tmp_path)
        with open(p, "r+b") as f:
            if damage == "middle":
                f.seek(at + n // 2)
                f.write(b"\xa5" * 64)
            elif damage == "truncated":           # the header's compressed_page_size stays: the frame's tail is zeros
                f.seek(at + n - n // 3)
                f.write(bytes(n // 3))
            else:
                f.seek(at)
                f.write(b"\x29")
        want = "bad zstd frame at offset"
    msg = _read_error(engine, p, "s")
    assert msg.startswith("Error reading Parquet file: " + p) and want in msg, msg
    _still_usable(engine, clean_table)
