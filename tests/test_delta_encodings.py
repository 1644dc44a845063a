"""DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and BYTE_STREAM_SPLIT data pages (k_delta_lengths,
k_dlba_copy, k_dba_tail / k_dba_link / k_dba_expand, k_bss_gather) against their PLAIN twin.

The oracle decoder (oracle/dk_ref.c) does not read these encodings, so every table is written twice
with pyarrow: PLAIN (held to the oracle, as everywhere) and with column_encoding. The encoded file
must then decode to byte-identical columns (ParquetSet.column) and identical ParquetReader batches,
and both must equal what pyarrow reads back. Floats are compared by their bits.

Reference: parquet-mr 1.12.3's DeltaLengthByteArrayValuesReader, DeltaByteArrayReader and
ByteStreamSplitValuesReader behind ParquetColumnReaders (kernel-defaults).
"""
import os
import struct

import numpy as np
import pyarrow as pa
import pyarrow.compute  # noqa: F401  (pa.compute)
import pyarrow.parquet as pq
import pytest

from oracle import ref
from tests.test_reader import _assert_leaf, _concat

pytestmark = pytest.mark.gpu

DLBA, DBA, BSS = "DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY", "BYTE_STREAM_SPLIT"
VARIANTS = [("1.0", "none"), ("2.0", "none"), ("1.0", "snappy"), ("2.0", "snappy")]
FIELDS = ("row_def", "row_offs", "entry_def", "fixed", "offs", "chars")


@pytest.fixture(scope="module")
def engine():
    from delta_amd import kernel as K
    eng = K.GpuEngine(parquet_batch_size=1000)
    yield eng
    eng.close()


def _leaves(schema, prefix=""):
    out = []
    for f in schema:
        if pa.types.is_struct(f.type):
            out += _leaves(f.type, prefix + f.name + ".")
        else:
            out.append(prefix + f.name)
    return out


def _write_twins(tmp_path, table, encoding, version, compression, **kw):
    """The table PLAIN and with `encoding` ({leaf: encoding}); returns (plain path, encoded path)."""
    base = dict(use_dictionary=False, compression=compression, data_page_version=version, write_statistics=False)
    if "max_rows_per_page" in kw:
        base["write_batch_size"] = kw["max_rows_per_page"]   # pages are cut between write batches
    base.update(kw)
    plain, enc = str(tmp_path / "plain.parquet"), str(tmp_path / "enc.parquet")
    pq.write_table(table, plain, **base)
    pq.write_table(table, enc, column_encoding=encoding, **base)
    md = pq.ParquetFile(enc).metadata
    for g in range(md.num_row_groups):
        for i in range(md.num_columns):
            c = md.row_group(g).column(i)
            if c.path_in_schema in encoding:
                assert encoding[c.path_in_schema] in c.encodings, (c.path_in_schema, c.encodings)
    return plain, enc


def _pylist(col, arrow_type):
    """A decoded non-repeated column as Python values (bytes / bit patterns / None)."""
    valid = col.row_def == col.max_def
    out = []
    if col.phys == 6:
        for i, ok in enumerate(valid):
            out.append(bytes(col.chars[col.offs[i]:col.offs[i + 1]]) if ok else None)
        return out
    bits = col.fixed.view({4: np.uint32, 8: np.uint64}[col.width])
    return [int(bits[i]) if ok else None for i, ok in enumerate(valid)]


def _arrow_pylist(arr):
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    t = arr.type
    if pa.types.is_floating(t):
        w = np.uint32 if t == pa.float32() else np.uint64
        vals = arr.fill_null(0).to_numpy(zero_copy_only=False).view(w)   # fill_null keeps the other bits
        return [int(v) if ok else None for v, ok in zip(vals, arr.is_valid().to_pylist())]
    return [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in arr.to_pylist()]


def _arrow_leaf(table, leaf):
    parts = leaf.split(".")
    arr = table.column(parts[0]).combine_chunks()
    for p in parts[1:]:
        valid = arr.is_valid()
        child = arr.field(p)
        arr = pa.compute.if_else(valid, child, pa.nulls(len(child), child.type))
    return arr


def _check_twins(engine, table, plain, enc):
    from delta_amd import kernel as K
    leaves = _leaves(table.schema)
    back = pq.read_table(enc)
    ps = K.ParquetSet(engine, [plain, enc], leaves).decode()
    try:
        for leaf in leaves:
            a, b = ps.column(0, leaf), ps.column(1, leaf)
            for f in FIELDS:
                x, y = getattr(a, f), getattr(b, f)
                assert (x is None) == (y is None), (leaf, f)
                if x is not None:
                    np.testing.assert_array_equal(y, x, err_msg="%s %s" % (leaf, f))
            if a.max_rep == 0:
                assert _pylist(b, None) == _arrow_pylist(_arrow_leaf(back, leaf)), leaf
    finally:
        ps.close() if hasattr(ps, "close") else None
    with engine.readParquetFiles([plain, enc], leaves, window_rows=0) as rd:
        batches = list(rd)
    by_file = {0: [], 1: []}
    for bt in batches:
        by_file[bt.file].append(bt)
    pf = ref.ParquetFile.open(plain)
    for leaf in leaves:
        want = pf.read(leaf)
        got = [_concat(by_file[k], leaf) for k in (0, 1)]
        _assert_leaf(got[0], want, leaf)          # the PLAIN twin against the oracle
        _assert_leaf(got[1], want, leaf)          # and the encoded file gives the same batches


def _path_values(n):
    """Sorted path-like strings: 1,000 consecutive values share a 40-byte prefix; a value equal to its
    predecessor, a strict prefix of its predecessor, and values sharing nothing (prefix 0 mid-page)."""
    out = []
    for i in range(n):
        out.append("date=2024-%02d-01/region=%08d/part-%05d-%s.c000.snappy.parquet"
                   % (1 + i // 1000 % 12, i // 1000, i, "abcdefghij"[: i % 11]))
    out[501] = out[500]                       # empty suffix
    out[701] = out[700][:25]                  # strict prefix of its predecessor
    out[900] = "zz-no-shared-prefix"          # prefix 0 in the middle of a page
    out[901] = "another/start"
    return out


def _length_values(kind, n, rng):
    if kind == "equal":                        # every delta 0: bit width 0
        return ["v%07d" % i for i in range(n)]
    if kind == "empty":
        return [""] * n
    if kind == "wide":                         # 0 .. 70,000 bytes in one page: wide miniblocks, a value
        out = []                               # longer than any LDS tile
        for i in range(n):
            r = i % 97
            ln = 70_000 if r == 13 else 0 if r in (0, 50) else 5_000 if r == 60 else int(rng.integers(1, 90))
            out.append(("w%d-" % i + "q" * ln)[:max(ln, 0)] if ln else "")
        # after the long value: values that keep a long prefix of it, one of them all of it
        for i in range(13, n, 97):
            if i + 3 < n:
                out[i + 1] = out[i][:69_000] + "tail"
                out[i + 2] = out[i + 1]
                out[i + 3] = out[i][:3000]
        return out
    raise ValueError(kind)


COUNTS = [1, 2, 128, 129, 130, 385, 1000]      # 130 / 385: the last block needs one of its four miniblocks


@pytest.mark.parametrize("version,compression", VARIANTS)
@pytest.mark.parametrize("encoding", [DLBA, DBA])
def test_value_counts_per_page(tmp_path, engine, encoding, version, compression):
    """Pages of 0 (all null), 1, 2, 128, 129 ... values: the rows are laid out so that with
    max_rows_per_page = 1000 every page holds exactly one of the counts (the rest of the page is null)."""
    vals = []
    for k, cnt in enumerate([0] + COUNTS):
        page = [None] * 1000
        for j in range(cnt):
            page[(j * 7 + k) % 1000 if cnt < 140 else j] = "k%d/value-%04d-%s" % (k, j, "x" * (j % 9))
        vals += page
    t = pa.table({"s": pa.array(vals, pa.string()), "b": pa.array([None if v is None else v.encode() for v in vals], pa.binary())})
    plain, enc = _write_twins(tmp_path, t, {"s": encoding, "b": encoding}, version, compression,
                              max_rows_per_page=1000, data_page_size=1 << 20, row_group_size=4000)
    assert pq.ParquetFile(enc).metadata.num_row_groups == 2
    _check_twins(engine, t, plain, enc)


@pytest.mark.parametrize("version,compression", VARIANTS)
@pytest.mark.parametrize("encoding", [DLBA, DBA])
@pytest.mark.parametrize("kind", ["equal", "empty", "wide"])
def test_lengths(tmp_path, engine, kind, encoding, version, compression):
    rng = np.random.default_rng(7)
    n = 1200
    vals = _length_values(kind, n, rng)
    nulls = [None if i % 3 == 1 else v for i, v in enumerate(vals)]
    inner = pa.StructArray.from_arrays([pa.array(nulls, pa.string())], names=["x"],
                                       mask=pa.array([i % 5 == 0 for i in range(n)]))
    t = pa.table({"s": pa.array(vals, pa.string()), "n": pa.array(nulls, pa.string()), "st": inner})
    plain, enc = _write_twins(tmp_path, t, {"s": encoding, "n": encoding, "st.x": encoding}, version, compression,
                              max_rows_per_page=200, data_page_size=64 << 20, row_group_size=600)
    _check_twins(engine, t, plain, enc)


@pytest.mark.parametrize("version,compression", VARIANTS)
def test_delta_byte_array_chains(tmp_path, engine, version, compression):
    n = 3000
    paths = _path_values(n)
    blob = [bytes([0, 255, 0, 255]) * (1 + i % 5) + struct.pack("<I", i // 7) + (b"\x00" if i % 2 else b"\xff\xff")
            for i in range(n)]
    t = pa.table({"p": pa.array(paths, pa.string()), "raw": pa.array(blob, pa.binary())})
    # 700 rows per page: more than five 128-value blocks, a partial last block, and page 2 starts
    # in the middle of a run of shared prefixes (the chain restarts there)
    plain, enc = _write_twins(tmp_path, t, {"p": DBA, "raw": DBA}, version, compression,
                              max_rows_per_page=700, data_page_size=64 << 20, row_group_size=2100)
    _check_twins(engine, t, plain, enc)


def _floats(n, dtype):
    rng = np.random.default_rng(n)
    if dtype == np.float32:
        special = np.array([0x7FC00001, 0xFFC12345, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001,
                            0x807FFFFF], np.uint32).view(np.float32)
    else:
        special = np.array([0x7FF8000000000001, 0xFFF80000DEADBEEF, 0, 0x8000000000000000, 0x7FF0000000000000,
                            0xFFF0000000000000, 1, 0x800FFFFFFFFFFFFF], np.uint64).view(np.float64)
    v = rng.standard_normal(n).astype(dtype)
    k = min(n, len(special))
    v[:k] = special[:k]
    return v


@pytest.mark.parametrize("version,compression", VARIANTS)
def test_byte_stream_split(tmp_path, engine, version, compression):
    """Pages of 1, 63, 64 and 65 non-null values (and an all-null one), float and double."""
    f4, f8, valid = [], [], []
    for cnt in (0, 1, 63, 64, 65, 100):
        a, b = _floats(cnt, np.float32), _floats(cnt, np.float64)
        page4, page8, ok = np.zeros(100, np.float32), np.zeros(100, np.float64), np.zeros(100, bool)
        idx = np.arange(cnt) if cnt == 100 else (np.arange(cnt) * 3 + 1) % 100 if cnt < 34 else np.arange(cnt)
        page4[idx], page8[idx], ok[idx] = a, b, True
        f4.append(page4); f8.append(page8); valid.append(ok)
    f4, f8, valid = np.concatenate(f4), np.concatenate(f8), np.concatenate(valid)
    t = pa.table({"f": pa.array(f4, pa.float32(), mask=~valid), "d": pa.array(f8, pa.float64(), mask=~valid),
                  "dense": pa.array(_floats(600, np.float64), pa.float64())})
    plain, enc = _write_twins(tmp_path, t, {"f": BSS, "d": BSS, "dense": BSS}, version, compression,
                              max_rows_per_page=100, data_page_size=64 << 20, row_group_size=300)
    _check_twins(engine, t, plain, enc)


# ---- malformed pages, still-refused encodings -----------------------------------------------------

def _clean(tmp_path_factory):
    from delta_amd import synth
    d = str(tmp_path_factory.mktemp("clean"))
    synth.write_table(d, synth.TableSpec(n_adds=2_000, n_commits=2))
    return d


@pytest.fixture(scope="module")
def clean_table(tmp_path_factory):
    return _clean(tmp_path_factory)


def _still_usable(engine, clean_table):
    from tests.parity_util import assert_same, oracle_scan, product_scan
    assert_same(product_scan(clean_table, engine=engine), oracle_scan(clean_table))


def _read_error(engine, path, leaf):
    from delta_amd import kernel as K
    from delta_amd._lib import DkError
    with pytest.raises(DkError) as ei:
        K.ParquetSet(engine, [path], [leaf]).decode()
    return str(ei.value)


def _patch_first_varint(path, leaf, new_bytes):
    """Overwrite the varint after the first DBP header (80 01 04: block 128, 4 miniblocks) behind the
    column's first data page offset: the header's value count stays, the first value changes."""
    md = pq.ParquetFile(path).metadata
    col = next(md.row_group(0).column(i) for i in range(md.num_columns) if md.row_group(0).column(i).path_in_schema == leaf)
    with open(path, "r+b") as f:
        f.seek(col.data_page_offset)
        buf = f.read(4096)
        at = buf.index(b"\x80\x01\x04") + 3
        while buf[at] & 0x80:                  # the value count
            at += 1
        at += 1
        end = at
        while buf[end] & 0x80:                 # the first value (zigzag varint)
            end += 1
        end += 1
        assert len(new_bytes) == end - at, (len(new_bytes), end - at)
        f.seek(col.data_page_offset + at)
        f.write(new_bytes)


@pytest.mark.parametrize("encoding,patch", [(DLBA, b"\xfe\xff\x7f"), (DBA, b"\x06")])
def test_malformed_lengths_are_rejected(tmp_path, engine, clean_table, encoding, patch):
    """A huge first length (DELTA_LENGTH_BYTE_ARRAY) and a non-zero first prefix (DELTA_BYTE_ARRAY):
    the length checks reject the page; nothing is read through such a length."""
    # the patch keeps the varint's size: a 70,000-byte first value has a 3-byte length, rewritten to ~1 MiB
    first = "a" * 70_000 if encoding == DLBA else "first"
    vals = [first] + ["a-value-%d" % i for i in range(300)]
    t = pa.table({"s": pa.array(vals, pa.string())})
    p = str(tmp_path / "bad.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="none", column_encoding={"s": encoding})
    _patch_first_varint(p, "s", patch)
    msg = _read_error(engine, p, "s")
    assert msg.startswith("Error reading Parquet file: " + p) and "bad values" in msg, msg
    _still_usable(engine, clean_table)


def test_still_refused(tmp_path, engine, clean_table):
    import decimal
    dec = pa.array([decimal.Decimal(i) / 100 for i in range(500)], pa.decimal128(20, 2))
    p = str(tmp_path / "flba.parquet")
    pq.write_table(pa.table({"d": dec}), p, use_dictionary=False, compression="none", column_encoding={"d": DBA})
    msg = _read_error(engine, p, "d")
    assert msg.startswith("Error reading Parquet file: " + p) and "unsupported encoding" in msg, msg
    q = str(tmp_path / "i64.parquet")
    try:
        pq.write_table(pa.table({"i": pa.array(range(500), pa.int64())}), q, use_dictionary=False, compression="none",
                       column_encoding={"i": BSS})
    except (pa.ArrowInvalid, pa.ArrowNotImplementedError, OSError) as e:
        pytest.skip("this pyarrow does not write BYTE_STREAM_SPLIT for int64: %s" % e)
    msg = _read_error(engine, q, "i")
    assert msg.startswith("Error reading Parquet file: " + q) and "unsupported encoding" in msg, msg
    _still_usable(engine, clean_table)
