"""Data rows filtered on the GPU (dk_data_scan_open / GpuScan.readData): deletion vector AND data filter
per row on the device, only the survivors emitted. Every case writes its files with pyarrow, reads them
back with pyarrow, applies tests/data_filter_oracle.py (a restatement of the reference's evaluator) and
compares exactly: emitted file rows (row_index), values, nulls and batch boundaries."""
import ctypes
import json
import math
import os
import struct
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from delta_amd.expressions import And, Column, Literal, Or, Predicate
from tests import data_filter_oracle as O
from tests.test_dv import _portable, _uuid_z85, _write_dv
from tests.txn_domain_tables import write_commit

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ---- helpers ---------------------------------------------------------------------------------------------
def ktype(t):
    if pa.types.is_decimal(t):
        return "decimal(%d,%d)" % (t.precision, t.scale)
    if pa.types.is_timestamp(t):
        return "timestamp" if t.tz else "timestamp_ntz"
    for name, test in (("byte", pa.types.is_int8), ("short", pa.types.is_int16), ("integer", pa.types.is_int32),
                       ("long", pa.types.is_int64), ("float", pa.types.is_float32), ("double", pa.types.is_float64),
                       ("boolean", pa.types.is_boolean), ("string", pa.types.is_string), ("binary", pa.types.is_binary),
                       ("date", pa.types.is_date32)):
        if test(t):
            return name
    return None


def raw_values(col):
    """A pyarrow column as the values the evaluator sees: ints for dates (days) and timestamps (micros)."""
    t = col.type
    if pa.types.is_timestamp(t):
        per = {"s": 1_000_000, "ms": 1000, "us": 1, "ns": 1}[t.unit]
        v = col.cast(pa.int64()).to_pylist()
        return [None if x is None else (x // 1000 if t.unit == "ns" else x * per) for x in v]
    if pa.types.is_date32(t):
        return col.cast(pa.int32()).to_pylist()
    return col.to_pylist()


def flatten(table):
    """{leaf path tuple: (Kernel type, raw values)} of the primitive leaves (structs flattened)."""
    out = {}

    def walk(prefix, arr):
        t = arr.type
        if pa.types.is_struct(t):
            arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
            valid = arr.is_valid().to_pylist()
            for i in range(t.num_fields):
                k = prefix + (t.field(i).name,)
                walk(k, arr.field(i))
                for kk in [x for x in out if x[:len(k)] == k]:     # a null struct: its fields are null
                    out[kk] = (out[kk][0], [v if ok else None for v, ok in zip(out[kk][1], valid)])
        elif ktype(t) is not None:
            out[prefix] = (ktype(t), raw_values(arr))
    for name in table.column_names:
        walk((name,), table.column(name))
    return out


def expected_rows(path, pred, deleted=(), extra_types=None):
    """File rows the reference keeps: not deleted, and the predicate TRUE (oracle over pyarrow's read)."""
    t = pq.read_table(path)
    leaves = flatten(t)
    types = {k: v[0] for k, v in leaves.items()}
    types.update(extra_types or {})
    deleted = set(deleted)
    keep = []
    for r in range(t.num_rows):
        row = {k: v[1][r] for k, v in leaves.items()}
        keep.append(O.keep(pred, row, types, existing=r not in deleted))
    return np.array(keep, dtype=bool), leaves


def cell(v):
    """A comparable form of one value (floats by their bits: NaN and -0.0 compare exactly)."""
    if isinstance(v, float):
        return ("f", struct.pack("<d", v))
    if isinstance(v, str):
        return v.encode()
    return v


def column_values(c, ktyp):
    """A BatchColumn of a non-repeated leaf as raw values."""
    n = c.n_rows
    if not c.present:
        return [None] * n
    valid = c.validity
    if c.phys == 6:
        vals = [bytes(c.chars[c.offs[i]:c.offs[i + 1]]) for i in range(n)]
    else:
        dt = {(1, 0): np.uint8, (4, 1): "<i4", (8, 2): "<i8", (4, 4): "<f4", (8, 5): "<f8"}[(c.width, c.phys)]
        arr = c.fixed.view(dt)
        vals = [float(x) if c.phys in (4, 5) else int(x) for x in arr]
        if ktyp == "boolean":
            vals = [bool(x) for x in vals]
        if ktyp and ktyp.startswith("decimal"):
            s = int(ktyp.split(",")[1].rstrip(")"))
            vals = [Decimal(x).scaleb(-s) for x in vals]
    return [cell(v) if ok else None for v, ok in zip(vals, valid)]


def read_all(eng, paths, leaves, schema, pred, **kw):
    from delta_amd import kernel as K, programs
    prog = programs.compile_data_filter(pred, schema) if pred is not None else None
    with K.DataReader(eng, paths, leaves, filter=prog, **kw) as rd:
        batches = list(rd)
        stats = rd.stats()
    return batches, stats


def schema_of(table, extra=()):
    def typ(t):
        if pa.types.is_struct(t):
            return {"type": "struct", "fields": [{"name": t.field(i).name, "type": typ(t.field(i).type), "nullable": True,
                                                  "metadata": {}} for i in range(t.num_fields)]}
        if pa.types.is_map(t):
            return {"type": "map", "keyType": typ(t.key_type), "valueType": typ(t.item_type), "valueContainsNull": True}
        return ktype(t)
    fields = [{"name": f.name, "type": typ(f.type), "nullable": True, "metadata": {}} for f in table.schema]
    fields += [{"name": n, "type": t, "nullable": True, "metadata": {}} for n, t in extra]
    return {"type": "struct", "fields": fields}


def check(eng, paths, leaves, pred, *, deleted=None, schema=None, extra=(), compact=True, batch_rows=None, pruned=None, **kw):
    """Run the reader and compare everything with the oracle. deleted: {file index: deleted file rows};
    pruned: {file index: file rows the row-group predicate removed}."""
    deleted, pruned = deleted or {}, pruned or {}
    schema = schema or schema_of(pq.read_table(paths[0]), extra)
    batches, stats = read_all(eng, paths, leaves, schema, pred, compact=compact, batch_rows=batch_rows, **kw)
    B = batch_rows or 1024
    for fi, path in enumerate(paths):
        keep, cols = expected_rows(path, pred, deleted.get(fi, ()), {(n,): t for n, t in extra})
        rows = np.array([r for r in range(len(keep)) if r not in set(pruned.get(fi, ()))], dtype=np.int64)
        mine = [b for b in batches if b.file_index == fi]
        want_rows = rows[keep[rows]] if compact else rows
        if not len(want_rows):
            assert mine == [], "a file without an emitted row yields no batch"
            continue
        got_rows = np.concatenate([b.row_index for b in mine])
        np.testing.assert_array_equal(got_rows, want_rows)
        if compact:
            assert all(b.selection is None for b in mine)
            assert [b.size for b in mine[:-1]] == [B] * (len(mine) - 1) and 0 < mine[-1].size <= B
        else:
            np.testing.assert_array_equal(np.concatenate([b.selection for b in mine]), keep[rows])
            assert all(0 < b.size <= B for b in mine)
        for leaf in leaves:
            key = tuple(leaf.split("."))
            if key not in cols:
                continue                                     # a repeated leaf: checked by its test
            kt, vals = cols[key]
            got = [v for b in mine for v in column_values(b.columns[leaf], kt)]
            assert got == [cell(vals[r]) for r in want_rows], leaf
    return batches, stats


@pytest.fixture(scope="module")
def eng():
    from delta_amd import kernel as K
    return K.GpuEngine()


def write(tmp_path, name, table, **kw):
    p = str(tmp_path / name)
    pq.write_table(table, p, **kw)
    return p


def make_dv(tmp_path, rows, tag=0):
    """A 'u' deletion vector over the given rows (array containers); its descriptor tuple."""
    u = bytes(range(16 * tag, 16 * tag + 16))
    conts = {}
    for r in sorted(rows):
        conts.setdefault(r >> 16, []).append(r & 0xFFFF)
    payload = _portable({0: {k: ("array", v) for k, v in conts.items()}})
    h = u.hex()
    d = tmp_path / "dv"
    d.mkdir(exist_ok=True)
    off = _write_dv(str(d / ("deletion_vector_%s-%s-%s-%s-%s.bin" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:]))), payload)
    return ("u", "dv" + _uuid_z85(u), off, len(payload), len(rows))


# ---- edge positions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_edge_positions(eng, tmp_path, n):
    p = write(tmp_path, "e.parquet", pa.table({"id": pa.array(range(n), pa.int64()), "s": ["v%d" % i for i in range(n)]}))
    for pred in (Predicate("=", Column("id"), Literal.ofLong(0)), Predicate("=", Column("id"), Literal.ofLong(n - 1)),
                 Predicate("<", Column("id"), Literal.ofLong(0)), Predicate(">=", Column("id"), Literal.ofLong(0))):
        check(eng, [p], ["id", "s"], pred)


# ---- types ---------------------------------------------------------------------------------------------
def _typed_table(n=300):
    rng = np.random.default_rng(7)
    f = rng.normal(size=n)
    special = [NAN, math.inf, -math.inf, 0.0, -0.0, 1.5, -1.5]
    for i, v in enumerate(special):
        f[i * 3 + 1] = v
    nul = lambda vals, k: [None if i % k == 0 else v for i, v in enumerate(vals)]
    ts = [1_600_000_000_000_000 + 1000 * int(x) for x in rng.integers(-5000, 5000, n)]
    return pa.table({
        "b8": pa.array(nul([int(x) for x in rng.integers(-128, 128, n)], 11), pa.int8()),
        "i16": pa.array(nul([int(x) for x in rng.integers(-3000, 3000, n)], 13), pa.int16()),
        "i32": pa.array(nul([int(x) for x in rng.integers(-10 ** 6, 10 ** 6, n)], 7), pa.int32()),
        "i64": pa.array(nul([int(x) for x in rng.integers(-10 ** 12, 10 ** 12, n)], 5), pa.int64()),
        "dt": pa.array(nul([int(x) for x in rng.integers(0, 20000, n)], 9), pa.date32()),
        "bo": pa.array(nul([bool(x) for x in rng.integers(0, 2, n)], 6), pa.bool_()),
        "s": pa.array(nul(["k%03d" % (x % 40) if x % 17 else "é%d" % x for x in range(n)], 8), pa.string()),
        "bin": pa.array(nul([bytes([x % 256, (x * 7) % 256]) for x in range(n)], 10), pa.binary()),
        "f32": pa.array(nul([float(np.float32(x)) for x in f], 14), pa.float32()),
        "f64": pa.array(nul([float(x) for x in f], 15), pa.float64()),
        "d9": pa.array(nul([Decimal(int(x)).scaleb(-2) for x in rng.integers(-10 ** 8, 10 ** 8, n)], 12), pa.decimal128(9, 2)),
        "d18": pa.array(nul([Decimal(int(x)).scaleb(-4) for x in rng.integers(-10 ** 17, 10 ** 17, n)], 4), pa.decimal128(18, 4)),
        "ts": pa.array(nul(ts, 16), pa.timestamp("us", tz="UTC")),
        "ntz": pa.array(nul(ts, 18), pa.timestamp("us")),
        "st": pa.array([None if i % 19 == 0 else {"x": None if i % 5 == 0 else i % 50} for i in range(n)],
                       pa.struct([("x", pa.int32())])),
    })


TYPE_CASES = [
    Predicate(">", Column("b8"), Literal.ofByte(3)),
    Predicate("<=", Column("i16"), Literal.ofShort(-7)),
    Predicate(">", Column("i32"), Literal.ofInt(1000)),
    Predicate("<", Column("i32"), Literal.ofLong(1000)),                 # integer column widened to long
    Predicate(">=", Column("i64"), Literal.ofLong(12345)),
    Predicate("<", Column("dt"), Literal.ofDate(10000)),
    Predicate("=", Column("bo"), Literal.ofBoolean(True)),
    Predicate(">", Column("s"), Literal.ofString("k020")),
    Predicate(">=", Column("s"), Literal.ofString("é")),
    Predicate("<", Column("bin"), Literal(b"\x80", "binary")),
    Predicate("<", Column("f32"), Literal.ofFloat(0.25)),
    Predicate("=", Column("f32"), Literal.ofFloat(NAN)),
    Predicate("<", Column("f32"), Literal.ofFloat(0.0)),                 # -0.0 < 0.0, -Inf
    Predicate(">=", Column("f64"), Literal.ofDouble(-0.0)),
    Predicate(">", Column("f64"), Literal.ofDouble(math.inf)),           # only NaN
    Predicate("<", Column("f32"), Literal.ofDouble(0.1)),                # float widened to double
    Predicate(">", Column("d9"), Literal.ofDecimal("12.50", 9, 2)),
    Predicate("<=", Column("d18"), Literal.ofDecimal("0", 18, 4)),
    Predicate(">", Column("ts"), Literal.ofTimestamp(1_600_000_000_000_000)),
    Predicate("<", Column("ntz"), Literal.ofTimestampNtz(1_600_000_000_000_000)),
    Predicate("<", Column("i64"), Column("f64")),                        # column to column: long < double
    Predicate("IS_NULL", Column("i64")),                                 # a nullable column
    Predicate("NOT", Predicate(">", Column("i64"), Literal.ofLong(0))),
    Predicate("=", Column("st", "x"), Literal.ofInt(7)),                 # a nested struct field
    Predicate("IS_NULL", Column("st", "x")),
    Or(Predicate("IS_NULL", Column("s")), And(Predicate(">", Column("i32"), Literal.ofInt(0)),
                                             Predicate("IS NOT DISTINCT FROM", Column("bo"), Literal.ofNull("boolean")))),
]
VARIANTS = {"dict": dict(use_dictionary=True, compression="none"), "plain": dict(use_dictionary=False, compression="none"),
            "snappy": dict(use_dictionary=True, compression="snappy")}


@pytest.fixture(scope="module")
def typed_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("typed")
    t = _typed_table()
    return {k: write(d, k + ".parquet", t, store_decimal_as_integer=True, **kw) for k, kw in VARIANTS.items()}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_types(eng, typed_files, variant):
    leaves = ["i64", "s", "f32", "f64", "d9", "bo", "st.x"]
    for pred in TYPE_CASES:
        check(eng, [typed_files[variant]], leaves, pred)


def test_timestamp_millis_and_int96(eng, tmp_path):
    n = 100
    us = [1_600_000_000_000_000 + 1_000 * i for i in range(n)]
    t = pa.table({"ts": pa.array(us, pa.timestamp("us", tz="UTC")), "id": pa.array(range(n), pa.int64())})
    ms = write(tmp_path, "ms.parquet", t, coerce_timestamps="ms")
    i96 = write(tmp_path, "i96.parquet", t, use_deprecated_int96_timestamps=True)
    pred = Predicate(">=", Column("ts"), Literal.ofTimestamp(us[40]))
    for p in (ms, i96):
        schema = {"type": "struct", "fields": [{"name": "ts", "type": "timestamp", "nullable": True, "metadata": {}},
                                               {"name": "id", "type": "long", "nullable": True, "metadata": {}}]}
        batches, _ = read_all(eng, [p], ["id"], schema, pred)
        np.testing.assert_array_equal(np.concatenate([b.row_index for b in batches]), np.arange(40, n))


def test_missing_column_is_null_everywhere(eng, tmp_path):
    p = write(tmp_path, "m.parquet", pa.table({"id": pa.array(range(70), pa.int64())}))
    extra = [("gone", "integer")]
    b, _ = check(eng, [p], ["id"], Predicate("IS_NULL", Column("gone")), extra=extra)
    assert sum(x.size for x in b) == 70
    b, _ = check(eng, [p], ["id"], Predicate("=", Column("gone"), Literal.ofInt(1)), extra=extra)
    assert b == []


# ---- deletion vectors --------------------------------------------------------------------------------------
def test_deletion_vectors(eng, tmp_path):
    from delta_amd import kernel as K
    n = 1000
    t = pa.table({"id": pa.array(range(n), pa.int64()), "v": pa.array([i % 10 for i in range(n)], pa.int32())})
    a, b = write(tmp_path, "a.parquet", t), write(tmp_path, "b.parquet", t)
    gone = [0, n - 1] + list(range(400, 470))
    big = [5, 999, 1500, 70000]                               # larger than the file
    dvs = K.DeletionVectors(eng, "file:" + str(tmp_path), [make_dv(tmp_path, gone, 1), make_dv(tmp_path, big, 2)])
    for k, rows in enumerate((gone, big)):                    # the bitmaps the kernel reads
        assert set(np.nonzero(dvs.deleted(k))[0].tolist()) == set(rows)
    pred = Predicate("<", Column("v"), Literal.ofInt(5))
    check(eng, [a], ["id"], None, deleted={0: gone}, dvs=dvs, dv_index=[0])                  # a DV alone
    check(eng, [a], ["id"], pred, deleted={0: gone}, dvs=dvs, dv_index=[0])                  # DV and predicate
    check(eng, [a], ["id"], pred)                                                             # a predicate alone
    check(eng, [a], ["id"], pred, deleted={0: big}, dvs=dvs, dv_index=[1])                   # DV larger than the file
    check(eng, [a, b], ["id", "v"], pred, deleted={0: gone}, dvs=dvs, dv_index=[0, -1])      # one file without a DV
    check(eng, [a, b], ["id"], None, deleted={1: gone}, dvs=dvs, dv_index=[-1, 0], compact=False)
    dvs.close()


# ---- row-group pruning -----------------------------------------------------------------------------------
def test_row_group_pruning_uses_file_rows(eng, tmp_path):
    from delta_amd import kernel as K
    from delta_amd._lib import dk_rg_filter
    from delta_amd.partitions import RF_COL, RF_GE, RF_LIT, RF_LT, RF_OR, RL, pack_row_group_filter
    n = 300
    p = write(tmp_path, "rg.parquet", pa.table({"id": pa.array(range(n), pa.int64()),
                                                  "v": pa.array([i % 7 for i in range(n)], pa.int32())}), row_group_size=100)
    flt = pack_row_group_filter((["id"], [(RF_COL, 0, 0), (RF_LIT, RL["long"], 100), (RF_LT, 0, 0), (RF_COL, 0, 0),
                                          (RF_LIT, RL["long"], 200), (RF_GE, 0, 0), (RF_OR, 0, 0)], b""), dk_rg_filter)
    gone = [3, 150, 205, 299]                                 # file rows: 205 is decoded row 105
    dvs = K.DeletionVectors(eng, "file:" + str(tmp_path), [make_dv(tmp_path, gone, 3)])
    mid = range(100, 200)
    pred = Predicate("<", Column("v"), Literal.ofInt(4))
    for compact in (True, False):
        check(eng, [p], ["id"], pred, deleted={0: gone}, pruned={0: mid}, dvs=dvs, dv_index=[0], predicate=flt,
              compact=compact)
    dvs.close()


# ---- batching -------------------------------------------------------------------------------------------------
def test_batching(eng, tmp_path):
    n = 4099
    t = pa.table({"id": pa.array(range(n), pa.int64()), "s": ["row-%d" % i for i in range(n)]})
    a = write(tmp_path, "a.parquet", t)
    none = write(tmp_path, "none.parquet", pa.table({"id": pa.array(range(-50, 0), pa.int64()), "s": ["x"] * 50}))
    pred = Predicate("=", Column("id"), Column("id"))
    for pr in (Predicate(">=", Column("id"), Literal.ofLong(3)), pred):
        b, st = check(eng, [a, none, a], ["id", "s"], pr, batch_rows=7, window_rows=21)
        assert st["batches"] == len(b) and st["rows"] == sum(x.size for x in b)
    check(eng, [a, none], ["id", "s"], Predicate(">=", Column("id"), Literal.ofLong(3)), batch_rows=7, window_rows=21,
          compact=False)


# ---- projection -----------------------------------------------------------------------------------------------
def test_filter_column_is_not_emitted(eng, tmp_path):
    n = 500
    p = write(tmp_path, "p.parquet", pa.table({"id": pa.array(range(n), pa.int64()), "k": pa.array([i % 3 for i in range(n)], pa.int32()),
                                                 "s": ["s%d" % i for i in range(n)]}))
    b, _ = check(eng, [p], ["s"], Predicate("=", Column("k"), Literal.ofInt(1)))
    assert list(b[0].columns) == ["s"]


def test_map_leaf_is_emitted_while_filtering_on_a_scalar(eng, tmp_path):
    n = 200
    maps = [None if i % 9 == 0 else [("k%d" % j, None if j == 1 else "v%d_%d" % (i, j)) for j in range(i % 4)] for i in range(n)]
    p = write(tmp_path, "m.parquet", pa.table({"id": pa.array(range(n), pa.int64()),
                                                 "m": pa.array(maps, pa.map_(pa.string(), pa.string()))}))
    pred = Predicate("=", Column("id"), Literal.ofLong(0))
    pred = Or(pred, Predicate(">", Column("id"), Literal.ofLong(120)))
    leaves = ["id", "m.key_value.key", "m.key_value.value"]
    b, _ = check(eng, [p], leaves, pred, batch_rows=16)
    got = []
    for x in b:
        k, v = x.columns[leaves[1]], x.columns[leaves[2]]
        for r in range(x.size):
            if k.row_def[r] < k.rep_def - 1:
                got.append(None)
                continue
            got.append([(k.string(e).decode(), v.string(e).decode() if v.validity[e] else None)
                        for e in range(int(k.row_offs[r]), int(k.row_offs[r + 1]))])
    want = [maps[i] for i in [0] + list(range(121, n))]
    assert got == want


# ---- lifetime and misuse ----------------------------------------------------------------------------------
def test_early_close_and_misuse(eng, tmp_path):
    from delta_amd import kernel as K, programs
    from delta_amd._lib import DkError
    n = 300
    p = write(tmp_path, "l.parquet", pa.table({"id": pa.array(range(n), pa.int64())}))
    schema = schema_of(pq.read_table(p))
    prog = programs.compile_data_filter(Predicate(">=", Column("id"), Literal.ofLong(10)), schema)
    rd = K.DataReader(eng, [p], ["id"], filter=prog, batch_rows=64)
    held = [rd.next_raw(), rd.next_raw()]
    rd.close()                                                # early, with batches outstanding
    for raw, _ in held:
        b = raw.contents
        ri = np.ctypeslib.as_array(ctypes.cast(b.row_index, ctypes.POINTER(ctypes.c_int64)), shape=(int(b.n_rows),))
        assert ri[0] in (10, 74) and int(b.n_rows) == 64
        K.DataReader.release(raw)
    part = programs.compile_partition(Predicate("=", Column("p"), Literal.ofString("a")), {"p": ("string", "p")})
    with pytest.raises(DkError, match="data-filter program"):
        K.DataReader(eng, [p], ["id"], filter=part)
    dvs = K.DeletionVectors(eng, "file:" + str(tmp_path), [make_dv(tmp_path, [1], 4)])
    with pytest.raises(DkError, match="out of range"):
        K.DataReader(eng, [p], ["id"], dvs=dvs, dv_index=[1])
    with pytest.raises(DkError, match="without a deletion vector set"):
        K.DataReader(eng, [p], ["id"], dv_index=[0])
    dvs.close()


# ---- end to end -----------------------------------------------------------------------------------------------
def _delta_table(tmp_path, mapping=False):
    root = tmp_path / "tbl"
    root.mkdir()
    names = {"id": "col-aa", "name": "col-bb", "part": "col-pp"} if mapping else {"id": "id", "name": "name", "part": "part"}

    def field(name, typ, i):
        md = {"delta.columnMapping.id": i, "delta.columnMapping.physicalName": names[name]} if mapping else {}
        return {"name": name, "type": typ, "nullable": True, "metadata": md}
    schema = {"type": "struct", "fields": [field("id", "long", 1), field("name", "string", 2), field("part", "string", 3)]}
    files = {}
    for fname, part, lo in (("f0.parquet", "a", 0), ("f1.parquet", "b", 100), ("f2.parquet", "a", 200)):
        ids = list(range(lo, lo + 100))
        t = pa.table({names["id"]: pa.array(ids, pa.int64()),
                      names["name"]: pa.array([None if i % 10 == 0 else "n%d" % i for i in ids], pa.string())})
        pq.write_table(t, str(root / fname))
        files[fname] = (part, t)
    dv = make_dv(root, [0, 1, 50, 99], 5)
    features = ["deletionVectors"] + (["columnMapping"] if mapping else [])
    conf = {"delta.enableDeletionVectors": "true"}
    if mapping:
        conf.update({"delta.columnMapping.mode": "name", "delta.columnMapping.maxColumnId": "3"})
    protocol = {"minReaderVersion": 3, "minWriterVersion": 7, "readerFeatures": features, "writerFeatures": features}
    meta = {"id": "t", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
            "partitionColumns": ["part"], "configuration": conf, "createdTime": 1}

    def add(fname, with_dv=False):
        a = {"path": fname, "partitionValues": {names["part"]: files[fname][0]}, "size": os.path.getsize(str(root / fname)),
             "modificationTime": 1, "dataChange": True}
        if with_dv:
            a["deletionVector"] = {"storageType": dv[0], "pathOrInlineDv": dv[1], "offset": dv[2], "sizeInBytes": dv[3],
                                   "cardinality": dv[4]}
        return {"add": a}
    write_commit(str(root), 0, [{"protocol": protocol}, {"metaData": meta}, add("f0.parquet"), add("f1.parquet")])
    write_commit(str(root), 1, [add("f2.parquet", with_dv=True)])
    return str(root), files, names, [0, 1, 50, 99]


@pytest.mark.parametrize("mapping", [False, True], ids=["plain", "name-mapped"])
def test_end_to_end(eng, tmp_path, mapping):
    from delta_amd import kernel as K
    root, files, names, gone = _delta_table(tmp_path, mapping)
    k = 230
    pred = And(Predicate("=", Column("part"), Literal.ofString("a")), Predicate(">", Column("id"), Literal.ofLong(k)))
    leaves = [names["id"], names["name"]]

    def scan():
        return K.Table.forPath(eng, root).getLatestSnapshot(eng).getScanBuilder().withFilter(pred).build()
    got = {}
    for b in scan().readData(eng, leaves, batch_rows=32):
        assert b.selection is None and b.partition_values == {names["part"]: "a"}
        ids = b.columns[leaves[0]].fixed.view("<i8").tolist()
        nm = column_values(b.columns[leaves[1]], "string")
        assert ids == [files[b.path][1].column(0)[int(r)].as_py() for r in b.row_index]
        got.setdefault(b.path, []).extend(zip(b.row_index.tolist(), ids, nm))
    want = {}
    for fname in ("f0.parquet", "f2.parquet"):                 # partition pruning selects part = 'a'
        t = files[fname][1]
        dead = set(gone) if fname == "f2.parquet" else set()
        rows = [(r, t.column(0)[r].as_py(), cell(t.column(1)[r].as_py())) for r in range(t.num_rows)
                if r not in dead and O.keep(Predicate(">", Column("id"), Literal.ofLong(k)), {("id",): t.column(0)[r].as_py()},
                                            {("id",): "long"})]
        if rows:
            want[fname] = rows
    assert got == want and list(want) == ["f2.parquet"]
    # filter=None: what read_scan_data returns (every row of the selected files, the DV as the selection)
    old = [(p, batch.row_index.tolist(), None if sel is None else sel.tolist(),
            batch.columns[leaves[0]].fixed.view("<i8").tolist()) for p, batch, sel in K.read_scan_data(eng, scan(), leaves)]
    new = [(b.path, b.row_index.tolist(), b.selection.tolist(), b.columns[leaves[0]].fixed.view("<i8").tolist())
           for b in scan().readData(eng, leaves, filter=None, compact=False)]
    assert [(p, r, ids) for p, r, _, ids in old] == [(p, r, ids) for p, r, _, ids in new]
    for (_, r, so, _), (_, _, sn, _) in zip(old, new):
        assert sn == (so if so is not None else [True] * len(r))
