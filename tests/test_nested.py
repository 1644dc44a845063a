"""Parquet columns nested more than one list deep, read on the GPU.

pyarrow is the reference reader: the leaf view of the product (delta_amd/nested.py: lists where the
schema has lists, None where a list, a struct above it or the value is null) must equal the same walk
over pq.read_table(...).to_pylist(). Through dk_parquet_column + dk_parquet_column_nest the layout's
invariants are checked directly; through readParquetFiles the batches must concatenate to the
whole-file read. Before this feature every one of these reads failed with
`nested repetition not supported`."""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from delta_amd import kernel as K
from delta_amd import synth
from delta_amd._lib import DkError
from delta_amd.nested import leaf_view, nest_levels, pylist_leaf_view

pytestmark = pytest.mark.gpu

N_ROWS = 4000
I32, I64, STR = pa.int32(), pa.int64(), pa.string()


# ---- data: nulls and empties at every depth, null leaf values -------------------------------------
def _leaf(rng, kind):
    if rng.random() < 0.1:
        return None
    v = int(rng.integers(-1000, 1000))
    return "s%d" % (v % 37) if kind == "str" else v


def _list(rng, make, lo=0, hi=6, p_null=0.08):
    """None, or a list of lo..hi items (an empty list included)."""
    if rng.random() < p_null:
        return None
    return [make() for _ in range(int(rng.integers(lo, hi + 1)))]


def _aa(rng, kind):
    return _list(rng, lambda: _list(rng, lambda: _leaf(rng, kind)))


def _aaa(rng):
    return _list(rng, lambda: _list(rng, lambda: _list(rng, lambda: _leaf(rng, "int"), hi=3), hi=3), hi=4)


def _map(rng, row):
    m = _list(rng, lambda: None)
    if m is None:
        return None
    return [("k%d_%d" % (row, j), _list(rng, lambda: _leaf(rng, "int"))) for j in range(len(m))]


def _structs(rng):
    def one():
        if rng.random() < 0.1:
            return None
        return {"a": _leaf(rng, "int"), "tags": _list(rng, lambda: _leaf(rng, "str"))}
    return _list(rng, one)


SHAPES = {
    # name: (arrow type, row maker, {leaf path: pylist steps})
    "aa_int32": (pa.list_(pa.list_(I32)), lambda rng, r: _aa(rng, "int"), {"c.list.element.list.element": ["list", "list"]}),
    "aa_string": (pa.list_(pa.list_(STR)), lambda rng, r: _aa(rng, "str"), {"c.list.element.list.element": ["list", "list"]}),
    "map_arr_int64": (pa.map_(STR, pa.list_(I64)), lambda rng, r: _map(rng, r),
                      {"c.key_value.key": ["list", "key"], "c.key_value.value.list.element": ["list", "value", "list"]}),
    "arr_struct_tags": (pa.list_(pa.struct([("a", I32), ("tags", pa.list_(STR))])), lambda rng, r: _structs(rng),
                        {"c.list.element.a": ["list", ("field", "a")],
                         "c.list.element.tags.list.element": ["list", ("field", "tags"), "list"]}),
    "aaa_int32": (pa.list_(pa.list_(pa.list_(I32))), lambda rng, r: _aaa(rng), {"c.list.element.list.element.list.element": ["list"] * 3}),
}

# variation over the cases, not a cross product: page version, codec, page size, row groups
CASES = {
    "aa_int32-v1-none-2rg": ("aa_int32", dict(data_page_version="1.0", compression="none", data_page_size=4096, row_group_size=2100)),
    "aa_string-plain-v2-snappy": ("aa_string", dict(data_page_version="2.0", compression="snappy", use_dictionary=False, data_page_size=8192)),
    "aa_string-dict-v1-zstd": ("aa_string", dict(data_page_version="1.0", compression="zstd", use_dictionary=True, data_page_size=2048)),
    "map_arr_int64-v2-none-2rg": ("map_arr_int64", dict(data_page_version="2.0", compression="none", row_group_size=1900)),
    "arr_struct_tags-v1-snappy-2rg": ("arr_struct_tags", dict(data_page_version="1.0", compression="snappy", data_page_size=4096, row_group_size=2500)),
    "aaa_int32-v2-zstd": ("aaa_int32", dict(data_page_version="2.0", compression="zstd", data_page_size=4096)),
}


def _rows(shape, seed, n=N_ROWS):
    rng = np.random.default_rng(seed)
    return [SHAPES[shape][1](rng, r) for r in range(n)]


def _write(path, shape, rows, **kw):
    t = pa.table({"id": pa.array(range(len(rows)), I64), "c": pa.array(rows, SHAPES[shape][0])})
    pq.write_table(t, path, **kw)


def _enc(v):
    """str -> bytes throughout (the product's strings are bytes)."""
    if isinstance(v, str):
        return v.encode()
    return [_enc(x) for x in v] if isinstance(v, list) else v


def _reference(path, shape):
    """{leaf: leaf view per row} from pyarrow, once per file."""
    t = pq.read_table(path)
    rows = t.column("c").to_pylist()
    ref = {leaf: [_enc(pylist_leaf_view(v, steps)) for v in rows] for leaf, steps in SHAPES[shape][2].items()}
    ref["id"] = t.column("id").to_pylist()
    return ref


@pytest.fixture(scope="module")
def eng():
    e = K.GpuEngine(timing=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """case -> (path, shape, reference), written and read with pyarrow once."""
    d = tmp_path_factory.mktemp("nested")
    out = {}
    for i, (case, (shape, kw)) in enumerate(CASES.items()):
        path = str(d / (case + ".parquet"))
        _write(path, shape, _rows(shape, 100 + i), **kw)
        out[case] = (path, shape, _reference(path, shape))
    # one file whose level tiles (2,048 levels) hold no row and no depth-1 element (a single inner list of
    # 5,000 elements) and depth-1 elements without a value (a row of 3,000 empty inner lists)
    rows = _rows("aa_int32", 7, 1500)
    rows[300] = [[int(x) for x in range(5000)]]
    rows[301] = [[] for _ in range(3000)]
    rows[700] = [[1], None] + [[] for _ in range(2500)] + [[None, 2]]
    path = str(d / "long_lists.parquet")
    _write(path, "aa_int32", rows, data_page_version="1.0", compression="none", data_page_size=4096)
    out["long_lists"] = (path, "aa_int32", _reference(path, "aa_int32"))
    return out


def _check_invariants(col):
    levels = nest_levels(col)
    assert len(levels) == col.max_rep >= 2
    n_parent = col.n_rows
    for k, (list_def, parent_def, offs) in enumerate(levels, 1):
        assert len(parent_def) == n_parent and len(offs) == n_parent + 1, (col.path, k)
        assert offs[0] == 0 and (np.diff(offs) >= 0).all(), (col.path, k)
        # a parent holds elements exactly when its definition level reaches the list's
        np.testing.assert_array_equal(np.diff(offs) > 0, parent_def >= list_def, err_msg="%s depth %d" % (col.path, k))
        n_parent = int(offs[-1])                     # offs_k[-1] == n_k: the next level's parents
    assert n_parent == len(col.entry_def)            # offs_R[-1] == n_entries
    assert levels[-1][0] == col.rep_def
    np.testing.assert_array_equal(levels[0][1], col.row_def)


@pytest.mark.parametrize("case", list(CASES) + ["long_lists"])
def test_whole_file_matches_pyarrow(eng, files, case):
    path, shape, ref = files[case]
    leaves = ["id"] + list(SHAPES[shape][2])
    with K.ParquetSet(eng, [path], leaves) as ps:
        ps.decode()
        for leaf in leaves:
            col = ps.column(0, leaf)
            assert col.present and col.n_rows == len(ref["id"])
            if col.max_rep > 1:
                _check_invariants(col)
            else:
                assert col.nest == []
            assert leaf_view(col) == ref[leaf], leaf
        stats = ps.kernel_stats()
    assert "k_nest_count" in stats and "k_nest_fill" in stats


def test_async_open_reads_a_nested_leaf(eng, files):
    """dk_parquet_open_async with a nested leaf projected takes the synchronous path."""
    path, shape, ref = files["aaa_int32-v2-zstd"]
    leaf = next(iter(SHAPES[shape][2]))
    with K.ParquetSet(eng, [path], [leaf, "id"], async_open=True) as ps:
        ps.decode()
        col = ps.column(0, leaf)
        _check_invariants(col)
        assert col.max_rep == 3 and leaf_view(col) == ref[leaf]
        assert leaf_view(ps.column(0, "id")) == ref["id"]


def _read_batches(paths, leaves, batch_size, window_rows=3000):
    e = K.GpuEngine(parquet_batch_size=batch_size)
    try:
        with e.readParquetFiles(paths, leaves, window_rows=window_rows) as rd:
            return list(rd)
    finally:
        e.close()


@pytest.mark.parametrize("batch_size", [1024, 777])
def test_batches_concatenate_to_the_whole_file(files, batch_size, tmp_path):
    """Two files, a flat leaf, a depth-1 map leaf and a nested leaf in one read: per file the batches
    concatenated equal the whole-file read, no batch spans files, and the flat and depth-1 leaves
    equal what they give when read alone."""
    p0, shape, ref0 = files["map_arr_int64-v2-none-2rg"]
    p1 = str(tmp_path / "second.parquet")
    _write(p1, shape, _rows(shape, 55, 3100), data_page_version="1.0", compression="snappy", data_page_size=4096)
    refs = [ref0, _reference(p1, shape)]
    flat, key, nested = "id", "c.key_value.key", "c.key_value.value.list.element"
    batches = _read_batches([p0, p1], [flat, key, nested], batch_size)
    alone = _read_batches([p0, p1], [flat, key], batch_size)
    assert [(b.file, b.n_rows) for b in batches] == [(b.file, b.n_rows) for b in alone]
    assert [b.file for b in batches] == sorted(b.file for b in batches)
    for fi in (0, 1):
        mine = [b for b in batches if b.file == fi]
        assert all(0 < b.n_rows <= batch_size for b in mine)
        assert sum(b.n_rows for b in mine) == len(refs[fi]["id"])
        for leaf in (flat, key, nested):
            got = [row for b in mine for row in leaf_view(b.columns[leaf])]
            assert got == refs[fi][leaf], (fi, leaf)
        for b in mine:
            c = b.columns[nested]
            assert c.max_rep == 2 and len(c.nest) == 2
            assert len(c.nest[0][2]) == b.n_rows + 1 and c.nest[1][2][-1] == len(c.entry_def)
    for a, b in zip(alone, batches):
        for leaf in (flat, key):
            x, y = a.columns[leaf], b.columns[leaf]
            np.testing.assert_array_equal(x.row_def, y.row_def)
            np.testing.assert_array_equal(x.validity, y.validity)
            for f in ("row_offs", "entry_def", "fixed", "offs", "chars"):
                if getattr(x, f) is not None:
                    np.testing.assert_array_equal(getattr(x, f), getattr(y, f), err_msg=leaf + "." + f)


@pytest.mark.parametrize("case", ["long_lists", "arr_struct_tags-v1-snappy-2rg", "aaa_int32-v2-zstd"])
def test_batches_of_every_shape(files, case):
    path, shape, ref = files[case]
    leaves = list(SHAPES[shape][2]) + ["id"]
    batches = _read_batches([path], leaves, 777)
    for leaf in leaves:
        assert [row for b in batches for row in leaf_view(b.columns[leaf])] == ref[leaf], leaf


# ---- limits and refusals --------------------------------------------------------------------------
def _clean_read(eng, files):
    path, shape, ref = files["aa_int32-v1-none-2rg"]
    with K.ParquetSet(eng, [path], ["id"]) as ps:
        ps.decode()
        assert leaf_view(ps.column(0, "id")) == ref["id"]


def test_five_deep_keeps_the_refusal(eng, files, tmp_path):
    typ = I32
    for _ in range(5):
        typ = pa.list_(typ)
    p = str(tmp_path / "five.parquet")
    pq.write_table(pa.table({"c": pa.array([[[[[[1]]]]], None], typ)}), p)
    leaf = "c" + ".list.element" * 5
    with pytest.raises(DkError, match=r"nested repetition not supported: c\.list\.element"):
        K.ParquetSet(eng, [p], [leaf])
    _clean_read(eng, files)


def test_accessors_refuse_a_bad_depth_and_a_flat_leaf(eng, files):
    import ctypes as C
    from delta_amd._lib import check, dk_column, dk_nest_level, lib
    path, shape, _ = files["aa_int32-v1-none-2rg"]
    leaf = next(iter(SHAPES[shape][2]))
    with K.ParquetSet(eng, [path], [leaf, "id"]) as ps:
        ps.decode()
        lv = dk_nest_level()
        for li, depth, what in ((0, 0, "depth 0 outside 1..2"), (0, 3, "depth 3 outside 1..2"), (1, 1, "not a nested leaf")):
            with pytest.raises(DkError, match=what):
                check(lib().dk_parquet_column_nest(ps._h, 0, li, depth, C.byref(lv)))
        with pytest.raises(DkError, match="nested leaf " + leaf.replace(".", r"\.")):
            ps.column_rows(0, leaf, 0, 10)
        c = dk_column()
        check(lib().dk_parquet_column(ps._h, 0, 1, C.byref(c)))      # the set still answers
        assert c.n_rows == N_ROWS


def _delta_table(root, rows):
    os.makedirs(os.path.join(root, "_delta_log"))
    pq.write_table(pa.table({"id": pa.array(range(len(rows)), I64), "c": pa.array(rows, pa.list_(pa.list_(I32)))}),
                   os.path.join(root, "f0.parquet"))
    arr = {"type": "array", "elementType": {"type": "array", "elementType": "integer", "containsNull": True}, "containsNull": True}
    schema = {"type": "struct", "fields": [{"name": "id", "type": "long", "nullable": True, "metadata": {}},
                                           {"name": "c", "type": arr, "nullable": True, "metadata": {}}]}
    meta = {"id": "t", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
            "partitionColumns": [], "configuration": {}, "createdTime": 1}
    add = {"path": "f0.parquet", "partitionValues": {}, "size": os.path.getsize(os.path.join(root, "f0.parquet")),
           "modificationTime": 1, "dataChange": True}
    with open(os.path.join(root, "_delta_log", "%020d.json" % 0), "w") as f:
        for a in ({"protocol": {"minReaderVersion": 1, "minWriterVersion": 2}}, {"metaData": meta}, {"add": add}):
            f.write(json.dumps(a) + "\n")


def test_read_data_refuses_a_nested_column(eng, files, tmp_path):
    root = str(tmp_path / "tbl")
    _delta_table(root, _rows("aa_int32", 3, 200))
    leaf = "c.list.element.list.element"

    def scan():
        return K.Table.forPath(eng, root).getLatestSnapshot(eng).getScanBuilder().build()
    with pytest.raises(DkError, match="nested leaf " + leaf.replace(".", r"\.")):
        list(scan().readData(eng, ["id", leaf]))
    # the engine still scans a clean projection of the same table, and a clean file
    got = [v for b in scan().readData(eng, ["id"]) for v in b.columns["id"].fixed.view("<i8").tolist()]
    assert got == list(range(200))
    _clean_read(eng, files)


def test_existing_shape_launches_no_nest_kernel(tmp_path):
    """A checkpoint of ADD_LEAVES (maps: max_rep 1) reports no nest kernel among its timer slots."""
    spec = synth.TableSpec(n_adds=3000, n_commits=4, adds_per_commit=20, removes_per_commit=10)
    synth.write_table(str(tmp_path), spec)
    e = K.GpuEngine(timing=True)
    try:
        scan = K.Table.forPath(e, str(tmp_path)).getLatestSnapshot(e).getScanBuilder().build()
        n = sum(len(b.selected_rows()) for b in scan.getScanFiles(e))
        stats = scan.kernel_stats()
        scan.close()
    finally:
        e.close()
    assert n > 0 and "k_tile_decode" in stats
    assert not [k for k in stats if "nest" in k], stats
