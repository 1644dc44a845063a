"""The Python wrappers' handle lifecycle (delta_amd/_lib.py: Handle, BatchReader) and GpuScan's
declared state.

Every class that owns a native handle frees it exactly once -- close(), the end of a `with` block or
garbage collection, whichever comes first -- and is falsy in `_h` afterwards; a batch reader closed
before its end leaves the batches it handed out valid (ScanImpl.java:376-392 closes its iterators
early); a scan's batches outlive the scan (GpuScan._detach_batches)."""
import gc
import os

import numpy as np
import pytest

from delta_amd import kernel as K
from delta_amd import synth
from delta_amd._lib import MAX_LEAF_DEPTH, Handle


# ---- CPU: the base class, a host-only handle, scan state, the small helpers ---------------------------------
def _skipping_program():
    from delta_amd import programs, skipping as sk
    from delta_amd.expressions import Column, Literal, Predicate
    leaves = {("a",): ("long", ("a",))}
    return programs.compile_skipping(sk.construct(Predicate(">", Column("a"), Literal.ofLong(5)), leaves), leaves)


def test_program_lifecycle():
    prog = _skipping_program()
    assert prog._h and prog.handle is prog._h
    assert prog.paths                                   # (the handle works)
    prog.close()
    assert not prog._h
    prog.close()
    assert not prog._h and not prog.handle
    del prog                                            # the last reference, after close()
    gc.collect()
    with _skipping_program() as p2:
        assert p2._h
    assert not p2._h


def test_handle_frees_once():
    freed = []

    class Counted(Handle):
        def __init__(self):
            self._h = 41

        def _free(self, h):
            freed.append(h)

    c = Counted()
    with c as inside:
        assert inside is c and c._h == 41
        c.close()
        assert c._h is None
        c.close()
    del c, inside
    gc.collect()
    assert freed == [41]
    with Counted():                                     # freed by __exit__ alone
        pass
    Counted()                                           # freed by __del__ alone
    gc.collect()
    assert freed == [41, 41, 41]


def test_handle_never_opened():
    class Unopened(Handle):
        _free_fn = "no_such_export"

    u = Unopened()
    assert not u._h
    u.close()                                           # nothing to free: the export is never looked up
    del u


@pytest.fixture()
def json_only_snapshot(tmp_path):
    """A snapshot object over a table of commit files only (no engine: the protocol and metadata are
    not loaded)."""
    d = str(tmp_path)
    synth.write_table(d, synth.TableSpec(n_adds=10, ckpt_version=-1, n_commits=3, adds_per_commit=5,
                                         removes_per_commit=2))
    log = os.path.join(d, "_delta_log")
    for f in os.listdir(log):
        if not f.endswith(".json"):
            os.remove(os.path.join(log, f))
    seg = K.build_log_segment(d)
    assert not seg.checkpoints and [f.version for f in seg.deltas] == [0, 1, 2]
    return K.Snapshot(K.Table(d), seg)


def test_scan_declared_state(json_only_snapshot):
    scan = K.ScanBuilder(json_only_snapshot).build()
    assert isinstance(scan, K.GpuScan)
    assert scan.owner is None and scan.exchange is None and scan.read_schema is None
    assert not scan.exchanging
    assert scan.replay is None and scan.ckpt is None and scan.tail is None and not scan._rh
    scan.close()                                        # never prepared
    scan.close()
    positional = K.GpuScan(json_only_snapshot, False, None, None)
    assert positional.owner is None and positional.exchange is None and positional.read_schema is None
    positional.close()


def test_scan_exchanging(json_only_snapshot):
    marker = object()
    b = K.ScanBuilder(json_only_snapshot)
    assert b.owner is None and b.exchange is None and b.read_schema is None
    assert b.withShard(2, 1, exchange=marker).build().exchanging
    assert not K.ScanBuilder(json_only_snapshot).withShard(1, 0, exchange=marker).build().exchanging
    assert K.ScanBuilder(json_only_snapshot).withShard(1, 0, owner=marker).build().exchanging
    assert not K.ScanBuilder(json_only_snapshot).withShard(2, 0).build().exchanging
    # an owner is honoured only on a sharded scan
    unsharded = K.GpuScan(json_only_snapshot, owner=marker)
    assert unsharded.owner is None and not unsharded.exchanging


@pytest.mark.parametrize("add_path,want", [
    ("date=2024-01-01/part%2000.parquet", "/tmp/t b/date=2024-01-01/part 00.parquet"),   # relative, escaped
    ("file:/data/x%20y.parquet", "/data/x%20y.parquet"),                                # absolute file: URI
    ("s3://bucket/key%20.parquet", "s3://bucket/key%20.parquet"),                       # another scheme
])
def test_data_file_path(add_path, want):
    assert K.data_file_path("file:/tmp/t b/", add_path) == want


def test_field_id_matrix():
    assert MAX_LEAF_DEPTH == 8
    got = K.field_id_matrix(["a.b.c", "x"], {"a.b.c": [7, None, 9]})
    want = np.array([7, -1, 9, -1, -1, -1, -1, -1,
                     -1, -1, -1, -1, -1, -1, -1, -1], np.int32)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    empty = K.field_id_matrix([], {"a": [1]})
    assert empty.dtype == np.int32
    np.testing.assert_array_equal(empty, np.full(8, -1, np.int32))


# ---- GPU: readers closed early, a scan's batches across close() ---------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """One checkpoint (2,000 adds) and three commits, and one data file beside them (the generator
    writes a log only)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    d = str(tmp_path_factory.mktemp("handles"))
    info = synth.write_table(d, synth.TableSpec(n_adds=2_000, n_commits=3, dv_frac=0.2))
    data = os.path.join(d, "data.parquet")
    pq.write_table(pa.table({"id": pa.array(range(1000), pa.int64()),
                             "name": pa.array(["n%d" % i for i in range(1000)])}), data)
    return d, info["checkpoint_files"][0], data


@pytest.fixture()
def eng():
    e = K.GpuEngine(parquet_batch_size=256)
    yield e
    e.close()


def _arrays(batch):
    """Every array a reader's batch holds, by name."""
    cols = batch.columns
    out = {}
    for leaf, c in cols.items():
        for a in ("row_def", "row_offs", "entry_def", "fixed", "offs", "chars", "validity"):
            v = getattr(c, a)
            if v is not None:
                out[leaf + ":" + a] = v
    for a in ("row_index", "selection"):
        v = getattr(batch, a, None)
        if v is not None:
            out[a] = v
    return out


def _open_reader(kind, eng, table):
    """(reader, the scan behind it or None)."""
    d, ckpt, data = table
    if kind == "parquet":
        return K.ParquetReader(eng, [ckpt], ["add.path", "add.size", K.ROW_INDEX_COLUMN]), None
    if kind == "data":
        return K.DataReader(eng, [data], ["id", "name"], batch_rows=256), None
    scan = K.Table.forPath(eng, d).getLatestSnapshot(eng).getScanBuilder().build()
    it = scan.getScanFileBatches(eng, batch_rows=256)   # a generator around the reader, not started here
    (rd,) = scan._scan_readers
    assert isinstance(rd, K.ScanFileReader)
    return rd, scan


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["parquet", "scan_files", "data"])
def test_reader_closed_early(eng, table, kind):
    rd, scan = _open_reader(kind, eng, table)
    try:
        batch = next(rd)
        before = {k: v.copy() for k, v in _arrays(batch).items()}
        assert before and all(len(v) for k, v in before.items() if k.endswith(":row_def"))
        rd.close()                                      # before the end
        assert not rd._h
        after = _arrays(batch)
        assert sorted(after) == sorted(before)
        for k in before:
            np.testing.assert_array_equal(after[k], before[k], err_msg=k)
        rd.close()
        assert not rd._h
    finally:
        if scan is not None:
            scan.close()
    rd2, scan2 = _open_reader(kind, eng, table)
    try:
        with rd2 as inside:
            assert inside is rd2 and rd2._h
            assert sum(1 for _ in rd2) > 1              # more than one batch: the close above was early
        assert not rd2._h
    finally:
        if scan2 is not None:
            scan2.close()


@pytest.mark.gpu
def test_scan_file_batches_generator_closed_early(eng, table):
    scan = K.Table.forPath(eng, table[0]).getLatestSnapshot(eng).getScanBuilder().build()
    it = scan.getScanFileBatches(eng, batch_rows=256)
    (rd,) = scan._scan_readers
    batch = next(it)
    before = {k: v.copy() for k, v in _arrays(batch).items()}
    it.close()                                          # closes its ScanFileReader
    assert not rd._h
    scan.close()
    scan.close()
    for k, v in _arrays(batch).items():
        np.testing.assert_array_equal(v, before[k], err_msg=k)


@pytest.mark.gpu
def test_scan_batches_across_close(eng, table):
    scan = K.Table.forPath(eng, table[0]).getLatestSnapshot(eng).getScanBuilder().build()
    batches = list(scan.getScanFiles(eng))
    assert {b.source for b in batches} >= {"json-tail", table[1]}     # a batch of either source
    leaves = ("add.path", "add.size", "add.deletionVector.cardinality")
    before = []
    for b in batches:
        held = {"selection": np.array(b.selection, copy=True)}
        for leaf in leaves[:2]:                         # (the third leaf is first read after close())
            c = b.data[leaf]
            held[leaf] = {a: getattr(c, a).copy() for a in ("row_def", "fixed", "offs", "chars")
                          if getattr(c, a) is not None}
        before.append(held)
    scan.close()
    assert not scan._rh and not scan.ckpt._h and not scan.tail._h
    scan.close()
    for b, held in zip(batches, before):
        np.testing.assert_array_equal(b.selection, held["selection"])
        assert len(b.selected_rows()) == int(held["selection"].sum())
        for leaf in leaves[:2]:
            for a, v in held[leaf].items():
                np.testing.assert_array_equal(getattr(b.data[leaf], a), v, err_msg=leaf + ":" + a)
        assert len(b.data[leaves[2]].row_def) == b.size
