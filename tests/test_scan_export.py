"""GpuScan.getScanFileBatches / dk_replay_scan_open: Scan.getScanFiles as bounded batches in the
ParquetHandler reader's layout (validity bits, int32 offsets), compacted to the selected rows or with
a selection vector, against the CPU oracle and the legacy getScanFiles path."""
import ctypes as C

import numpy as np
import pytest

from delta_amd import synth
from tests.parity_util import oracle_scan
from tests.scan_export_util import read_batches, scan_rows
from tests.test_gpu_parity import CASES, V2_CASES

pytestmark = pytest.mark.gpu

# shape -> (TableSpec arguments, json batch size, with stats)
SHAPES = {
    "dict-v1": (dict(n_adds=20_000, n_commits=12, adds_per_commit=40, removes_per_commit=40, **CASES["dict-v1"]), 3, False),
    "plain-v2-smallpages": (dict(n_adds=20_000, n_commits=12, adds_per_commit=40, removes_per_commit=40,
                                 **CASES["plain-v2-smallpages"]), 1024, False),
    "pv2-dv-removes": (dict(n_adds=20_000, n_commits=12, adds_per_commit=40, removes_per_commit=40,
                            **CASES["pv2-dv-removes"]), 3, False),
    "snappy-stats-variable": (dict(n_adds=20_000, n_commits=12, adds_per_commit=40, removes_per_commit=40,
                                   **CASES["snappy-stats-variable"]), 1024, True),
    "multi-rowgroup": (dict(n_adds=20_000, n_commits=12, adds_per_commit=40, removes_per_commit=40,
                            **CASES["multi-rowgroup"]), 1024, False),
    "v2-json-manifest-adds": (dict(n_adds=20_000, n_commits=8, **V2_CASES["v2-json-manifest-adds"]), 1024, True),
    # no tags, baseRowId or deletion vectors anywhere
    "plain-small": (dict(n_adds=3_000, n_commits=3), 1024, False),
}


class Tables:
    """One table, oracle result and synced scan per shape, shared by the module's tests."""

    def __init__(self, factory):
        self.factory = factory
        self.made = {}
        self.engines = {}

    def engine(self, jbs):
        from delta_amd import kernel as K
        if jbs not in self.engines:
            self.engines[jbs] = K.GpuEngine(json_batch_size=jbs)
        return self.engines[jbs]

    def get(self, name):
        from delta_amd import kernel as K
        if name not in self.made:
            spec, jbs, stats = SHAPES[name]
            root = str(self.factory.mktemp(name.replace("-", "_")))
            synth.write_table(root, synth.TableSpec(seed=synth.SEED + len(self.made), **spec))
            eng = self.engine(jbs)
            snap = K.Table.forPath(eng, root).getLatestSnapshot(eng)
            scan = snap.getScanBuilder().withStats(stats).build()
            self.made[name] = (root, eng, scan, oracle_scan(root, jbs, stats))
        return self.made[name]

    def close(self):
        for _, _, scan, _ in self.made.values():
            scan.close()
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    t = Tables(tmp_path_factory)
    yield t
    t.close()


def _synced(scan, eng):
    """The scan with a result (run once; later readers reuse it)."""
    if scan.replay is None or not getattr(scan, "_synced", False):
        for _ in scan.getScanFileBatches(eng, batch_rows=1 << 20):
            break
    return scan


def _read(scan, eng, **kw):
    from delta_amd import kernel as K
    rd = K.ScanFileReader(_synced(scan, eng), **kw)
    try:
        return read_batches(rd, scan.table_root())
    finally:
        rd.close()


def _legacy_positions(scan, eng):
    """(source key, row) of every selected row of the legacy getScanFiles on the same scan, and the
    legacy selection per source. Source keys: replay-order checkpoint file index, -1 tail, -2 manifest."""
    pos, sels = set(), {}
    for b in scan.getScanFiles(eng):
        if b.file_index >= 0:
            key = scan.ckpt_index.index(b.file_index)
        else:
            key = -1 if b.source == "json-tail" else -2
        sel = np.ones(b.size, bool) if b.selection is None else np.array(b.selection, dtype=bool)
        sels[key] = sel
        pos.update((key, int(r)) for r in np.nonzero(sel)[0])
    return pos, sels


def _check_shape(batches, compact, batch_rows, n_source_rows=None):
    """Batch shape per source: full batches but the last, no empty batch, sources in order."""
    order = {-1: -2, -2: -1}                    # tail, manifest, then files 0, 1, ...
    keys = [order.get(b.file, b.file) for b in batches]
    assert keys == sorted(keys), "sources out of order"
    by_src = {}
    for b in batches:
        by_src.setdefault(b.file, []).append(b)
    for key, bs in by_src.items():
        assert all(b.n_rows > 0 for b in bs)
        assert all(b.n_rows == batch_rows for b in bs[:-1]) and bs[-1].n_rows <= batch_rows
        ri = np.concatenate([b.row_index for b in bs])
        assert np.all(np.diff(ri) > 0), "row_index not strictly increasing within a source"
        if compact:
            assert all(b.selection is None for b in bs)
        else:
            assert all(b.selection is not None and len(b.selection) == b.n_rows for b in bs)
            assert np.array_equal(ri, np.arange(len(ri)))
            if n_source_rows is not None:
                assert len(ri) == n_source_rows[key]


@pytest.mark.parametrize("batch_rows", [1000, 333])
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", ["dict-v1", "plain-v2-smallpages", "pv2-dv-removes", "snappy-stats-variable",
                                  "multi-rowgroup", "v2-json-manifest-adds"])
def test_parity_with_oracle(tables, name, compact, batch_rows):
    root, eng, scan, o = tables.get(name)
    batches = _read(scan, eng, compact=compact, batch_rows=batch_rows)
    assert scan.metrics.as_tuple() == o[2]
    rows = scan_rows(batches)
    assert len(rows) == len(o[1])
    for i, (a, b) in enumerate(zip(rows, o[1])):
        assert a == b, ("row", i, a, b)
    _check_shape(batches, compact, batch_rows)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("name", ["pv2-dv-removes", "snappy-stats-variable", "v2-json-manifest-adds"])
def test_windows(tables, name, compact):
    """window_rows = 2048 with batch_rows = 1000: every file spans several windows (of 2000 rows),
    and maps and strings cross the window edges."""
    from delta_amd import kernel as K
    root, eng, scan, o = tables.get(name)
    rd = K.ScanFileReader(_synced(scan, eng), compact=compact, batch_rows=1000, window_rows=2048)
    batches = read_batches(rd, scan.table_root())
    st = rd.stats()
    rd.close()
    assert scan_rows(batches) == o[1]
    _check_shape(batches, compact, 1000)
    assert st["batches"] == len(batches) and st["rows"] == sum(b.n_rows for b in batches)
    assert st["windows"] >= len({b.file for b in batches}) + 3


@pytest.mark.parametrize("name", ["pv2-dv-removes", "v2-json-manifest-adds"])
def test_batch_shape_against_legacy(tables, name):
    root, eng, scan, o = tables.get(name)
    compact = _read(scan, eng, compact=True, batch_rows=1000)
    full = _read(scan, eng, compact=False, batch_rows=1000)
    legacy, sels = _legacy_positions(scan, eng)
    # a second getScanFiles after the readers still equals the oracle: the legacy path is undisturbed
    from oracle import ref
    rows = [ref.canon_add_from_cols(b.data, int(r)) + (b.table_root,) for b in scan.getScanFiles(eng)
            for r in b.selected_rows()]
    assert rows == o[1] and scan.metrics.as_tuple() == o[2]
    got = {(b.file, int(r)) for b in compact for r in b.row_index}
    assert got == legacy
    assert sum(b.n_rows for b in compact) == len(legacy)
    _check_shape(compact, True, 1000)
    _check_shape(full, False, 1000, {k: len(v) for k, v in sels.items()})
    for key, sel in sels.items():
        mine = [b.selection for b in full if b.file == key]
        assert np.array_equal(np.concatenate(mine) if mine else np.zeros(0, bool), sel)
    sizes = [b.n_rows for b in full if b.file == 0]
    n = len(sels[0])
    assert sizes == [min(1000, n - k) for k in range(0, n, 1000)]


def test_compaction_under_skipping(tmp_path):
    """Data skipping leaves few or no survivors: the compact reader emits exactly the oracle's rows,
    and a file without a survivor yields no batch."""
    from delta_amd import kernel as K
    from tests.test_skipping import SYNTH_PREDICATES, oracle_files
    root = str(tmp_path)
    synth.write_table(root, synth.TableSpec(n_adds=40_000, n_parts=3, n_commits=6, dv_frac=0.2, ckpt_removes=200,
                                            with_stats=True))
    eng = K.GpuEngine()
    few, none, mid = SYNTH_PREDICATES[2], SYNTH_PREDICATES[7], SYNTH_PREDICATES[3]
    assert few.name == "=" and none.name == "IS_NULL" and mid.name == "AND"
    for p in (few, none, mid):
        snap = K.Table.forPath(eng, root).getLatestSnapshot(eng)
        scan = snap.getScanBuilder().withFilter(p).build()
        try:
            rd_batches = []
            from delta_amd.kernel import ScanFileReader
            for _ in scan.getScanFileBatches(eng, batch_rows=1 << 20):
                break
            rd = ScanFileReader(scan, compact=True, batch_rows=1000)
            rd_batches = read_batches(rd, scan.table_root())
            rd.close()
            o_rows, o_counters = oracle_files(root, p)
            assert scan.metrics.as_tuple() == o_counters, p
            assert scan_rows(rd_batches) == o_rows, p
            _check_shape(rd_batches, True, 1000)
            legacy, sels = _legacy_positions(scan, eng)
            with_rows = {b.file for b in rd_batches}
            assert with_rows == {k for k, s in sels.items() if s.any()}, p
            if p is none:
                assert not [b for b in rd_batches if b.file >= 0]
        finally:
            scan.close()
    eng.close()


def _small_scan(root, eng, spec):
    from delta_amd import kernel as K
    synth.write_table(root, spec)
    snap = K.Table.forPath(eng, root).getLatestSnapshot(eng)
    return snap.getScanBuilder().build()


@pytest.mark.parametrize("ckpt_rows", [3, 63, 64, 65, 4097])
def test_ballot_and_scan_edges(tmp_path, ckpt_rows):
    """Checkpoint files of 3 (the smallest the generator writes: one add + protocol + metaData), 63,
    64, 65 and 4097 rows: the last ballot word, one wave exactly, one row into the next wave, and more
    than one scan block."""
    from delta_amd import kernel as K
    n_adds = ckpt_rows - 2
    eng = K.GpuEngine()
    k = min(2, n_adds)
    scan = _small_scan(str(tmp_path), eng, synth.TableSpec(n_adds=n_adds, n_commits=2, adds_per_commit=k,
                                                           removes_per_commit=min(1, n_adds)))
    try:
        o = oracle_scan(str(tmp_path))
        for compact in (True, False):
            for batch_rows in (64, 1000):
                batches = _read(scan, eng, compact=compact, batch_rows=batch_rows)
                assert scan.ckpt.num_rows(0) == ckpt_rows
                assert scan_rows(batches) == o[1], (compact, batch_rows)
                _check_shape(batches, compact, batch_rows)
        assert scan.metrics.as_tuple() == o[2]
    finally:
        scan.close()
        eng.close()


def test_selected_count_multiple_of_64_and_batch(tmp_path):
    """640 selected rows in the one checkpoint file, batches of 64: ten full batches, no empty one."""
    from delta_amd import kernel as K
    eng = K.GpuEngine()
    scan = _small_scan(str(tmp_path), eng, synth.TableSpec(n_adds=640, n_commits=0))
    try:
        o = oracle_scan(str(tmp_path))
        assert len(o[1]) == 640                 # the oracle confirms the count first
        batches = _read(scan, eng, compact=True, batch_rows=64)
        assert [b.n_rows for b in batches] == [64] * 10
        assert all(b.file == 0 for b in batches)
        assert scan_rows(batches) == o[1]
        _check_shape(batches, True, 64)
    finally:
        scan.close()
        eng.close()


def test_absent_and_all_null_leaves(tables):
    root, eng, scan, o = tables.get("plain-small")
    for compact in (True, False):
        batches = _read(scan, eng, compact=compact, batch_rows=1000)
        rows = scan_rows(batches)
        assert rows == o[1]
        # tags, baseRowId, defaultRowCommitVersion and the deletion vector decode to None
        assert all(r[5] is None and r[6] is None and r[7] is None and r[8] is None for r in rows)
    # a subset of the leaves: only those columns come back
    sub = _read(scan, eng, compact=True, batch_rows=1000, leaves=["add.path", "add.size"])
    assert all(set(b.present) == {"add.path", "add.size"} and all(b.present.values()) for b in sub if b.file >= 0)
    assert [(r[0], r[2]) for r in scan_rows(sub)] == [(r[0], r[2]) for r in o[1]]
    from delta_amd._lib import DkError
    with pytest.raises(DkError, match="leaf not projected"):
        _read(scan, eng, leaves=["add.nope"])


def test_python_mirror(tables):
    """getScanFileBatches yields ScanFileBatch objects whose BatchColumns decode to the oracle's rows."""
    from oracle import ref
    root, eng, scan, o = tables.get("pv2-dv-removes")
    for compact in (True, False):
        rows = []
        for b in scan.getScanFileBatches(eng, compact=compact, batch_rows=777):
            assert b.size <= 777 and len(b.row_index) == b.size and (b.selection is None) == compact
            assert b.table_root == scan.table_root() and b.source
            rows += [ref.canon_add_from_cols(b.columns, int(r)) + (b.table_root,) for r in b.selected_rows()]
        assert rows == o[1]


def test_lifetime_and_misuse(tmp_path):
    from delta_amd import kernel as K
    from delta_amd._lib import DkError, lib
    from tests.scan_export_util import RawBatch
    eng = K.GpuEngine()
    scan = _small_scan(str(tmp_path), eng, synth.TableSpec(n_adds=5_000, n_commits=4, pv_keys=2, dv_frac=0.2))
    try:
        o = oracle_scan(str(tmp_path))
        scan.prepare(eng)
        scan.replay = True
        # no result yet
        with pytest.raises(DkError, match="no result"):
            K.ScanFileReader(scan)
        scan.run()
        with pytest.raises(DkError, match="no result"):
            K.ScanFileReader(scan)
        scan.sync()
        # owner mode is refused
        lib().dk_replay_set_owner(scan._rh, 2, 0)
        with pytest.raises(DkError, match="not supported"):
            K.ScanFileReader(scan)
        lib().dk_replay_set_owner(scan._rh, 0, 0)
        # batches outlive the close of their reader, whether it was exhausted or closed early
        rd = K.ScanFileReader(scan, compact=True, batch_rows=1000)
        held = []
        while True:
            got = rd.next_raw()
            if got is None:
                break
            held.append(got)
        rd.close()
        early = K.ScanFileReader(scan, compact=True, batch_rows=1000)
        first = early.next_raw()
        early.close()                           # closing after the first batch is clean
        rows = []
        for raw, sel in held:
            rows += RawBatch(rd, raw, sel, scan.table_root()).rows
            rd.release(raw)
        assert rows == o[1]
        assert RawBatch(early, first[0], first[1], scan.table_root()).rows == o[1][:first[0].contents.n_rows]
        early.release(first[0])
        # a rerun invalidates an open reader: next fails, nothing is touched
        stale = K.ScanFileReader(scan, compact=False, batch_rows=1000)
        kept = stale.next_raw()
        scan.run()
        scan.sync()
        with pytest.raises(DkError, match="ran again or was freed"):
            stale.next_raw()
        kept_rows = RawBatch(stale, kept[0], kept[1], scan.table_root()).rows
        assert kept_rows == o[1][:len(kept_rows)]
        stale.release(kept[0])
        stale.close()
        # and the scan still serves both paths
        assert scan_rows(_read(scan, eng, compact=True, batch_rows=512)) == o[1]
        from oracle import ref
        rows = [ref.canon_add_from_cols(b.data, int(r)) + (b.table_root,) for b in scan.getScanFiles(eng)
                for r in b.selected_rows()]
        assert rows == o[1] and scan.metrics.as_tuple() == o[2]
    finally:
        scan.close()
        eng.close()
