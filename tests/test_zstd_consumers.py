"""Every consumer of decoded checkpoint or data pages once over zstd, against its snappy twin: the
scan-file batch reader, readData with a predicate and a deletion vector, the txn and domainMetadata
replays, and the sliced checkpoint open. The pages land in the arena slot a snappy page uses
(k_zstd_page, delta_amd/csrc/dk_zstd.hip), so each twin must give the same answer as the other and
as the oracle. tests/test_zstd_pages.py holds the page-level twins and the malformed frames."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from delta_amd import synth
from delta_amd.expressions import Column, Literal, Predicate
from tests import txn_domain_oracle as O
from tests import txn_domain_tables as T
from tests.parity_util import assert_same, oracle_scan, product_scan
from tests.scan_export_util import read_batches, scan_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from delta_amd import kernel as K
    e = K.GpuEngine()
    yield e
    e.close()


def _codecs(path):
    md = pq.ParquetFile(path).metadata
    return {md.row_group(g).column(i).compression for g in range(md.num_row_groups) for i in range(md.num_columns)}


def _checkpoints(d):
    log = os.path.join(d, "_delta_log")
    return sorted(os.path.join(log, f) for f in os.listdir(log) if ".checkpoint" in f and f.endswith(".parquet"))


def _twin_tables(tmp_path, **spec):
    out = {}
    for codec in ("snappy", "zstd"):
        d = str(tmp_path / codec)
        synth.write_table(d, synth.TableSpec(compression=codec, **spec))
        parts = _checkpoints(d)
        assert parts and all(_codecs(p) == {codec.upper()} for p in parts)
        out[codec] = d
    return out


def test_scan_file_batches(tmp_path, eng):
    from delta_amd import kernel as K
    tables = _twin_tables(tmp_path, n_adds=6_000, n_commits=9, adds_per_commit=30, removes_per_commit=30)
    got = {}
    for codec, d in tables.items():
        snap = K.Table.forPath(eng, d).getLatestSnapshot(eng)
        scan = snap.getScanBuilder().build()
        for _ in scan.getScanFileBatches(eng, batch_rows=1 << 20):     # run once; the readers reuse the result
            break
        per = {}
        for compact in (True, False):
            rd = K.ScanFileReader(scan, compact=compact, batch_rows=700)
            try:
                bs = read_batches(rd, scan.table_root())
            finally:
                rd.close()
            per[compact] = ([(b.file, b.n_rows, b.row_index.tolist(), None if b.selection is None else b.selection.tolist())
                             for b in bs], [r[:-1] for r in scan_rows(bs)])
        got[codec] = (per, scan.metrics.as_tuple())
        scan.close()
    assert got["zstd"] == got["snappy"]
    o = oracle_scan(tables["snappy"])              # the oracle reads snappy; the twins hold the same rows
    assert got["zstd"][1] == o[2]
    assert got["zstd"][0][True][1] == [r[:-1] for r in o[1]] and len(o[1]) > 0


def test_read_data_with_predicate_and_deletion_vector(tmp_path, eng):
    from delta_amd import kernel as K
    from tests.test_data_filter import check, make_dv, write
    n = 3000
    rng = np.random.default_rng(11)
    t = pa.table({"id": pa.array(range(n), pa.int64()), "v": pa.array([i % 10 for i in range(n)], pa.int32()),
                  "s": pa.array(["name-%04d" % (i * 13 % 997) if i % 6 else None for i in range(n)], pa.string()),
                  "d": pa.array(rng.standard_normal(n), pa.float64())})
    kw = dict(use_dictionary=False, write_statistics=False, data_page_size=8 << 10)
    paths = {c: write(tmp_path, c + ".parquet", t, compression=c, **kw) for c in ("snappy", "zstd")}
    assert _codecs(paths["zstd"]) == {"ZSTD"} and _codecs(paths["snappy"]) == {"SNAPPY"}
    gone = [0, n - 1] + list(range(1400, 1470))
    dvs = K.DeletionVectors(eng, "file:" + str(tmp_path), [make_dv(tmp_path, gone, 1)])
    pred = Predicate("<", Column("v"), Literal.ofInt(5))
    got = {}
    try:
        for c, p in paths.items():       # check() compares rows, values and batch shape with the oracle
            bs, _ = check(eng, [p], ["id", "s", "d"], pred, deleted={0: gone}, dvs=dvs, dv_index=[0], batch_rows=500)
            got[c] = [(b.size, b.row_index.tolist()) for b in bs]
    finally:
        dvs.close()
    assert got["zstd"] == got["snappy"] and sum(k for k, _ in got["zstd"]) > 0


def test_txn_and_domain_replays(tmp_path, eng):
    from delta_amd import kernel as K
    got = {}
    for codec in ("snappy", "zstd"):
        d = str(tmp_path / codec)
        T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("appId1", 0), T.dom("a", "a0")])
        T.write_commit(d, 1, [T.add("p1"), T.txn("appId1", 2), T.txn("appId2", 7), T.dom("b", "b0")])
        ck = os.path.join(d, "_delta_log", "%020d.checkpoint.parquet" % 1)
        pq.write_table(T.checkpoint_table(n=300, txns={100: ("appId1", 2), 250: ("appId2", 7), 251: (None, 9)},
                                          doms={5: ("a", "a-ckpt", False), 64: ("b", "b-ckpt", True)}),
                       ck, compression=codec)
        assert _codecs(ck) == {codec.upper()}
        T.write_commit(d, 2, [T.add("p2"), T.txn("appId2", 25), T.dom("c", "c-commit")])
        snap = K.Table.forPath(eng, d).getLatestSnapshot(eng)
        apps = ["appId1", "appId2", "appId", "nobody"]
        got[codec] = ([snap.getLatestTransactionVersion(eng, a) for a in apps], snap.getDomainMetadataMap(eng))
        assert got[codec][0] == [O.latest_transaction_version(d, a) for a in apps] == [2, 25, None, None]
        assert got[codec][1] == O.domain_metadata_map(d)
    assert got["zstd"] == got["snappy"]
    assert got["zstd"][1]["a"]["configuration"] == "a-ckpt" and got["zstd"][1]["b"]["removed"] is True


def test_sliced_open(tmp_path, eng):
    """Six checkpoint parts: the open decodes them slice by slice as their copies land."""
    tables = _twin_tables(tmp_path, n_adds=40_000, n_parts=6, n_commits=4)
    z, s = product_scan(tables["zstd"], engine=eng), product_scan(tables["snappy"], engine=eng)
    assert z[0] == s[0] and z[2] == s[2]
    assert [r[:-1] for r in z[1]] == [r[:-1] for r in s[1]] and len(z[1]) > 0
    assert_same(s, oracle_scan(tables["snappy"]))  # the oracle reads snappy; the twins hold the same rows
