"""The delta byte-array / byte-stream-split decoders under their consumers: getScanFiles over a
checkpoint whose string leaves are DELTA_BYTE_ARRAY or DELTA_LENGTH_BYTE_ARRAY (add.path is the
reconciliation key: its decode-time hashes must equal the PLAIN path's), the txn lookup, and
GpuScan.readData's reader over data files with a DELTA_BYTE_ARRAY string, a BYTE_STREAM_SPLIT
double and a DELTA_BINARY_PACKED long. The oracle reads the PLAIN twin of every table."""
import os
import shutil

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from delta_amd import synth
from delta_amd.expressions import And, Column, Literal, Predicate
from tests.parity_util import assert_same, oracle_scan, product_scan

pytestmark = pytest.mark.gpu

DLBA, DBA, BSS = "DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY", "BYTE_STREAM_SPLIT"
STRING_LEAVES = ["add.path", "add.stats", "add.deletionVector.pathOrInlineDv",
                 "add.partitionValues.key_value.key", "add.partitionValues.key_value.value"]


@pytest.fixture(scope="module")
def engine():
    from delta_amd import kernel as K
    eng = K.GpuEngine()
    yield eng
    eng.close()


def _spec(**extra):
    # a few thousand adds, a commit tail with removes, DVs, paths that need %-canonicalisation
    return synth.TableSpec(n_adds=5_000, n_commits=4, dv_frac=0.2, with_stats=True, variable_paths=True,
                           use_dictionary=False, extra=extra)


@pytest.fixture(scope="module")
def plain_table(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plain"))
    synth.write_table(d, _spec())
    return d, oracle_scan(d), oracle_scan(d, with_stats=True)


def _encoded_copy(tmp_path, plain_root, encoding):
    """The PLAIN table with its checkpoint's string leaves rewritten in `encoding`."""
    d = str(tmp_path / "enc")
    shutil.copytree(plain_root, d)
    log = os.path.join(d, "_delta_log")
    n = 0
    for f in os.listdir(log):
        if ".checkpoint" in f and f.endswith(".parquet"):
            p = os.path.join(log, f)
            t = pq.read_table(p)
            have = set(synth._leaf_paths(t.schema))
            enc = {leaf: encoding for leaf in STRING_LEAVES if leaf in have}
            assert "add.path" in enc and "add.stats" in enc
            pq.write_table(t, p, use_dictionary=False, compression="snappy", column_encoding=enc, max_rows_per_page=1500)
            md = pq.ParquetFile(p).metadata
            used = {md.row_group(0).column(i).path_in_schema: md.row_group(0).column(i).encodings for i in range(md.num_columns)}
            assert all(encoding in used[leaf] for leaf in enc), used
            n += 1
    assert n
    return d


@pytest.mark.parametrize("encoding", [DBA, DLBA])
def test_scan_files_over_delta_encoded_checkpoint(tmp_path, engine, plain_table, encoding):
    root, want, want_stats = plain_table
    d = _encoded_copy(tmp_path, root, encoding)
    got = product_scan(d, engine=engine)
    # (table_root differs between the copies: compare rows without it)
    strip = lambda s: (s[0], [r[:-1] for r in s[1]], s[2])
    assert_same(strip(got), strip(want))
    assert_same(strip(product_scan(d, with_stats=True, engine=engine)), strip(want_stats))


@pytest.mark.parametrize("encoding", [DBA, DLBA])
def test_data_skipping_over_delta_encoded_stats(tmp_path, engine, plain_table, encoding):
    from tests.test_skipping import _gpu_files, oracle_files
    root, _, _ = plain_table
    d = _encoded_copy(tmp_path, root, encoding)
    pred = Predicate(">", Column("id"), Literal.ofLong(30_000_000))
    want_rows, want_counters = oracle_files(root, pred)          # the oracle over the PLAIN twin
    full = len(plain_table[1][1])
    assert 0 < len(want_rows) < full                             # the predicate skips some files, not all
    got_rows, got_counters = _gpu_files(d, pred, engine)
    assert got_counters == want_counters
    assert [r[:-1] for r in got_rows] == [r[:-1] for r in want_rows]


def test_txn_lookup_over_delta_encoded_app_ids(tmp_path, engine):
    from delta_amd import kernel as K
    from tests import txn_domain_oracle as O
    from tests import txn_domain_tables as T
    roots = []
    for name, kw in (("plain", dict(use_dictionary=False)),
                     ("dba", dict(use_dictionary=False, column_encoding={"txn.appId": DBA})),
                     ("dlba", dict(use_dictionary=False, column_encoding={"txn.appId": DLBA}))):
        d = str(tmp_path / name)
        T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("app-000", 1)])
        T.write_commit(d, 1, [T.add("p1")])
        txns = {2 + 3 * i: ("app-%03d" % i, 10 + i) for i in range(200)}
        txns[700] = (None, 9)
        pq.write_table(T.checkpoint_table(n=800, txns=txns), os.path.join(d, "_delta_log", "%020d.checkpoint.parquet" % 1), **kw)
        T.write_commit(d, 2, [T.add("p2"), T.txn("app-150", 999)])
        roots.append(d)
    apps = ["app-000", "app-001", "app-150", "app-199", "app-19", "nobody", ""]
    want = [O.latest_transaction_version(roots[0], a) for a in apps]
    assert want[:4] == [10, 11, 999, 209]
    for d in roots:
        snap = K.Table.forPath(engine, d).getLatestSnapshot(engine)
        assert [snap.getLatestTransactionVersion(engine, a) for a in apps] == want, d


def test_data_reader_over_encoded_data_files(tmp_path, engine):
    from delta_amd import kernel as K
    from tests.test_data_filter import check, make_dv
    n = 3000
    rng = np.random.default_rng(5)
    name = ["region=%04d/key-%06d-%s" % (i // 500, i, "z" * (i % 13)) for i in range(n)]
    name = [None if i % 41 == 0 else v for i, v in enumerate(name)]
    x = rng.standard_normal(n)
    x[::97] = np.nan
    x[1::101] = -0.0
    t = pa.table({"id": pa.array(range(n), pa.int64()), "name": pa.array(name, pa.string()),
                  "x": pa.array(x, pa.float64(), mask=np.arange(n) % 29 == 0)})
    kw = dict(use_dictionary=False, max_rows_per_page=700, row_group_size=2000)
    plain = str(tmp_path / "plain.parquet")
    enc = str(tmp_path / "enc.parquet")
    pq.write_table(t, plain, **kw)
    pq.write_table(t, enc, column_encoding={"id": "DELTA_BINARY_PACKED", "name": DBA, "x": BSS}, **kw)
    gone = [0, 5, 699, 700, 701, 2999] + list(range(1400, 1500))
    dvs = K.DeletionVectors(engine, "file:" + str(tmp_path), [make_dv(tmp_path, gone, 1)])
    pred = And(Predicate(">=", Column("name"), Literal.ofString("region=0002")),
               Predicate("<", Column("x"), Literal.ofDouble(0.25)))
    leaves = ["id", "name", "x"]
    for compact in (True, False):
        res = [check(engine, [p], leaves, pred, deleted={0: gone}, dvs=dvs, dv_index=[0], compact=compact)[0]
               for p in (plain, enc)]
        a, b = res
        assert len(a) == len(b)
        for ba, bb in zip(a, b):                     # the encoded file's batches equal the PLAIN twin's
            np.testing.assert_array_equal(ba.row_index, bb.row_index)
            for leaf in leaves:
                ca, cb = ba.columns[leaf], bb.columns[leaf]
                for f in ("row_def", "validity", "fixed", "offs", "chars"):
                    u, v = getattr(ca, f), getattr(cb, f)
                    assert (u is None) == (v is None)
                    if u is not None:
                        np.testing.assert_array_equal(u, v, err_msg="%s %s" % (leaf, f))
    dvs.close()
