"""The txn / domainMetadata replays on the CPU: the two device lookups are part of the C ABI and
of the Python surface, and the plain-Python oracle the GPU tests are held to
(tests/txn_domain_oracle.py) gives the known answers on hand-written tables."""
import ctypes
import os
import re

from tests import txn_domain_oracle as O
from tests import txn_domain_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dk_parquet_find_bytes", "dk_parquet_nonnull_rows")


def test_header_declares_the_lookups():
    with open(os.path.join(ROOT, "include", "dkgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in names


def test_library_exports_the_lookups():
    from delta_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(so, n)
        assert n in _lib.EXPORTS


def test_snapshot_has_the_public_methods():
    from delta_amd import kernel as K
    assert callable(K.Snapshot.getLatestTransactionVersion)
    assert callable(K.Snapshot.getDomainMetadataMap)
    assert callable(K.ParquetSet.find_bytes) and callable(K.ParquetSet.nonnull_rows)


# ---- the oracle's known answers ----
def test_oracle_set_transaction_checkpoint_shape(tmp_path):
    """Several versions per app id over commits, a checkpoint and later commits: the latest wins."""
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("appId1", 0)])
    T.write_commit(d, 1, [T.add("p1"), T.txn("appId1", 2)])
    T.write_commit(d, 2, [T.add("p2"), T.txn("appId2", 7)])
    # the checkpoint of version 2 holds the latest per app id, as a writer would have left them
    T.write_classic(d, 2, n=8, txns={3: ("appId1", 2), 6: ("appId2", 7)})
    T.write_commit(d, 3, [T.add("p3"), T.txn("appId2", 25)])
    T.write_commit(d, 4, [T.add("p4"), T.txn("appId3", 7908), T.txn("appId3", 7909)])
    assert [os.path.basename(p) for p in O.log_files_reversed(d)] == [
        "%020d.json" % 4, "%020d.json" % 3, "%020d.checkpoint.parquet" % 2]
    assert O.latest_transaction_version(d, "appId1") == 2        # only in the checkpoint
    assert O.latest_transaction_version(d, "appId2") == 25       # a commit overrides the checkpoint
    assert O.latest_transaction_version(d, "appId3") == 7908     # line order inside one commit
    assert O.latest_transaction_version(d, "appId") is None      # a proper prefix is no match
    assert O.latest_transaction_version(d, "appId4") is None


def test_oracle_removed_domain_hides_an_older_live_one(tmp_path):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.dom("a", '{"v":0}'), T.dom("b", '{"v":0}')])
    T.write_classic(d, 0, n=6, doms={2: ("a", '{"v":0}', False), 4: ("b", '{"v":0}', False)})
    T.write_commit(d, 1, [T.dom("a", "", removed=True)])
    T.write_commit(d, 2, [T.dom("c", '{"v":2}')])
    assert O.domain_metadata_map(d) == {
        "a": {"domain": "a", "configuration": "", "removed": True},
        "b": {"domain": "b", "configuration": '{"v":0}', "removed": False},
        "c": {"domain": "c", "configuration": '{"v":2}', "removed": False}}


def test_oracle_multipart_parts_in_descending_name_order(tmp_path):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm())
    T.write_multipart(d, 0, [dict(n=5, txns={3: ("x", 1)}, doms={4: ("dd", "one", False)}),
                             dict(n=4, with_pm=False, txns={0: ("x", 2)}),
                             dict(n=4, with_pm=False, txns={1: ("x", 3)}, doms={2: ("dd", "three", True)})])
    names = [os.path.basename(p) for p in O.log_files_reversed(d)]
    assert [n.split(".")[2] for n in names] == ["0000000003", "0000000002", "0000000001"]
    assert O.latest_transaction_version(d, "x") == 3
    assert O.domain_metadata_map(d) == {"dd": {"domain": "dd", "configuration": "three", "removed": True}}


def test_oracle_file_matches(tmp_path):
    p = str(tmp_path / "t.parquet")
    T.write_txn_file(p, 6, {0: ("a", 1), 2: (None, 2), 3: ("ab", 3), 4: ("a", 4), 5: ("", 5)})
    assert O.file_matches(p, b"a") == [0, 4]
    assert O.file_matches(p, b"a", 1) == [4]
    assert O.file_matches(p, b"") == [5]
    assert O.file_matches(p, b"abc") == []
