"""Snapshot.getLatestTransactionVersion / getDomainMetadataMap and the two device lookups under them
(dk_parquet_find_bytes, dk_parquet_nonnull_rows) against the plain-Python oracle
(tests/txn_domain_oracle.py). Tables are hand-written in tmp_path."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import txn_domain_oracle as O
from tests import txn_domain_tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from delta_amd import kernel
    return kernel


@pytest.fixture(scope="module")
def eng(K):
    e = K.GpuEngine()
    yield e
    e.close()


def _misses(needle):
    """Near misses of a needle: proper prefix, proper extension, same length with another last
    byte, and a non-ASCII string (of the same byte length where the needle has two bytes to give)."""
    out = [needle + "x", needle[:-1] + "Z" if needle else "Z", (needle[:-2] if len(needle) >= 2 else needle) + "é"]
    if needle:
        out.append(needle[:-1])
    return out


def _rows(n, hits, needle, base=0):
    """txn rows of a file: near misses on every 5th row, a null appId inside a non-null struct on
    every 11th, the needle at `hits`; everything else a null struct."""
    miss = _misses(needle)
    rows = {r: (miss[(r // 5) % len(miss)], r) for r in range(0, n, 5)}
    rows.update({r: (None, r) for r in range(3, n, 11)})
    rows.update({h: (needle, base + h) for h in hits})
    return rows


def _walk(ps, fi, needle):
    got, r = [], ps.find_bytes(fi, "txn.appId", needle)
    while r >= 0:
        got.append(r)
        r = ps.find_bytes(fi, "txn.appId", needle, from_row=r + 1)
    return got


def _version(ps, fi, r):
    c = ps.column_rows(fi, "txn.version", r, 1)
    return int(c.fixed.view(np.int64)[0])


# ---- positions at wave, block and grid edges ----
POSITIONS = [0, 63, 64, 255, 256, 262_149, -1]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300_000])
def test_find_bytes_positions(tmp_path, K, eng, n):
    """The only match at each edge position that fits the file (300,000 rows: more than one pass of a
    1024 x 256 grid), then two matches in one file (the lower row wins) and the walk over all."""
    needle = "app-needle-0123"
    pos = sorted({p % n for p in POSITIONS if p < n})
    paths = []
    for i, p in enumerate(pos):
        paths.append(str(tmp_path / ("one%d.parquet" % i)))
        T.write_txn_file(paths[-1], n, _rows(n, [p], needle))
    paths.append(str(tmp_path / "all.parquet"))
    T.write_txn_file(paths[-1], n, _rows(n, pos, needle))
    ps = K.ParquetSet(eng, paths, K.TXN_LEAVES).decode()
    try:
        for i, p in enumerate(pos):
            assert ps.find_bytes(i, "txn.appId", needle.encode()) == p
            assert _version(ps, i, p) == p
            assert ps.find_bytes(i, "txn.appId", needle.encode(), from_row=p) == p
            assert ps.find_bytes(i, "txn.appId", needle.encode(), from_row=p + 1) == -1
        assert ps.find_bytes(len(pos), "txn.appId", needle.encode()) == pos[0]
        assert _walk(ps, len(pos), needle.encode()) == pos == O.file_matches(paths[-1], needle.encode())
        assert ps.find_bytes(len(pos), "txn.appId", b"absent") == -1
    finally:
        ps.close()


# ---- needles ----
@pytest.mark.parametrize("needle", [("abcdefghij" * 7)[:L] for L in (0, 1, 15, 16, 17, 70)]
                         + ["ключ-é-鍵"], ids=lambda s: "len%d" % len(s.encode()))
def test_find_bytes_needles(tmp_path, K, eng, needle):
    """Needle lengths around the 16-byte mark, an empty needle (matches an empty non-null string and
    nothing else) and a non-ASCII one; the file holds every near miss and null appIds."""
    n, hits = 200, [77, 150]
    p = str(tmp_path / "n.parquet")
    rows = _rows(n, hits, needle)
    rows[9] = ("", 9)                           # an empty, non-null appId
    T.write_txn_file(p, n, rows)
    nb = needle.encode("utf-8")
    want = O.file_matches(p, nb)
    assert want == (sorted(hits + [9]) if needle == "" else hits)
    ps = K.ParquetSet(eng, [p], K.TXN_LEAVES).decode()
    try:
        assert _walk(ps, 0, nb) == want
        for m in _misses(needle):               # each near miss finds its own rows, never the needle's
            mb = m.encode("utf-8")
            assert _walk(ps, 0, mb) == O.file_matches(p, mb)
        assert ps.find_bytes(0, "txn.appId", nb, from_row=n) == -1
    finally:
        ps.close()


# ---- encodings ----
@pytest.mark.parametrize("dictionary", [True, False], ids=["dict", "plain"])
@pytest.mark.parametrize("compression", ["snappy", "none"])
@pytest.mark.parametrize("page_version", ["1.0", "2.0"])
def test_find_bytes_encodings(tmp_path, K, eng, dictionary, compression, page_version):
    """Five row groups of 1,000 rows, groups 0, 2 and 4 all-null (pruned by their footer null
    counts), the match in the last kept one."""
    n, needle = 5000, "stream-query-42"
    rows = {r: ("app-%d" % (r % 50), r) for g in (1, 3) for r in range(g * 1000, (g + 1) * 1000, 3)}
    rows.update({r: (None, r) for r in (1001, 3002)})
    rows[3777] = (needle, 4242)
    p = str(tmp_path / "e.parquet")
    T.write_txn_file(p, n, rows, row_group_size=1000, use_dictionary=dictionary, compression=compression,
                     data_page_version=page_version, data_page_size=2048)
    assert K.nonnull_row_groups(p, "txn.appId") == [False, True, False, True, False]
    ps = K.ParquetSet(eng, [p], K.TXN_LEAVES, groups=[[1, 3]]).decode()
    try:
        assert ps.num_rows(0) == 2000
        r = ps.find_bytes(0, "txn.appId", needle.encode())
        assert r == 1777 and _version(ps, 0, r) == 4242
        assert ps.find_bytes(0, "txn.appId", needle.encode(), from_row=r + 1) == -1
        assert _walk(ps, 0, b"app-7") == [x - (1000 if x < 2000 else 2000) for x in O.file_matches(p, b"app-7")]
    finally:
        ps.close()


# ---- order across sources ----
def _snapshot(K, eng, d):
    return K.Table.forPath(eng, d).getLatestSnapshot(eng)


@pytest.fixture
def opened(K, monkeypatch):
    """Base names of the Parquet files every ParquetSet opened."""
    seen = []
    init = K.ParquetSet.__init__

    def spy(self, engine, paths, *a, **kw):
        seen.extend(os.path.basename(p) for p in paths)
        init(self, engine, paths, *a, **kw)
    monkeypatch.setattr(K.ParquetSet, "__init__", spy)
    return seen


def test_txn_checkpoint_then_commits(tmp_path, K, eng):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("appId1", 0), T.txn("only-old", 5)])
    T.write_commit(d, 1, [T.add("p1"), T.txn("appId1", 2), T.txn("appId2", 7)])
    T.write_classic(d, 1, n=300, txns={100: ("appId1", 2), 250: ("appId2", 7), 251: (None, 9), 7: ("only-old", 5)})
    T.write_commit(d, 2, [T.add("p2"), T.txn("appId2", 25)])
    T.write_commit(d, 3, [T.add("p3"), T.txn("appId3", 7908), T.txn("appId3", 7909)])
    snap = _snapshot(K, eng, d)
    want = {"appId1": 2, "only-old": 5, "appId2": 25, "appId3": 7908, "appId": None, "appId11": None, "nobody": None}
    for app, v in want.items():
        assert O.latest_transaction_version(d, app) == v
        assert snap.getLatestTransactionVersion(eng, app) == v


def test_txn_multipart_later_named_part_wins(tmp_path, K, eng, opened):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm())
    T.write_multipart(d, 0, [dict(n=70, txns={3: ("x", 1), 60: ("first-only", 11)}),
                             dict(n=40, with_pm=False),
                             dict(n=40, with_pm=False, txns={1: ("y", 5)}),
                             dict(n=66, with_pm=False, txns={65: ("x", 3)})])
    snap = _snapshot(K, eng, d)
    del opened[:]
    assert snap.getLatestTransactionVersion(eng, "x") == 3 == O.latest_transaction_version(d, "x")
    # the newest-named part answers; no other part is opened
    assert [n.split(".")[2] for n in opened] == ["0000000004"]
    del opened[:]
    assert snap.getLatestTransactionVersion(eng, "first-only") == 11 == O.latest_transaction_version(d, "first-only")
    # part 2 has no txn row at all: its footer rules it out and it is never opened
    assert [n.split(".")[2] for n in opened] == ["0000000004", "0000000003", "0000000001"]
    assert snap.getLatestTransactionVersion(eng, "z") is None


def test_txn_v2_parquet_manifest_ignores_sidecars(tmp_path, K, eng, opened):
    import pyarrow.parquet as pq
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm())
    side = os.path.join(d, "_delta_log", "_sidecars")
    os.makedirs(side)
    # a txn row in a sidecar is not part of this replay (sidecars are read for add / remove only)
    pq.write_table(T.checkpoint_table(n=10, with_pm=False, txns={4: ("x", 99), 5: ("side-only", 1)}),
                   os.path.join(side, "s1.parquet"))
    pq.write_table(T.checkpoint_table(n=12, txns={7: ("x", 4)}, doms={9: ("dm", "c", False)}, sidecars=["s1.parquet"]),
                   os.path.join(d, "_delta_log", "%020d.checkpoint.%s.parquet" % (0, "80a083e8-7026-4e79-81be-64bd76c43a11")))
    snap = _snapshot(K, eng, d)
    del opened[:]
    assert snap.getLatestTransactionVersion(eng, "x") == 4 == O.latest_transaction_version(d, "x")
    assert snap.getLatestTransactionVersion(eng, "side-only") is None
    assert snap.getDomainMetadataMap(eng) == O.domain_metadata_map(d) == {
        "dm": {"domain": "dm", "configuration": "c", "removed": False}}
    assert "s1.parquet" not in opened and opened


def test_no_checkpoint_goes_through_the_same_methods(tmp_path, K, eng, opened):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.txn("a", 1), T.dom("d1", "old")])
    T.write_commit(d, 1, [T.txn("a", 2), T.txn("ä", 3), T.dom("d1", "new", removed=True)])
    snap = _snapshot(K, eng, d)
    del opened[:]
    assert snap.getLatestTransactionVersion(eng, "a") == 2
    assert snap.getLatestTransactionVersion(eng, "ä") == 3
    assert snap.getLatestTransactionVersion(eng, "b") is None
    assert snap.getDomainMetadataMap(eng) == O.domain_metadata_map(d) == {
        "d1": {"domain": "d1", "configuration": "new", "removed": True}}
    assert opened == []


# ---- nonnull_rows ----
@pytest.fixture(scope="module")
def level_files(tmp_path_factory):
    """One 20,000-row file per count of non-null txn rows; every third of them has a null appId."""
    d = tmp_path_factory.mktemp("levels")
    rng = np.random.default_rng(7)
    out = {}
    for cnt in (0, 1, 64, 65, 5000):
        rows = sorted(int(r) for r in rng.choice(20_000, size=cnt, replace=False))
        p = str(d / ("l%d.parquet" % cnt))
        T.write_txn_file(p, 20_000, {r: (None if i % 3 == 2 else "a%d" % i, i) for i, r in enumerate(rows)})
        out[cnt] = (p, rows)
    return out


@pytest.mark.parametrize("cnt", [0, 1, 64, 65, 5000])
def test_nonnull_rows(K, eng, level_files, cnt):
    p, rows = level_files[cnt]
    ps = K.ParquetSet(eng, [p], K.TXN_LEAVES).decode()
    try:
        lv = ps.column(0, "txn.appId").row_def
        assert len(lv) == 20_000
        for min_def in (1, 2):
            want = np.nonzero(lv >= min_def)[0]
            got = ps.nonnull_rows(0, "txn.appId", min_def)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            mid = 10_001
            assert np.array_equal(ps.nonnull_rows(0, "txn.appId", min_def, from_row=mid), want[want >= mid])
        assert list(ps.nonnull_rows(0, "txn.appId", 1)) == rows
        assert len(ps.nonnull_rows(0, "txn.appId", 1, from_row=20_000)) == 0
        # a capacity below the count: *n is still the total, the first `cap` rows are written
        cap = max(1, cnt // 2)
        buf = np.full(cap + 1, -7, np.int64)
        n = C.c_int64()
        K.check(K.lib().dk_parquet_nonnull_rows(ps._h, 0, 0, 1, 0, buf.ctypes.data, cap, C.byref(n)))
        assert n.value == cnt
        assert list(buf[:min(cap, cnt)]) == rows[:cap] and buf[cap] == -7
    finally:
        ps.close()


# ---- the domain metadata map ----
def test_domain_metadata_map(tmp_path, K, eng, opened):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.dom("a", "a0"), T.dom("b", "b0"), T.dom("c", "c0"), T.dom("e", "e0")])
    T.write_multipart(d, 0, [
        dict(n=80, doms={5: ("a", "a-part1", False), 6: ("b", "b-part1", False), 70: ("c", "c-part1", False)}),
        dict(n=30, with_pm=False),
        dict(n=90, with_pm=False, doms={64: ("c", "c-part3", True), 65: ("e", "e-part3", False), 89: ("c", "late", False)})])
    T.write_commit(d, 1, [T.add("p"), T.dom("a", "a-commit1", removed=True)])
    T.write_commit(d, 2, [T.dom("f", "f-commit2"), T.dom("f", "f-second-line")])
    snap = _snapshot(K, eng, d)
    del opened[:]
    got = snap.getDomainMetadataMap(eng)
    assert got == O.domain_metadata_map(d)
    assert got["a"] == {"domain": "a", "configuration": "a-commit1", "removed": True}     # a removed winner is kept
    assert got["c"] == {"domain": "c", "configuration": "c-part3", "removed": True}       # part 3 before part 1
    assert got["b"]["configuration"] == "b-part1" and got["e"]["configuration"] == "e-part3"
    assert got["f"]["configuration"] == "f-commit2"
    assert sorted(n.split(".")[2] for n in opened) == ["0000000001", "0000000003"]      # part 2: no domain rows
    del opened[:]
    assert snap.getDomainMetadataMap(eng) is got          # cached: no device work the second time
    assert opened == []


def test_domain_metadata_map_empty(tmp_path, K, eng, opened):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("a", 1)])
    T.write_classic(d, 0, n=50, txns={9: ("a", 1)})
    snap = _snapshot(K, eng, d)
    del opened[:]
    assert snap.getDomainMetadataMap(eng) == {} == O.domain_metadata_map(d)
    assert opened == []                                   # no row group can hold a domain row


# ---- round trip through Table.checkpoint ----
def test_round_trip_through_a_written_checkpoint(tmp_path, K, eng):
    d = str(tmp_path)
    T.write_commit(d, 0, T.pm() + [T.add("p0"), T.txn("app", 1, 5), T.dom("dom", "{}")])
    T.write_commit(d, 1, [T.add("p1"), T.txn("app", 9, 6), T.txn("other", 3), T.dom("gone", "x", removed=True)])
    T.write_commit(d, 2, [T.add("p2"), T.dom("dom", '{"k":"é"}')])
    snap = _snapshot(K, eng, d)
    apps = ["app", "other", "absent", "ap"]
    before = ([snap.getLatestTransactionVersion(eng, a) for a in apps], snap.getDomainMetadataMap(eng))
    assert before[0] == [9, 3, None, None] == [O.latest_transaction_version(d, a) for a in apps]
    assert before[1] == O.domain_metadata_map(d) and before[1]["gone"]["removed"] is True
    K.Table.forPath(eng, d).checkpoint(eng)
    fresh = _snapshot(K, eng, d)
    assert fresh.log_segment.checkpoints and not fresh.log_segment.deltas     # answered by the checkpoint alone
    after = ([fresh.getLatestTransactionVersion(eng, a) for a in apps], fresh.getDomainMetadataMap(eng))
    assert after == before
    assert after[1] == O.domain_metadata_map(d)


# ---- misuse ----
def test_misuse_fails_and_the_set_keeps_serving(tmp_path, K, eng):
    import pyarrow.parquet as pq
    from delta_amd._lib import DkError
    p = str(tmp_path / "c.parquet")
    pq.write_table(T.checkpoint_table(n=100, txns={40: ("a", 4)}), p)
    leaves = K.TXN_LEAVES + ["protocol.readerFeatures.list.element", "add.partitionValues.key_value.key"]
    ps = K.ParquetSet(eng, [p], leaves).decode()
    ok = lambda: ps.find_bytes(0, "txn.appId", b"a") == 40 and list(ps.nonnull_rows(0, "txn.appId")) == [40]  # noqa: E731
    try:
        assert ok()
        for bad in (lambda: ps.find_bytes(0, "txn.version", b"a"),                               # fixed width
                    lambda: ps.find_bytes(0, "protocol.readerFeatures.list.element", b"a"),     # repeated
                    lambda: ps.find_bytes(0, "add.partitionValues.key_value.key", b"a"),        # repeated
                    lambda: ps.find_bytes(0, "txn.appId", b"a", from_row=-1),
                    lambda: ps.find_bytes(0, "txn.appId", b"a", from_row=101),
                    lambda: ps.nonnull_rows(0, "txn.appId", from_row=-1),
                    lambda: ps.nonnull_rows(0, "txn.appId", from_row=101)):
            with pytest.raises(DkError):
                bad()
            assert ok()
        assert ps.find_bytes(0, "txn.appId", b"a", from_row=100) == -1
    finally:
        ps.close()
