"""A sharded scan's files streamed from every rank and merged in replay order: dk_replay_scan_open_rank
(the rank reader over a finished owner or exchange replay), dk_scan_batch_order (the order key of a
batch), dk_scan_merge_* (one ordered iterator over the in-process ranks) and dk_replay_counters_sum,
with their Python mirror (kernel.ScanFileReader on a sharded scan, shard.ScanFileMerge,
shard.merged_scan_file_batches), against the CPU oracle and the unsharded reader of the same table.

The GPU checks follow tests/test_owner.py::test_gpu_owner_loopback: the ranks of one process, each
rank's owner run on its own thread over the library's in-process transport, in a fresh process that
imports torch before libdkgpu. One table and one oracle replay serve the whole module."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from delta_amd import shard, synth

HERE = os.path.dirname(os.path.abspath(__file__))

# about 20,000 adds in a 5-part checkpoint whose parts hold row groups of 900, 900, 900, 900 and 400
# rows (no multiple of the 1000-row batches), 7 commits with removes and re-adds, deletion vectors on
# a fifth of the files, two partition columns, snappy pages
SPEC = dict(n_adds=20_000, n_parts=5, row_group_size=900, n_commits=7, adds_per_commit=30, removes_per_commit=30,
            readd_frac=0.2, dv_frac=0.2, pv_keys=2, compression="snappy")


def _plan(table, world):
    """Every rank's units [(replay-order file, first row group, end row group)] of the table."""
    from delta_amd import kernel as K
    from oracle import ref
    files = [f.path for f in ref.load_log_segment(table).all_files_reversed() if f.kind != "commit"]
    rows = [K.row_group_rows(p) for p in files]
    return rows, [shard.plan_units(rows, world, r) for r in range(world)]


def _assert_split(table, world):
    """The shapes the merge has to get right: every rank holds rows, and at least one checkpoint part
    is split between two ranks (each holding a run of its row groups)."""
    rows, plan = _plan(table, world)
    assert len(rows) >= 3 and all(len(r) >= 3 for r in rows), rows
    assert all(sum(rows[f][g] for f, a, b in units for g in range(a, b)) > 0 for units in plan), plan
    holders = {}
    for r, units in enumerate(plan):
        for f, a, b in units:
            holders.setdefault(f, set()).add(r)
    split = [f for f, rs in holders.items() if len(rs) >= 2]
    assert split, plan
    return split


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scan_merge"))
    synth.write_table(root, synth.TableSpec(**SPEC))
    return root


@pytest.fixture(scope="module")
def oracle(table, tmp_path_factory):
    """The oracle's ordered rows and counters of the table, computed once, in a file the checks' own
    processes read."""
    from tests.parity_util import oracle_scan
    o = oracle_scan(table)
    path = str(tmp_path_factory.mktemp("scan_merge_oracle") / "oracle.pkl")
    with open(path, "wb") as f:
        pickle.dump((o[1], o[2]), f)
    return path


@pytest.mark.parametrize("world", [2, 3])
def test_plan_splits_a_part_between_ranks(table, world):
    _assert_split(table, world)


# ---- the checks' bodies (run in a fresh process) ------------------------------------------------
def _load(oracle):
    with open(oracle, "rb") as f:
        return pickle.load(f)


def _torch_first():
    """torch's HIP runtime is loaded before libdkgpu's first call (the ranks' import order: both then
    share it, which the exchange's device tensors need)."""
    import torch
    torch.cuda.init()


class World:
    """The ranks of one scan in this process, run and synced."""

    def __init__(self, table, world, mode, run=True):
        _torch_first()
        from delta_amd import kernel as K
        self.K, self.mode, self.world = K, mode, world
        self.eng = K.GpuEngine()
        self.comms, self.scans, self.sides = [], [], []
        if mode == "owner":
            snap = K.Table.forPath(self.eng, table).getLatestSnapshot(self.eng)
            self.comms = shard.OwnerComm.local(world, steps=shard.OwnerComm.table_steps(self.eng, snap))
        for r in range(world):
            snap = K.Table.forPath(self.eng, table).getLatestSnapshot(self.eng)
            sb = snap.getScanBuilder()
            sb = sb.withShard(world, r, owner=self.comms[r]) if mode == "owner" else \
                sb.withShard(world, r, exchange=self.sides.append)
            sc = sb.build()
            sc.prepare(self.eng)
            sc.replay = True
            self.scans.append(sc)
        if run:
            self.run()

    def run(self):
        if self.mode == "owner":
            shard.run_local(self.scans)
        else:
            del self.sides[:]
            for sc in self.scans:
                sc.run()
            shard.exchange_local(self.sides)
            for sc in self.scans:
                sc.sync()

    def plain_scan(self, table):
        snap = self.K.Table.forPath(self.eng, table).getLatestSnapshot(self.eng)
        sc = snap.getScanBuilder().build()
        sc.prepare(self.eng)
        sc.replay = True
        sc.run()
        sc.sync()
        return sc

    def close(self):
        for sc in self.scans:
            sc.close()
        for c in self.comms:
            c.close()
        self.eng.close()


def _order(raw):
    from delta_amd._lib import check, lib
    key = (C.c_int64 * 3)()
    check(lib().dk_scan_batch_order(raw, key))
    return tuple(int(x) for x in key)


def _merged(w, emit_tail_rank=0, decode=True, **kw):
    """One merged pass over the world's rank readers: [(RawBatch, order key, rank)] and the readers'
    stats."""
    from tests.scan_export_util import RawBatch
    readers = [w.K.ScanFileReader(sc, emit_tail=(r == emit_tail_rank), **kw) for r, sc in enumerate(w.scans)]
    merge = shard.ScanFileMerge(readers)
    out = []
    try:
        while True:
            got = merge.next_raw()
            if got is None:
                break
            raw, sel, rank = got
            try:
                out.append((RawBatch(readers[rank], raw, sel, w.scans[rank].table_root(), decode), _order(raw), rank))
            finally:
                merge.release(raw)
        stats = [rd.stats() for rd in readers]
    finally:
        merge.close()
        for rd in readers:
            rd.close()
    return out, stats


def _rows(merged):
    return [row for b, _, _ in merged for row in b.rows]


def _check_keys(w, merged, compact, batch_rows):
    """Order keys: strictly increasing over the merged stream and within every rank; a checkpoint
    batch's key is (2, the file's replay-order index, the file row of its first row), a tail batch's
    (0, the commit file's replay-order index, its first row within that file); batches are full but
    the last of each source."""
    keys = [k for _, k, _ in merged]
    assert all(a < b for a, b in zip(keys, keys[1:])), "merged keys are not strictly increasing"
    n_commits = len(w.scans[0].snapshot.log_segment.deltas)
    by_src = {}
    for b, k, rank in merged:
        sc = w.scans[rank]
        assert b.n_rows > 0 and np.all(np.diff(b.row_index) > 0)
        if k[0] == 2:
            assert b.file >= 0 and k[1] == sc.ckpt_index[b.file]
            assert k[2] == sc.ckpt.row_offset(b.file) + int(b.row_index[0])      # the FILE row
        else:
            assert k[0] == 0 and b.file == -1 and 0 <= k[1] < n_commits and k[2] == int(b.row_index[0])
            if w.mode == "owner":
                assert k[1] in sc.tail_commits                                  # a commit file this rank parsed
        assert (b.selection is None) == compact
        by_src.setdefault((rank,) + k[:2], []).append(b)
    for r in range(w.world):
        mine = [k for _, k, rank in merged if rank == r]
        assert mine, "rank %d emitted nothing" % r
        assert all(a < b for a, b in zip(mine, mine[1:])), "rank %d's keys are not strictly increasing" % r
    for bs in by_src.values():
        assert all(b.n_rows == batch_rows for b in bs[:-1]) and bs[-1].n_rows <= batch_rows
    # one checkpoint part reaches the consumer from two ranks, and their batches do not interleave
    holders = {}
    for _, k, rank in merged:
        if k[0] == 2:
            holders.setdefault(k[1], []).append(rank)
    assert any(len(set(rs)) >= 2 for rs in holders.values()), holders
    for rs in holders.values():
        assert sum(a != b for a, b in zip(rs, rs[1:])) == len(set(rs)) - 1, rs


def _parity_check(table, oracle, world):
    from oracle import ref
    from tests.scan_export_util import read_batches, scan_rows
    _torch_first()
    _assert_split(table, world)
    want, counters = _load(oracle)
    w = World(table, world, "owner")
    n_commits = len(w.scans[0].snapshot.log_segment.deltas)
    for sc in w.scans:                                   # no rank parsed more than its share of the commits
        assert len(sc.tail_commits) <= -(-n_commits // world)
    # the unsharded reader of the same table
    plain = w.plain_scan(table)
    rd = w.K.ScanFileReader(plain, compact=True, batch_rows=1000)
    unsharded = scan_rows(read_batches(rd, plain.table_root()))
    rd.close()
    assert plain.metrics.as_tuple() == counters
    assert unsharded == want
    assert shard.merged_counters(w.scans) == counters
    for compact, kw in ((True, dict(batch_rows=1000)), (False, {})):
        merged, stats = _merged(w, compact=compact, **kw)
        rows = _rows(merged)
        assert len(rows) == len(want), (compact, len(rows), len(want))
        for i, (a, b) in enumerate(zip(rows, unsharded)):
            assert a == b, ("row", compact, i, a, b)
        _check_keys(w, merged, compact, kw.get("batch_rows", 1024))
        assert sum(s["batches"] for s in stats) == len(merged)
        assert sum(s["rows"] for s in stats) == sum(b.n_rows for b, _, _ in merged)
        assert all(s["d2h_bytes"] > 0 for s in stats)
        if compact:
            where = {(k[0], k[1], k[2] - int(b.row_index[0]) + int(i)) for b, k, _ in merged for i in b.row_index}
    if world == 3:
        # small batches and windows: several batches per commit file, several windows per run; the
        # same source rows come out, under strictly increasing keys
        merged, _ = _merged(w, decode=False, compact=True, batch_rows=13, window_rows=130)
        _check_keys(w, merged, True, 13)
        assert {(k[0], k[1], k[2] - int(b.row_index[0]) + int(i)) for b, k, _ in merged for i in b.row_index} == where
        assert max(sum(1 for _, k, _ in merged if k[:2] == (0, j)) for j in range(n_commits)) >= 2
    if world == 2:
        # the Python mirror: one generator over the ranks, and a rank's own getScanFileBatches
        rows, keys, ranks = [], [], []
        for b in shard.merged_scan_file_batches(w.scans, compact=True, batch_rows=1000):
            assert b.order is not None and 0 <= b.rank < world and b.selection is None
            keys.append(b.order)
            ranks.append(b.rank)
            rows += [ref.canon_add_from_cols(b.columns, int(r)) + (b.table_root,) for r in b.selected_rows()]
        assert rows == want and keys == sorted(keys) and len(set(keys)) == len(keys)
        own = [b.order for b in w.scans[1].getScanFileBatches(w.eng, compact=True, batch_rows=1000)]
        assert own and own == [k for k, rank in zip(keys, ranks) if rank == 1]
    w.run()                                              # a second run reuses the replays
    assert shard.merged_counters(w.scans) == counters
    assert _rows(_merged(w, compact=True, batch_rows=1000)[0]) == want
    plain.close()
    w.close()
    print("ok")


def _exchange_check(table, oracle):
    _torch_first()
    _assert_split(table, 2)
    want, counters = _load(oracle)
    w = World(table, 2, "exchange")
    assert shard.merged_counters(w.scans) == counters
    for compact, kw in ((True, dict(batch_rows=1000)), (False, {})):
        merged, _ = _merged(w, emit_tail_rank=0, compact=compact, **kw)     # the tail from rank 0 only
        assert _rows(merged) == want, compact
        _check_keys(w, merged, compact, kw.get("batch_rows", 1024))
        assert all(rank == 0 for _, k, rank in merged if k[0] == 0)
    w.close()
    print("ok")


def _open_rank(scan, ckpt_index=None, tail_index=None, emit_tail=0):
    """dk_replay_scan_open_rank with explicit index arrays: (status, handle, message)."""
    from delta_amd import _lib
    from delta_amd.kernel import ADD_LEAVES, _cstrs
    ck = list(scan.ckpt_index) if ckpt_index is None else list(ckpt_index)
    tf = list(getattr(scan, "tail_commits", []) + getattr(scan, "tail_parts", [])) if tail_index is None else list(tail_index)
    a, b = (C.c_int32 * max(1, len(ck)))(*ck), (C.c_int32 * max(1, len(tf)))(*tf)
    opt = _lib.dk_rank_scan_options(1, 1000, 0, emit_tail, len(ck), len(tf), a, b)
    h = C.c_void_p(1)
    rc = _lib.lib().dk_replay_scan_open_rank(scan._rh, _cstrs(ADD_LEAVES), len(ADD_LEAVES), C.byref(opt), C.byref(h))
    return rc, h, _lib.lib().dk_last_error().decode()


def _misuse_check(table, oracle):
    from delta_amd._lib import DkError, check, lib
    from tests.scan_export_util import read_batches, scan_rows
    want, counters = _load(oracle)
    w = World(table, 2, "owner", run=False)
    K = w.K
    # an owner replay before dk_replay_owner_run
    rc, h, msg = _open_rank(w.scans[0])
    assert rc != 0 and not h.value and "dk_replay_scan_open_rank" in msg and "has not finished" in msg, msg
    # a plain replay, and the same replay switched to owner mode after its plain run
    plain = w.plain_scan(table)
    rc, h, msg = _open_rank(plain, tail_index=[])
    assert rc != 0 and not h.value and "dk_replay_scan_open_rank" in msg and "neither" in msg, msg
    check(lib().dk_replay_set_owner(plain._rh, 2, 0))
    rc, h, msg = _open_rank(plain, tail_index=[])
    assert rc != 0 and not h.value and "dk_replay_scan_open_rank" in msg and "has not finished" in msg, msg
    with pytest.raises(DkError, match="dk_replay_scan_open: owner and exchange .* not supported"):
        K.ScanFileReader(plain)                          # (a plain scan opens with dk_replay_scan_open)
    check(lib().dk_replay_set_owner(plain._rh, 0, 0))
    # dk_scan_batch_order on a batch of a plain dk_replay_scan_open
    rd = K.ScanFileReader(plain, compact=True, batch_rows=1000)
    raw, _sel = rd.next_raw()
    with pytest.raises(DkError, match="dk_scan_batch_order: the batch did not come from a rank reader"):
        _order(raw)
    rd.release(raw)
    # and a plain reader is no input of a merge
    with pytest.raises(DkError, match="is not a rank reader"):
        shard.ScanFileMerge([rd])
    rd.close()
    w.run()
    # index arrays of the wrong length
    sc0, sc1 = w.scans
    rc, h, msg = _open_rank(sc0, ckpt_index=list(sc0.ckpt_index) + [9])
    assert rc != 0 and not h.value and "dk_replay_scan_open_rank: ckpt_index has" in msg, msg
    rc, h, msg = _open_rank(sc0, tail_index=(sc0.tail_commits + sc0.tail_parts)[:-1])
    assert rc != 0 and not h.value and "dk_replay_scan_open_rank: tail_index has" in msg, msg
    rc, h, msg = _open_rank(sc0, ckpt_index=[-1] + list(sc0.ckpt_index)[1:])
    assert rc != 0 and not h.value and "negative" in msg, msg
    # two readers given the same replay-order index for different parts: their file rows overlap
    assert sc1.ckpt_index[0] == sc0.ckpt_index[-1] and sc1.ckpt.row_offset(0) > 0      # the split part
    rc, h0, msg = _open_rank(sc0)
    assert rc == 0, msg
    rc, h1, msg = _open_rank(sc1, ckpt_index=[sc0.ckpt_index[0]] + list(sc1.ckpt_index)[1:])
    assert rc == 0, msg
    m = C.c_void_p(1)
    rc = lib().dk_scan_merge_open((C.c_void_p * 2)(h0, h1), 2, C.byref(m))
    msg = lib().dk_last_error().decode()
    assert rc != 0 and not m.value and "dk_scan_merge_open" in msg and "overlap in checkpoint file" in msg, msg
    for h in (h0, h1):                                   # nothing was read, copied or launched for it
        st = (C.c_int64 * 4)()
        check(lib().dk_scan_stats(h, st))
        assert list(st) == [0, 0, 0, 0]
    rc = lib().dk_scan_merge_open((C.c_void_p * 2)(h0, h0), 2, C.byref(m))
    assert rc != 0 and "given twice" in lib().dk_last_error().decode()
    lib().dk_scan_close(h0)
    lib().dk_scan_close(h1)
    # after all of it the engine still scans the table correctly, sharded and plain
    assert _rows(_merged(w, compact=True, batch_rows=1000)[0]) == want
    assert shard.merged_counters(w.scans) == counters
    rd = K.ScanFileReader(plain, compact=True, batch_rows=1000)
    assert scan_rows(read_batches(rd, plain.table_root())) == want
    rd.close()
    plain.close()
    w.close()
    print("ok")


def _lifetime_check(table, oracle):
    from tests.scan_export_util import RawBatch
    want, _ = _load(oracle)
    w = World(table, 2, "owner")
    root = w.scans[0].table_root()
    # batches held past the close of the merge and of their readers
    readers = [w.K.ScanFileReader(sc, compact=True, batch_rows=1000) for sc in w.scans]
    merge = shard.ScanFileMerge(readers)
    held = []
    while True:
        got = merge.next_raw()
        if got is None:
            break
        held.append(got)
    merge.close()
    for rd in readers:
        rd.close()
    rows = []
    for raw, sel, rank in held:
        rows += RawBatch(readers[rank], raw, sel, root).rows
        merge.release(raw)
    assert rows == want
    # closing the merge early, with a batch looked ahead on every reader, is safe; readers closed
    # before the merge are safe too
    readers = [w.K.ScanFileReader(sc, compact=False, batch_rows=1000) for sc in w.scans]
    merge = shard.ScanFileMerge(readers)
    first = merge.next_raw()
    for rd in readers:
        rd.close()
    from delta_amd._lib import DkError
    with pytest.raises(DkError, match="the reader is closed"):
        while merge.next_raw() is not None:              # (a looked-ahead batch may still come out)
            pass
    merge.close()
    got = RawBatch(readers[first[2]], first[0], first[1], root).rows
    assert got and got == want[:len(got)]
    merge.release(first[0])
    # and the scans still stream
    assert _rows(_merged(w, compact=True, batch_rows=1000)[0]) == want
    w.close()
    print("ok")


# ---- the GPU tests ------------------------------------------------------------------------------
def _run(body, *args):
    root = os.path.dirname(HERE)
    code = ("import sys; sys.path.insert(0, %r); from tests import test_scan_merge as T; T.%s(*%r)" % (root, body, args))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_merged_stream_parity(table, oracle, world):
    """In-process owner worlds 2 and 3, compact with 1000-row batches and uncompacted: the merged
    stream equals, row for row and in order, the unsharded getScanFileBatches output and the
    oracle's ordered rows; dk_replay_counters_sum gives the oracle's five counters; the order keys
    are strictly increasing per reader and over the merge, and a checkpoint batch's third key is the
    file row of its first row."""
    _run("_parity_check", table, oracle, world)


@pytest.mark.gpu
def test_exchange_mode_merged_stream(table, oracle):
    """Exchange mode, world 2 in one process (as tests/test_exchange.py builds it): with emit_tail on
    rank 0 only the merged rows and counters equal the oracle's."""
    _run("_exchange_check", table, oracle)


@pytest.mark.gpu
def test_misuse(table, oracle):
    """Each misuse fails with a message that names its function and launches nothing: a plain
    replay, an owner replay before dk_replay_owner_run (and one switched to owner mode after a plain
    run), index arrays of the wrong length, two readers overlapping in one file's rows, the order key
    of a plain reader's batch. The engine then scans the table correctly."""
    _run("_misuse_check", table, oracle)


@pytest.mark.gpu
def test_lifetime(table, oracle):
    """Batches held past dk_scan_merge_close and past the close of their readers still read
    correctly; closing the merge early is safe."""
    _run("_lifetime_check", table, oracle)
