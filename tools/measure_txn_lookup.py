"""Measure Snapshot.getLatestTransactionVersion over a checkpoint on one MI355X, beside the only way
the code before it could answer the same question (checkpoint._checkpoint_other_rows over the same
file, then a dictionary lookup). Two shapes, written here with pyarrow:
  (a) sparse  a --rows checkpoint (default 10M) whose txn column is non-null in 100 rows spread over
              the file; the app id looked up is the first, the last, and an absent one
  (b) dense   a checkpoint with --dense non-null txn rows (default 1M, a streaming table), absent
              app id: the whole leaf is scanned
Per case: wall ms (median of --repeat runs after --warmup), bytes decoded (the decoded buffers the
device wrote) and bytes copied D2H. One JSON line per case. The snapshot load is outside the timed
region.

    python tools/measure_txn_lookup.py
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_table(root, n, txn_rows, apps):
    """Commit 0 (protocol, metaData) and its classic checkpoint of n rows: protocol / metaData in rows
    0 / 1, txn (apps[i], version i) at txn_rows[i], an add everywhere else."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from delta_amd import synth
    log = os.path.join(root, "_delta_log")
    os.makedirs(log)
    proto, meta = synth._pm_rows(synth.TableSpec(n_adds=1))
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": proto}) + "\n")
        f.write(json.dumps({"metaData": dict(meta, format={"provider": "parquet", "options": {}},
                                             configuration=dict(meta["configuration"]))}) + "\n")
    is_txn = np.zeros(n, bool)
    is_txn[txn_rows] = True
    app = np.full(n, None, object)
    app[txn_rows] = apps
    ver = np.zeros(n, np.int64)
    ver[txn_rows] = np.arange(len(txn_rows))
    txn = pa.StructArray.from_arrays(
        [pa.array(app, type=pa.string()), pa.array(ver), pa.nulls(n, pa.int64())],
        fields=[pa.field("appId", pa.string()), pa.field("version", pa.int64()), pa.field("lastUpdated", pa.int64())],
        mask=pa.array(~is_txn))
    is_add = ~is_txn
    is_add[:2] = False
    add = pa.StructArray.from_arrays(
        [pa.array(np.arange(n)).cast(pa.string()), pa.array(np.full(n, 1, np.int64)), pa.array(np.zeros(n, bool))],
        fields=[pa.field("path", pa.string()), pa.field("size", pa.int64()), pa.field("dataChange", pa.bool_())],
        mask=pa.array(~is_add))
    t = pa.table({"txn": txn, "add": add,
                  "metaData": pa.concat_arrays([pa.array([None, meta], type=synth.METADATA_TYPE),
                                                pa.nulls(n - 2, type=synth.METADATA_TYPE)]),
                  "protocol": pa.concat_arrays([pa.array([proto, None], type=synth.PROTOCOL_TYPE),
                                                pa.nulls(n - 2, type=synth.PROTOCOL_TYPE)])})
    path = os.path.join(log, "%020d.checkpoint.parquet" % 0)
    pq.write_table(t, path, compression="snappy")
    return path


class Meter:
    """Counts what the sets opened inside a timed call decoded and copied back."""

    def __init__(self, K):
        self.K = K
        self.decoded = self.d2h = 0
        PS = K.ParquetSet
        self._orig = (PS.close, PS.column_rows, PS.find_bytes, PS.columns)
        close, column_rows, find_bytes, columns = self._orig
        me = self

        def nbytes(c):
            return sum(a.nbytes for a in (c.row_def, c.row_offs, c.entry_def, c.fixed, c.offs, c.chars) if a is not None)

        def close_(ps):
            if ps._h:
                me.decoded += ps.traffic()[1]
            close(ps)

        def column_rows_(ps, *a):
            c = column_rows(ps, *a)
            me.d2h += nbytes(c)
            return c

        def find_bytes_(ps, *a, **kw):
            me.d2h += 8
            return find_bytes(ps, *a, **kw)

        def columns_(ps, fi):
            out = columns(ps, fi)
            me.d2h += sum(nbytes(c) for c in out.values() if c is not None)
            return out
        PS.close, PS.column_rows, PS.find_bytes, PS.columns = close_, column_rows_, find_bytes_, columns_

    def reset(self):
        self.decoded = self.d2h = 0

    def restore(self):
        PS = self.K.ParquetSet
        PS.close, PS.column_rows, PS.find_bytes, PS.columns = self._orig


def parent_lookup(eng, ckpt, app):
    """What the parent commit offers: every txn / domainMetadata row of the file on the host
    (checkpoint._checkpoint_other_rows), then a dictionary of the first version per app id."""
    from delta_amd import checkpoint as CK
    first = {}
    for rows in CK._checkpoint_other_rows(eng, [ckpt]):
        for r in sorted(rows):
            kind, v = rows[r]
            if kind == "txn":
                first.setdefault(v["appId"], v["version"])
    return first.get(app)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dense", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    from delta_amd import kernel as K
    eng = K.GpuEngine()
    meter = Meter(K)
    shapes = []
    n = args.rows
    rows = np.linspace(2, n - 1, 100).astype(np.int64)
    shapes.append(("sparse", n, rows, np.array(["app-%03d" % i for i in range(100)], object),
                   [("first", "app-000", 0), ("last", "app-099", 99), ("absent", "app-100", None)]))
    m = args.dense
    shapes.append(("dense", m + 2, np.arange(2, m + 2), np.array(["query-%07d" % i for i in range(m)], object),
                   [("absent", "query-absent", None)]))
    for shape, total, txn_rows, apps, cases in shapes:
        with tempfile.TemporaryDirectory() as root:
            t0 = time.perf_counter()
            ckpt = write_table(root, total, txn_rows, apps)
            print("%s: %d rows written in %.1f s (%d bytes)" % (shape, total, time.perf_counter() - t0,
                                                                 os.path.getsize(ckpt)), file=sys.stderr, flush=True)
            snap = K.Table.forPath(eng, root).getLatestSnapshot(eng)
            runs = [("device", pos, app, want, lambda app=app: snap.getLatestTransactionVersion(eng, app))
                    for pos, app, want in cases]
            # the parent's path reads everything whatever the app id: measured once per shape
            pos, app, want = cases[-1]
            runs.append(("parent", pos, app, want, lambda app=app: parent_lookup(eng, ckpt, app)))
            for path, pos, app, want, fn in runs:
                times = []
                for k in range(args.warmup + args.repeat):
                    meter.reset()
                    t0 = time.perf_counter()
                    got = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    assert got == want, (path, pos, got, want)
                    if k >= args.warmup:
                        times.append(dt)
                print(json.dumps(dict(shape=shape, ckpt_rows=total, txn_rows=len(txn_rows), path=path, app_id=pos,
                                      wall_ms_median=round(statistics.median(times), 2),
                                      wall_ms_min=round(min(times), 2), wall_ms_max=round(max(times), 2),
                                      bytes_decoded=int(meter.decoded), bytes_d2h=int(meter.d2h))), flush=True)
    meter.restore()
    eng.close()


if __name__ == "__main__":
    main()
