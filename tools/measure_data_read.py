"""Data rows filtered on the device against the host path.

Writes a synthetic table of a few data files (about 10M rows in total by default: a long, a string and
a double column; deletion vectors on half the files) and, for predicates keeping about 0.1 %, 10 % and
100 % of the rows, reports per path the bytes copied from the device per input row and the wall time
of one pass:

  device   GpuScan.readData: DV and predicate per row on the GPU, only survivors copied (dk_scan_stats[0]);
  host     kernel.read_scan_data (every row of every projected column to the host, the DV selection per
           batch) plus a numpy evaluation of the same predicate over the copied columns.

Both passes start from a built scan and include the scan-file replay, the DV load and the decode.
Prints one JSON line per predicate. Usage: python tools/measure_data_read.py [--rows N] [--files K] [--passes P]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from delta_amd import kernel as K                                  # noqa: E402
from delta_amd.expressions import Column, Literal, Predicate       # noqa: E402
from tests.test_dv import _portable, _uuid_z85, _write_dv          # noqa: E402
from tests.txn_domain_tables import write_commit                   # noqa: E402

LEAVES = ["id", "name", "score"]


def write_table(root, rows, n_files):
    per = rows // n_files
    schema = {"type": "struct", "fields": [{"name": n, "type": t, "nullable": True, "metadata": {}}
                                           for n, t in (("id", "long"), ("name", "string"), ("score", "double"))]}
    features = ["deletionVectors"]
    actions = [{"protocol": {"minReaderVersion": 3, "minWriterVersion": 7, "readerFeatures": features,
                             "writerFeatures": features}},
               {"metaData": {"id": "m", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
                             "partitionColumns": [], "configuration": {"delta.enableDeletionVectors": "true"},
                             "createdTime": 1}}]
    rng = np.random.default_rng(1)
    os.makedirs(os.path.join(root, "dv"), exist_ok=True)
    deleted = 0
    for f in range(n_files):
        ids = np.arange(f * per, (f + 1) * per, dtype=np.int64)
        t = pa.table({"id": ids, "name": pa.array(["name-%09d" % i for i in ids]), "score": rng.random(per)})
        name = "part-%05d.parquet" % f
        pq.write_table(t, os.path.join(root, name), compression="snappy")
        add = {"path": name, "partitionValues": {}, "size": os.path.getsize(os.path.join(root, name)),
               "modificationTime": 1, "dataChange": True}
        if f % 2 == 0:                                  # a DV over 1 % of the file's rows
            gone = np.sort(rng.choice(per, per // 100, replace=False))
            conts = {}
            for r in gone.tolist():
                conts.setdefault(r >> 16, []).append(r & 0xFFFF)
            payload = _portable({0: {k: ("array", v) for k, v in conts.items()}})
            u = bytes([f % 256]) * 16
            h = u.hex()
            off = _write_dv(os.path.join(root, "dv", "deletion_vector_%s-%s-%s-%s-%s.bin" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])),
                            payload)
            add["deletionVector"] = {"storageType": "u", "pathOrInlineDv": "dv" + _uuid_z85(u), "offset": off,
                                     "sizeInBytes": len(payload), "cardinality": len(gone)}
            deleted += len(gone)
        actions.append({"add": add})
    write_commit(root, 0, actions)
    return per * n_files, deleted


def device_pass(eng, root, pred):
    scan = K.Table.forPath(eng, root).getLatestSnapshot(eng).getScanBuilder().build()
    t0 = time.perf_counter()
    rows = 0
    for b in scan.readData(eng, LEAVES, filter=pred):
        rows += b.size
    return rows, (time.perf_counter() - t0) * 1e3


def device_bytes(eng, root, pred):
    """One more pass through the reader itself for dk_scan_stats (readData owns its reader)."""
    from delta_amd import programs
    scan = K.Table.forPath(eng, root).getLatestSnapshot(eng).getScanBuilder().build()
    state = scan.getScanState(eng)
    prog = programs.compile_data_filter(pred, state["physicalDataReadSchemaString"])
    files = []
    for b in scan.getScanFiles(eng):
        for r in b.selected_rows():
            files.append((b.data["add.path"].string(int(r)).decode(), K._dv_of(b.data, int(r))))
    with_dv = [dv for _, dv in files if dv is not None]
    dvs = K.DeletionVectors(eng, scan.table_root(), with_dv)
    idx, k = [], 0
    for _, dv in files:
        idx.append(-1 if dv is None else k)
        k += dv is not None
    with K.DataReader(eng, [os.path.join(root, p) for p, _ in files], LEAVES, filter=prog, dvs=dvs, dv_index=idx) as rd:
        while True:
            got = rd.next_raw()
            if got is None:
                break
            rd.release(got[0])
        st = rd.stats()
    dvs.close()
    return st["d2h_bytes"]


def host_pass(eng, root, threshold):
    scan = K.Table.forPath(eng, root).getLatestSnapshot(eng).getScanBuilder().build()
    t0 = time.perf_counter()
    rows = copied = 0
    for _, batch, sel in K.read_scan_data(eng, scan, LEAVES):
        ids = batch.columns["id"].fixed.view("<i8")
        keep = ids < threshold
        if sel is not None:
            keep &= sel
        rows += int(keep.sum())
        for c in batch.columns.values():
            copied += c.row_def.nbytes + (c.validity.size + 7) // 8
            copied += c.fixed.nbytes if c.fixed is not None else c.offs.nbytes // 2 + c.chars.nbytes
        copied += 8 * batch.n_rows
    return rows, (time.perf_counter() - t0) * 1e3, copied


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    eng = K.GpuEngine()
    with tempfile.TemporaryDirectory() as root:
        total, deleted = write_table(root, a.rows, a.files)
        for frac in (0.001, 0.1, 1.0):
            thr = int(total * frac)
            pred = Predicate("<", Column("id"), Literal.ofLong(thr))
            dev = [device_pass(eng, root, pred) for _ in range(a.passes)]
            host = [host_pass(eng, root, thr) for _ in range(a.passes)]
            assert dev[0][0] == host[0][0], (dev[0][0], host[0][0])
            print(json.dumps({"keep": frac, "input_rows": total, "dv_deleted": deleted, "rows_kept": dev[0][0],
                              "device_bytes_per_input_row": round(device_bytes(eng, root, pred) / total, 3),
                              "host_bytes_per_input_row": round(host[0][2] / total, 3),
                              "device_ms": [round(x[1], 1) for x in dev], "host_ms": [round(x[1], 1) for x in host]}),
                  flush=True)


if __name__ == "__main__":
    main()
