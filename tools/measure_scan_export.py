"""Measure full-row consumption of Scan.getScanFiles over three paths on one synthetic table:
  (a) legacy   GpuScan.getScanFiles: one FilteredColumnarBatch per checkpoint file, dk_column mirrors
  (b) full     dk_scan_next, compact = 0: bounded batches + selection vector
  (c) compact  dk_scan_next, compact = 1: only the selected rows
once without a predicate and once with a selective one (id = 25000123 over the stats). "Full row" =
add.path, add.partitionValues (key, value) and add.size of every selected row are touched on the
host. Per path: wall ms per consumption (median of --repeat runs after --warmup), D2H bytes per
checkpoint row and rows emitted. The replay itself (prepare, run, sync) is outside the timed region:
every path consumes the same finished replay.

    python tools/measure_scan_export.py --rows 10000000
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

LEAVES = ["add.path", "add.partitionValues.key_value.key", "add.partitionValues.key_value.value", "add.size"]


def consume_legacy(scan):
    """Touch the selected rows' path, partitionValues and size of the per-file batches; returns
    (selected rows, D2H bytes: the mirrored arrays of the four leaves plus the selection bytes)."""
    rows = moved = emitted = 0
    acc = 0
    for b in scan._batches():
        sel = b.selected_rows()
        rows += len(sel)
        emitted += b.size
        on_device = b.file_index >= 0 and b.source != "json-tail"
        if on_device:
            moved += b.size
        for leaf in LEAVES:
            c = b.data.get(leaf)
            if c is None:
                continue
            if on_device:
                moved += sum(a.nbytes for a in (c.row_def, c.row_offs, c.entry_def, c.fixed, c.offs, c.chars)
                             if a is not None)
            if not len(sel):
                continue
            if c.max_rep > 0:
                lo, hi = c.row_offs[sel], c.row_offs[sel + 1]
                acc += int((hi - lo).sum())
                if c.offs is not None and len(c.offs) > 1:
                    acc += int((c.offs[hi] - c.offs[lo]).sum())
            elif c.offs is not None:
                acc += int((c.offs[sel + 1] - c.offs[sel]).sum())
            else:
                acc += int(c.fixed.view(np.int64)[sel].sum() & 0xffff)
    return emitted, moved, acc, rows


def consume_reader(scan, compact, batch_rows):
    """Touch the same values through dk_scan_next's batches (zero-copy views of the window)."""
    import ctypes as C

    from delta_amd import kernel as K
    rd = K.ScanFileReader(scan, compact=compact, batch_rows=batch_rows, leaves=LEAVES)
    rows = acc = 0

    def view(ptr, n, dtype):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(int(n),))
    while True:
        got = rd.next_raw()
        if got is None:
            break
        raw, sel_ptr = got
        b = raw.contents
        n = int(b.n_rows)
        sel = np.arange(n) if not sel_ptr else np.nonzero(view(sel_ptr, n, np.uint8))[0]
        rows += len(sel)
        if len(sel):
            for i in range(len(LEAVES)):
                c = b.cols[i]
                if not c.present:
                    continue
                v0 = int(c.value_offset)
                if c.max_rep > 0:
                    ro = view(c.row_offs, n + 1, np.int32)
                    lo, hi = ro[sel], ro[sel + 1]
                    acc += int((hi - lo).sum())
                    if c.offs and c.n_values:
                        o = view(c.offs, int(ro[n]) + 1, np.int32)
                        acc += int((o[hi].astype(np.int64) - o[lo]).sum())
                elif c.phys == 6:
                    o = view(c.offs, v0 + n + 1, np.int32)
                    acc += int((o[v0 + sel + 1].astype(np.int64) - o[v0 + sel]).sum())
                else:
                    acc += int(view(c.fixed, v0 + n, np.int64)[v0 + sel].sum() & 0xffff)
        rd.release(raw)
    st = rd.stats()
    rd.close()
    return st["rows"], st["d2h_bytes"], acc, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--batch-rows", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--table", default=None, help="directory to build the table in (default: a temporary one)")
    args = ap.parse_args()
    from delta_amd import kernel as K
    from delta_amd import synth
    from delta_amd.expressions import Column, Literal, Predicate
    tmp = None
    root = args.table
    if root is None:
        tmp = tempfile.TemporaryDirectory()
        root = tmp.name
    if not os.path.exists(os.path.join(root, "_delta_log")):
        t0 = time.perf_counter()
        synth.write_table(root, synth.TableSpec(n_adds=args.rows, pv_keys=2, compression="snappy", with_stats=True,
                                                n_commits=100, adds_per_commit=50, removes_per_commit=50))
        print("table: %d adds written in %.1f s" % (args.rows, time.perf_counter() - t0), file=sys.stderr, flush=True)
    eng = K.GpuEngine()
    selective = Predicate("=", Column("id"), Literal.ofLong(25_000_123))
    for label, pred in (("no-predicate", None), ("selective", selective)):
        snap = K.Table.forPath(eng, root).getLatestSnapshot(eng)
        sb = snap.getScanBuilder().withStats(True)
        scan = (sb.withFilter(pred) if pred is not None else sb).build()
        scan.prepare(eng)
        scan.replay = True
        scan.run()
        scan.sync()
        ckpt_rows = sum(scan.ckpt.num_rows(f) for f in range(len(scan.ckpt_files)))
        paths = (("legacy", lambda: consume_legacy(scan)),
                 ("full", lambda: consume_reader(scan, False, args.batch_rows)),
                 ("compact", lambda: consume_reader(scan, True, args.batch_rows)))
        for name, fn in paths:
            times, got = [], None
            for k in range(args.warmup + args.repeat):
                if name == "legacy":
                    # a fresh result: the legacy mirrors are cached per decode, every repeat must move them again
                    scan._detach_batches()
                    scan.run()
                    scan.sync()
                t0 = time.perf_counter()
                got = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if k >= args.warmup:
                    times.append(dt)
            print(json.dumps(dict(predicate=label, path=name, ckpt_rows=ckpt_rows, rows_emitted=got[0], rows_selected=got[3],
                                  wall_ms_median=round(statistics.median(times), 2),
                                  wall_ms_min=round(min(times), 2), wall_ms_max=round(max(times), 2),
                                  d2h_bytes_per_ckpt_row=round(got[1] / max(1, ckpt_rows), 3),
                                  d2h_bytes=int(got[1]))), flush=True)
        scan.close()
    eng.close()
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
