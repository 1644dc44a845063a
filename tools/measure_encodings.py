"""PLAIN against DELTA_LENGTH_BYTE_ARRAY / DELTA_BYTE_ARRAY / BYTE_STREAM_SPLIT decode.

Writes one file set (10M rows by default, 8 files) three ways -- the same rows every time:

  plain   path PLAIN,                   x PLAIN,             id PLAIN
  dlba    path DELTA_LENGTH_BYTE_ARRAY, x BYTE_STREAM_SPLIT, id PLAIN
  dba     path DELTA_BYTE_ARRAY,        x BYTE_STREAM_SPLIT, id PLAIN

(path: sorted 60-byte path-like strings; x: a double; id: a long) and reports per variant the file
bytes, the bytes copied to the device, and the wall time of ParquetSet open + decode over --passes
passes. The decode kernels' times come from the engine's timing=True counters, which a scan exposes
(GpuScan.kernel_stats), so a checkpoint of --ckpt-rows adds is written the same three ways with
synth (add.path in the variant's encoding) and scanned once cold and once warm.

Every step runs in a child process of its own under a timeout (--step-timeout seconds); a step that
fails or runs out of time is reported and ends the run (nothing more is started on a device that
may have faulted). One JSON line per step.
Usage: python tools/measure_encodings.py [--rows N] [--files K] [--passes P] [--ckpt-rows M]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAVES = ["path", "x", "id"]
VARIANTS = {"plain": {}, "dlba": {"path": "DELTA_LENGTH_BYTE_ARRAY", "x": "BYTE_STREAM_SPLIT"},
            "dba": {"path": "DELTA_BYTE_ARRAY", "x": "BYTE_STREAM_SPLIT"}}
CKPT = {"plain": None, "dlba": "DELTA_LENGTH_BYTE_ARRAY", "dba": "DELTA_BYTE_ARRAY"}
KERNELS = ("k_delta_lengths", "k_dlba_copy", "k_dba_tail", "k_dba_link", "k_dba_expand", "k_bss_gather",
           "k_string_positions", "k_string_copy", "k_tile_chars", "k_tile_decode", "k_delta_decode")


def write_files(root, rows, n_files, compression):
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    per = rows // n_files
    rng = np.random.default_rng(1)
    for f in range(n_files):
        ids = np.arange(f * per, (f + 1) * per, dtype=np.int64)
        num = pc.utf8_lpad(pc.cast(pa.array(ids), pa.string()), 12, "0")
        day = pc.utf8_lpad(pc.cast(pa.array(ids // 100_000 % 28 + 1), pa.string()), 2, "0")
        path = pc.binary_join_element_wise("date=2024-01-", day, "/part-", num, "-0123456789abc.c000.parquet", "")
        assert len(path[0].as_py()) == 60
        t = pa.table({"path": path, "x": rng.standard_normal(per), "id": ids})
        for name, enc in VARIANTS.items():
            os.makedirs(os.path.join(root, name), exist_ok=True)
            kw = dict(column_encoding=enc) if enc else {}
            pq.write_table(t, os.path.join(root, name, "part-%05d.parquet" % f), compression=compression,
                           use_dictionary=False, **kw)
    return per * n_files


def files_of(root, name):
    d = os.path.join(root, name)
    return [os.path.join(d, f) for f in sorted(os.listdir(d))]


def child_files(root, name, passes):
    from delta_amd import kernel as K
    paths = files_of(root, name)
    eng = K.GpuEngine()
    ms, h2d, rows = [], 0, 0
    for _ in range(passes):
        t0 = time.perf_counter()
        ps = K.ParquetSet(eng, paths, LEAVES).decode()
        ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        h2d = ps.traffic()[0]
        rows = sum(ps.num_rows(i) for i in range(len(paths)))
        ps.close()
    eng.close()
    return {"step": "files", "variant": name, "rows": rows, "file_bytes": sum(os.path.getsize(p) for p in paths),
            "h2d_bytes": h2d, "path_chars": 60 * rows, "open_decode_ms": ms}


def child_ckpt_write(root, name, rows):
    from delta_amd import synth
    extra = {"column_encoding": {"add.path": CKPT[name]}} if CKPT[name] else {}
    info = synth.write_table(os.path.join(root, "ckpt-" + name),
                             synth.TableSpec(n_adds=rows, n_commits=2, use_dictionary=False, compression="none", extra=extra))
    return {"step": "ckpt_write", "variant": name, "rows": rows,
            "checkpoint_bytes": sum(os.path.getsize(p) for p in info["checkpoint_files"])}


def child_ckpt_scan(root, name):
    from delta_amd import kernel as K
    eng = K.GpuEngine(timing=True)
    out = {"step": "ckpt_scan", "variant": name, "scan_ms": []}
    for _ in range(2):
        snap = K.Table.forPath(eng, os.path.join(root, "ckpt-" + name)).getLatestSnapshot(eng)
        scan = snap.getScanBuilder().build()
        t0 = time.perf_counter()
        n = sum(len(b.selected_rows()) for b in scan.getScanFiles(eng))
        out["scan_ms"].append(round((time.perf_counter() - t0) * 1e3, 1))
        st = scan.kernel_stats()
        out["scan_files"] = n
        out["kernels_us_x_launches"] = {k: [round(st[k][0], 1), st[k][1]] for k in KERNELS if k in st}
        scan.close()
    eng.close()
    return out


def step(args, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    except subprocess.TimeoutExpired:
        print(json.dumps({"step": args[0], "variant": args[2], "error": "timeout after %d s" % timeout}), flush=True)
        return False
    if r.returncode != 0:
        print(json.dumps({"step": args[0], "variant": args[2], "error": "exit %d" % r.returncode,
                          "stderr": r.stderr[-400:]}), flush=True)
        return False
    print(r.stdout.strip().splitlines()[-1], flush=True)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ckpt-rows", type=int, default=10_000_000)
    ap.add_argument("--compression", default="none")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, root, name = a.child[:3]
        if kind == "files":
            out = child_files(root, name, int(a.child[3]))
        elif kind == "ckpt_write":
            out = child_ckpt_write(root, name, int(a.child[3]))
        else:
            out = child_ckpt_scan(root, name)
        print(json.dumps(out), flush=True)
        return 0
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        rows = write_files(root, a.rows, a.files, a.compression)
        print(json.dumps({"step": "write_files", "rows": rows, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)
        for name in VARIANTS:
            if not step(["files", root, name, a.passes], a.step_timeout):
                return 1
        for name in VARIANTS if a.ckpt_rows > 0 else ():
            if not step(["ckpt_write", root, name, a.ckpt_rows], a.step_timeout) or \
                    not step(["ckpt_scan", root, name], a.step_timeout):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
