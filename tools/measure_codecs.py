"""none against snappy against zstd level 3 over one synthetic checkpoint.

Writes the same checkpoint (--rows adds, 10M by default) three ways with synth and reports per codec
the checkpoint bytes, the wall time of a getScanFiles that only counts its selected rows (cold and
warm), the engine's kernel times (timing=True, GpuScan.kernel_stats), and the decompression kernels'
output bytes per second (dk_parquet_kernel_traffic's written bytes over their summed time). Beside
them, for orientation only, pyarrow's host decompression time over the same page bodies: the pages of
every column chunk are walked with a small Thrift reader and each compressed body goes through
pyarrow.Codec.decompress on one thread.

Every device step runs in a child process of its own under a timeout (--step-timeout seconds); a step
that fails or runs out of time is reported and ends the run (nothing more is started on a device
that may have faulted). One JSON line per step.
Usage: python tools/measure_codecs.py [--rows N] [--parts K]
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

CODECS = {"none": {}, "snappy": {}, "zstd": {"compression_level": 3}}
DECOMP = {"snappy": ("k_snap_walk_link", "k_snap_fix", "k_snap_frag", "k_snappy_serial"), "zstd": ("k_zstd_page",), "none": ()}
MODEL = {"snappy": "k_snap_frag", "zstd": "k_zstd_page"}


# ---- the page bodies of a file (Thrift compact protocol, PageHeader only) ----
def _varint(b, p):
    v = s = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, p


def _struct(b, p):
    """{field id: value} of a compact-protocol struct (ints un-zigzagged, nested structs as dicts), end."""
    out, fid = {}, 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        t = h & 15
        if h >> 4:
            fid += h >> 4
        else:
            z, p = _varint(b, p)
            fid = (z >> 1) ^ -(z & 1)
        out[fid], p = _value(b, p, t)


def _value(b, p, t):
    if t in (1, 2):
        return t == 1, p
    if t == 3:
        return b[p], p + 1
    if t in (4, 5, 6):
        z, p = _varint(b, p)
        return (z >> 1) ^ -(z & 1), p
    if t == 7:
        return None, p + 8
    if t == 8:
        n, p = _varint(b, p)
        return None, p + n
    if t in (9, 10):
        h = b[p]
        p += 1
        n = h >> 4
        if n == 15:
            n, p = _varint(b, p)
        for _ in range(n):
            _, p = _value(b, p, h & 15) if h & 15 not in (1, 2) else (None, p + 1)
        return None, p
    if t == 12:
        return _struct(b, p)
    raise ValueError("thrift type %d" % t)


def page_bodies(path):
    """(compressed body, uncompressed size) of every compressed page of the file, v2 level prefixes left out."""
    import pyarrow.parquet as pq
    md = pq.ParquetFile(path).metadata
    out = []
    with open(path, "rb") as f:
        for g in range(md.num_row_groups):
            for c in range(md.num_columns):
                col = md.row_group(g).column(c)
                if col.compression == "UNCOMPRESSED":
                    continue
                start = col.dictionary_page_offset if col.has_dictionary_page and col.dictionary_page_offset else col.data_page_offset
                f.seek(start)
                buf = f.read(col.total_compressed_size)
                p = 0
                while p < len(buf):
                    h, p = _struct(buf, p)
                    usize, csize = h[2], h[3]
                    v2 = h.get(8)
                    lv = (v2.get(5, 0) + v2.get(6, 0)) if v2 else 0
                    if not (v2 and v2.get(7) is False):
                        out.append((bytes(buf[p + lv:p + csize]), usize - lv))
                    p += csize
    return out


def host_decompress(paths, codec):
    import pyarrow as pa
    bodies = [b for p in paths for b in page_bodies(p)]
    c = pa.Codec(codec)
    t0 = time.perf_counter()
    n = 0
    for body, usize in bodies:
        n += c.decompress(body, decompressed_size=usize).size if usize else 0
    return {"pages": len(bodies), "compressed_bytes": sum(len(b) for b, _ in bodies), "output_bytes": n,
            "host_ms_one_thread": round((time.perf_counter() - t0) * 1e3, 1)}


# ---- steps ----
def table_dir(root, name):
    return os.path.join(root, "ckpt-" + name)


def write_tables(root, rows, parts):
    from delta_amd import synth
    out = {}
    for name, extra in CODECS.items():
        info = synth.write_table(table_dir(root, name), synth.TableSpec(n_adds=rows, n_parts=parts, n_commits=2,
                                                                         compression=name, extra=dict(extra)))
        out[name] = info["checkpoint_files"]
    return out


def child_scan(root, name):
    from delta_amd import kernel as K
    eng = K.GpuEngine(timing=True)
    out = {"step": "scan", "codec": name, "scan_ms": []}
    for _ in range(3):
        snap = K.Table.forPath(eng, table_dir(root, name)).getLatestSnapshot(eng)
        scan = snap.getScanBuilder().build()
        t0 = time.perf_counter()
        n = sum(len(b.selected_rows()) for b in scan.getScanFiles(eng))
        out["scan_ms"].append(round((time.perf_counter() - t0) * 1e3, 1))
        st = scan.kernel_stats()
        out["scan_files"] = n
        out["checkpoint_open_ms"] = round(scan.prepare_ms.get("checkpoint_open", 0.0), 1)
        # average time per launch x launches (all passes so far); a sliced open launches once per slice
        out["kernels_us_x_launches"] = {k: [round(v[0], 1), v[1]] for k, v in sorted(st.items(), key=lambda kv: -kv[1][0] * kv[1][1])
                                        if v[1] and k != "step_total"}
        if name in MODEL:
            us_per_pass = sum(st[k][0] * st[k][1] for k in DECOMP[name] if k in st) / len(out["scan_ms"])
            _, wr = scan.ckpt.kernel_traffic(MODEL[name])
            out["decompress"] = {"kernels": [k for k in DECOMP[name] if k in st and st[k][1]], "us_per_pass": round(us_per_pass, 1),
                                 "output_bytes": wr, "output_gbs": round(wr / (us_per_pass * 1e-6) / 1e9, 2) if us_per_pass else None}
        scan.close()
    eng.close()
    return out


def step(args, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    except subprocess.TimeoutExpired:
        print(json.dumps({"step": args[0], "codec": args[2], "error": "timeout after %d s" % timeout}), flush=True)
        return False
    if r.returncode != 0:
        print(json.dumps({"step": args[0], "codec": args[2], "error": "exit %d" % r.returncode, "stderr": r.stderr[-400:]}),
              flush=True)
        return False
    print(r.stdout.strip().splitlines()[-1], flush=True)
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--no-device", action="store_true", help="write the tables and time the host decompression only")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_scan(a.child[1], a.child[2])), flush=True)
        return 0
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        files = write_tables(root, a.rows, a.parts)
        print(json.dumps({"step": "write", "rows": a.rows, "parts": a.parts, "seconds": round(time.perf_counter() - t0, 1),
                          "checkpoint_bytes": {k: sum(os.path.getsize(p) for p in v) for k, v in files.items()}}), flush=True)
        for name in ("snappy", "zstd"):
            print(json.dumps(dict(host_decompress(files[name], name), step="host_decompress", codec=name)), flush=True)
        for name in () if a.no_device else CODECS:
            if not step(["scan", root, name], a.step_timeout):
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
