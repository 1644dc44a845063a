#!/usr/bin/env python3
"""Nested read, measured: one array<array<int64>> file of --rows rows (0-6 x 0-6
elements a row, nulls and empties at both depths) read by the engine (open + decode + sync, cold pass
and warm ones) and by pyarrow on one host thread. Prints wall ms per pass and the nest kernels' summed
HIP event time per pass (engine timers), one JSON line at the end."""
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
from delta_amd import kernel as K  # noqa: E402

LEAF = "c.list.element.list.element"


def write_file(path, n, seed=1):
    """Built from numpy offsets (a Python list of 2M nested rows would take minutes)."""
    rng = np.random.default_rng(seed)
    outer = rng.integers(0, 7, n)
    outer_null = rng.random(n) < 0.05
    outer[outer_null] = 0
    n1 = int(outer.sum())
    inner = rng.integers(0, 7, n1)
    inner_null = rng.random(n1) < 0.05
    inner[inner_null] = 0
    n2 = int(inner.sum())
    vals = pa.array(rng.integers(-1 << 40, 1 << 40, n2), pa.int64(), mask=rng.random(n2) < 0.05)
    o2 = pa.array(np.concatenate([[0], np.cumsum(inner)]).astype(np.int32))
    l2 = pa.ListArray.from_arrays(o2, vals, mask=pa.array(inner_null))
    o1 = pa.array(np.concatenate([[0], np.cumsum(outer)]).astype(np.int32))
    l1 = pa.ListArray.from_arrays(o1, l2, mask=pa.array(outer_null))
    pq.write_table(pa.table({"c": l1}), path, compression="snappy", row_group_size=1 << 20)
    return n1, n2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "nested.parquet")
        n1, n2 = write_file(path, a.rows)
        size = os.path.getsize(path)
        pa.set_cpu_count(1)
        pa.set_io_thread_count(1)
        arrow_ms = []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            t = pq.read_table(path, use_threads=False)
            arrow_ms.append((time.perf_counter() - t0) * 1e3)
        assert t.num_rows == a.rows
        eng = K.GpuEngine(timing=True)
        wall_ms, nest_ms, decode_ms = [], [], []
        for _ in range(a.passes):
            t0 = time.perf_counter()
            ps = K.ParquetSet(eng, [path], [LEAF])
            ps.decode()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            st = ps.kernel_stats()
            nest_ms.append(sum(avg * cnt for k, (avg, cnt) in st.items() if k.startswith("k_nest")) / 1e3)
            decode_ms.append(sum(avg * cnt for k, (avg, cnt) in st.items() if k == "k_tile_decode") / 1e3)
            col = ps.column(0, LEAF, copy=False)
            assert col.n_rows == a.rows and len(col.nest) == 2
            assert int(col.nest[0][2][-1]) == n1 and int(col.nest[1][2][-1]) == n2 == len(col.entry_def)
            ps.close()
        eng.close()
    out = dict(rows=a.rows, depth1_elements=n1, values=n2, file_bytes=size,
               engine_wall_ms=[round(x, 1) for x in wall_ms], nest_kernels_ms=[round(x, 3) for x in nest_ms],
               tile_decode_ms=[round(x, 3) for x in decode_ms], pyarrow_one_thread_ms=[round(x, 1) for x in arrow_ms])
    for k, v in out.items():
        print("%-24s %s" % (k, v))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
