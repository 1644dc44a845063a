"""One merged pass over in-process owner worlds 2 and 3 next to the unsharded reader, on the test
table of tests/test_scan_merge.py: bytes copied from the device and wall time (raw batches, released
at once; every window ends in a stream synchronise; the replays are outside the timed region). The
ranks share one GPU, so these are one-GPU rehearsal numbers, not a node measurement. Prints one JSON
line."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_scan_merge as T   # noqa: E402

T._torch_first()
from delta_amd import shard, synth       # noqa: E402

REPS = 9


def drain(next_raw, release):
    n = 0
    while True:
        got = next_raw()
        if got is None:
            return n
        release(got[0])
        n += 1


def merged_pass(w, **kw):
    t0 = time.perf_counter()
    readers = [w.K.ScanFileReader(sc, **kw) for sc in w.scans]
    m = shard.ScanFileMerge(readers)
    n = drain(m.next_raw, m.release)
    st = [rd.stats() for rd in readers]
    m.close()
    for rd in readers:
        rd.close()
    return (time.perf_counter() - t0) * 1e3, sum(s["d2h_bytes"] for s in st), n, sum(s["rows"] for s in st)


def plain_pass(w, plain, **kw):
    t0 = time.perf_counter()
    rd = w.K.ScanFileReader(plain, **kw)
    n = drain(rd.next_raw, rd.release)
    st = rd.stats()
    rd.close()
    return (time.perf_counter() - t0) * 1e3, st["d2h_bytes"], n, st["rows"]


out = {}
with tempfile.TemporaryDirectory() as d:
    synth.write_table(d, synth.TableSpec(**T.SPEC))
    for world in (2, 3):
        w = T.World(d, world, "owner")
        plain = w.plain_scan(d)
        for compact in (True, False):
            kw = dict(compact=compact, batch_rows=1000)
            merged_pass(w, **kw), plain_pass(w, plain, **kw)          # warm-up
            a, b = [], []
            for _ in range(REPS):                                       # alternating
                a.append(merged_pass(w, **kw))
                b.append(plain_pass(w, plain, **kw))
            key = "world%d_%s" % (world, "compact" if compact else "full")
            out[key] = dict(
                merged_ms=[round(x[0], 3) for x in a], plain_ms=[round(x[0], 3) for x in b],
                merged_ms_median=round(statistics.median(x[0] for x in a), 3),
                plain_ms_median=round(statistics.median(x[0] for x in b), 3),
                merged_bytes=a[0][1], plain_bytes=b[0][1], merged_batches=a[0][2], plain_batches=b[0][2],
                merged_rows=a[0][3], plain_rows=b[0][3])
        plain.close()
        w.close()
print(json.dumps(out))
