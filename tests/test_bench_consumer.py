"""bench.py's JMH-shaped consumer sums add.size over the selected rows of every batch with
masked_sum (a packed-word scan for near-uniform masks, a blocked multiply-add for irregular ones);
it must equal the plain masked sum for every mask shape and length (the headline value's size_sum
is checked against the oracle only through the counters)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1000, 65536 + 3, 300001])
@pytest.mark.parametrize("frac", [0.0, 0.0005, 0.03, 0.5, 0.97, 0.9995, 1.0])
def test_masked_sum_equals_plain(bench, n, frac):
    rng = np.random.default_rng(n * 1000 + int(frac * 997))
    v = rng.integers(-(1 << 40), 1 << 40, n).astype("<i8")
    sel = rng.random(n) < frac
    assert bench.masked_sum(v, sel) == (int(v[sel].sum()), int(sel.sum()))


def test_masked_sum_on_views(bench):
    """Batches hand out views (slices of a pinned block): odd offsets and lengths."""
    rng = np.random.default_rng(7)
    base_v = rng.integers(0, 1 << 40, 100003).astype("<i8")
    base_s = rng.random(100003) < 0.999
    for a, b in [(0, 100003), (3, 99999), (17, 50017), (1, 2)]:
        v, sel = base_v[a:b], base_s[a:b]
        assert bench.masked_sum(v, sel) == (int(v[sel].sum()), int(sel.sum()))


def test_dump_outputs_files(bench, tmp_path):
    """--dump-outputs: batches are written in replay order whatever order they arrived in, the
    sampled window is the same rows in every run, and every file is float32 / float64."""
    from types import SimpleNamespace
    rng = np.random.default_rng(3)

    def batch(file_index, rows, selection=True):
        v = rng.integers(0, 1 << 40, rows).astype("<i8")
        sel = (rng.random(rows) < 0.9) if selection else None
        b = SimpleNamespace(file_index=file_index, commit_index=-1, row_offset=0, size=rows, selection=sel)
        k = rows if sel is None else int(sel.sum())
        s = int(v.sum()) if sel is None else int(v[sel].sum())
        return b, v, k, s

    batches = [batch(-1, 100), batch(0, bench.DUMP_WINDOW + 1000), batch(1, 5, selection=False)]
    for order, name in (((0, 1, 2), "a"), ((2, 0, 1), "b")):
        dumped = [bench.dump_sample(*batches[i]) for i in order] + [(1, 2, 3, 4, 5)]
        bench.dump_outputs(str(tmp_path / name), dumped, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["add_size_sample.npy", "batches.npy", "counters.npy", "selection_sample.npy"]
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert got[f].dtype in (np.float32, np.float64)
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f)), f
    assert got["counters.npy"].tolist() == [1, 2, 3, 4, 5]
    bt = got["batches.npy"]
    assert bt[:, 0].tolist() == [-1, 0, 1] and bt[:, 3].tolist() == [100, bench.DUMP_WINDOW + 1000, 5]
    assert bt[:, 4].tolist() == [b[2] for b in batches] and bt[:, 5].tolist() == [b[3] for b in batches]
    n = 100 + bench.DUMP_WINDOW + 5
    assert got["selection_sample.npy"].shape == got["add_size_sample.npy"].shape == (n,)
    start = int(bt[1, 6])
    b, v, _, _ = batches[1]
    assert np.array_equal(got["add_size_sample.npy"][100:100 + bench.DUMP_WINDOW], v[start:start + bench.DUMP_WINDOW])
    assert np.array_equal(got["selection_sample.npy"][100:100 + bench.DUMP_WINDOW],
                          b.selection[start:start + bench.DUMP_WINDOW])
    assert got["selection_sample.npy"][-5:].tolist() == [1.0] * 5
