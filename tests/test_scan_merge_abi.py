"""The sharded scan's streaming ABI on the CPU: dk_replay_scan_open_rank, dk_scan_batch_order,
dk_scan_merge_* and dk_replay_counters_sum are declared in include/dkgpu.h, listed in _lib.EXPORTS with
ctypes signatures, exported by the built library and mirrored in Python; the calls that need no
device fail cleanly without one."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dk_replay_scan_open_rank", "dk_scan_batch_order", "dk_scan_batch_selection", "dk_scan_merge_open",
         "dk_scan_merge_next", "dk_scan_merge_close", "dk_replay_counters_sum")
OPTION_FIELDS = ["compact", "batch_rows", "window_rows", "emit_tail", "n_ckpt_files", "n_tail_files",
                 "ckpt_index", "tail_index"]


def _header():
    with open(os.path.join(ROOT, "include", "dkgpu.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_the_rank_reader_and_the_merge():
    text = _header()
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, n
    m = re.search(r"typedef\s+struct\s+dk_rank_scan_options\s*\{(.*?)\}\s*dk_rank_scan_options\s*;", text, flags=re.S)
    assert m, "dk_rank_scan_options is not declared"
    fields = [n for decl in re.findall(r"(?:const\s+)?int32_t\s*\*?\s*([\w\s,]+);", m.group(1))
              for n in re.split(r"\s*,\s*", decl.strip())]
    assert fields == OPTION_FIELDS
    assert re.search(r"typedef\s+struct\s+dk_scan_merge\s+dk_scan_merge\s*;", text)
    # dk_scan_options did not grow
    m = re.search(r"typedef\s+struct\s+dk_scan_options\s*\{(.*?)\}\s*dk_scan_options\s*;", text, flags=re.S)
    assert re.findall(r"int32_t\s+(\w+)\s*;", m.group(1)) == ["compact", "batch_rows", "window_rows"]


def test_exports_list_and_signatures():
    from delta_amd import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    assert [f[0] for f in _lib.dk_rank_scan_options._fields_] == OPTION_FIELDS
    assert C.sizeof(_lib.dk_rank_scan_options) == 6 * 4 + 2 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.dk_scan_options) == 12
    L = _lib.lib()
    assert len(L.dk_replay_scan_open_rank.argtypes) == 5
    assert len(L.dk_scan_batch_order.argtypes) == 2
    assert len(L.dk_scan_merge_open.argtypes) == 3 and len(L.dk_scan_merge_next.argtypes) == 3
    assert L.dk_scan_merge_close.restype is None
    assert len(L.dk_replay_counters_sum.argtypes) == 3


def test_library_exports_the_symbols():
    from delta_amd import _lib
    _lib.lib()
    so = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(so, n), n


def test_python_mirror_exists():
    from delta_amd import kernel as K, shard
    fields = K.ScanFileBatch.__dataclass_fields__
    assert "order" in fields and fields["order"].default is None
    assert callable(shard.merged_scan_file_batches) and callable(shard.merged_counters)
    assert callable(shard.ScanFileMerge.next_raw)
    assert "order" in shard.merged_scan_file_batches.__doc__ or "order" in K.ScanFileReader.__doc__


def test_calls_without_a_device_fail_cleanly():
    """No reader, no batch, no replay: each call returns non-zero with a message that names it, touches
    no device (this test runs without one) and leaves the outputs cleared."""
    from delta_amd import _lib
    from delta_amd._lib import DkError, check
    L = _lib.lib()
    key = (C.c_int64 * 3)(7, 7, 7)
    with pytest.raises(DkError, match="dk_scan_batch_order"):
        check(L.dk_scan_batch_order(None, key))
    assert list(key) == [7, 7, 7]
    m = C.c_void_p(1)
    with pytest.raises(DkError, match="dk_scan_merge_open: no readers"):
        check(L.dk_scan_merge_open(None, 0, C.byref(m)))
    assert not m.value
    hs = (C.c_void_p * 1)(None)
    with pytest.raises(DkError, match="dk_scan_merge_open: null reader"):
        check(L.dk_scan_merge_open(hs, 1, C.byref(m)))
    with pytest.raises(DkError, match="dk_scan_merge_open"):
        check(L.dk_scan_merge_open(hs, 0, C.byref(m)))
    out, rank = C.POINTER(_lib.dk_batch)(), C.c_int32(5)
    with pytest.raises(DkError, match="dk_scan_merge_next: null merge"):
        check(L.dk_scan_merge_next(None, C.byref(out), C.byref(rank)))
    assert not out and rank.value == -1
    L.dk_scan_merge_close(None)                       # a no-op
    cnt = (C.c_int64 * 5)()
    with pytest.raises(DkError, match="dk_replay_counters_sum"):
        check(L.dk_replay_counters_sum(None, 0, cnt))
    rd = C.c_void_p(1)
    opt = _lib.dk_rank_scan_options()
    with pytest.raises(DkError, match="dk_replay_scan_open_rank: null replay"):
        check(L.dk_replay_scan_open_rank(None, None, 0, C.byref(opt), C.byref(rd)))
    assert not rd.value
    sel = C.c_void_p(1)
    with pytest.raises(DkError, match="dk_scan_batch_selection"):
        check(L.dk_scan_batch_selection(None, C.byref(sel)))
