"""The scan-file batch reader's C ABI on the CPU: declared in include/dkgpu.h, listed in
_lib.EXPORTS with ctypes signatures, exported by the built library, mirrored by GpuScan."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dk_replay_scan_open", "dk_scan_next", "dk_scan_close")


def _header():
    with open(os.path.join(ROOT, "include", "dkgpu.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_declares_the_scan_reader():
    text = _header()
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, n
    m = re.search(r"typedef\s+struct\s+dk_scan_options\s*\{(.*?)\}\s*dk_scan_options\s*;", text, flags=re.S)
    assert m, "dk_scan_options is not declared"
    fields = re.findall(r"int32_t\s+(\w+)\s*;", m.group(1))
    assert fields == ["compact", "batch_rows", "window_rows"]
    assert re.search(r"typedef\s+struct\s+dk_scan_reader\s+dk_scan_reader\s*;", text)


def test_exports_list_and_signatures():
    from delta_amd import _lib
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    assert [f[0] for f in _lib.dk_scan_options._fields_] == ["compact", "batch_rows", "window_rows"]
    assert ctypes.sizeof(_lib.dk_scan_options) == 12
    L = _lib.lib()
    assert L.dk_replay_scan_open.argtypes is not None and len(L.dk_replay_scan_open.argtypes) == 5
    assert len(L.dk_scan_next.argtypes) == 3
    assert L.dk_scan_close.restype is None


def test_library_exports_the_scan_reader():
    from delta_amd import _lib
    _lib.lib()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(so, n), n


def test_python_mirror_exists():
    from delta_amd import kernel as K
    assert callable(K.GpuScan.getScanFileBatches)
    names = set(K.ScanFileBatch.__dataclass_fields__)
    assert {"columns", "selection", "row_index", "file_index", "source", "table_root", "size"} <= names
