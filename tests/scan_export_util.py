"""Helpers for the scan-file batch reader's tests: reduce dk_scan_next batches to the canonical row
tuples of oracle.ref.canon_add_from_cols (plus the table root), reading the C layout directly --
validity bits, int32 offsets, value_offset -- rather than through delta_amd.kernel.BatchColumn."""
import ctypes as C

import numpy as np

from oracle.ref import STATS_LEAF


def _view(ptr, n, dtype):
    if not ptr or n <= 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(int(n),))


class RawColumn:
    """One dk_batch_column. Value-indexed arrays are viewed from their base: value i of the batch is
    at index value_offset + i, a repeated leaf's row r holds values [row_offs[r], row_offs[r + 1])."""

    def __init__(self, c, n_rows):
        self.present = bool(c.present)
        self.n_rows = n_rows
        self.phys, self.width, self.max_def, self.max_rep, self.rep_def = c.phys, c.width, c.max_def, c.max_rep, c.rep_def
        self.row_def = _view(c.row_def, n_rows, np.uint8)
        if not self.present:
            return
        self.v0, self.nv = int(c.value_offset), int(c.n_values)
        end = self.v0 + self.nv
        if self.max_rep > 0:
            self.row_offs = _view(c.row_offs, n_rows + 1, np.int32)
            assert self.row_offs.dtype == np.int32
            assert n_rows == 0 or (self.row_offs[0] == self.v0 and self.row_offs[n_rows] == end)
            assert np.all(np.diff(self.row_offs) >= 0)
            self.entry_def = _view(c.entry_def, end, np.uint8)
        else:
            assert self.nv == n_rows
        self.valid = np.unpackbits(_view(c.validity, (end + 7) // 8, np.uint8), bitorder="little")[:end].astype(bool)
        # a validity bit is set exactly where the definition level reaches the leaf
        levels = self.entry_def[self.v0:end] if self.max_rep > 0 else self.row_def
        assert np.array_equal(self.valid[self.v0:end], levels == self.max_def)
        if self.phys == 6:
            self.offs = _view(c.offs, end + 1, np.int32)
            assert np.all(np.diff(self.offs[self.v0:]) >= 0)
            self.chars = _view(c.chars, int(self.offs[end]) if end + 1 <= len(self.offs) else 0, np.uint8)
        else:
            self.fixed = _view(c.fixed, end * self.width, np.uint8)

    def string(self, v):
        return bytes(self.chars[self.offs[v]:self.offs[v + 1]])

    def str_row(self, r):
        if not self.present or not self.valid[self.v0 + r]:
            return None
        return self.string(self.v0 + r)

    def fixed_row(self, r, dtype):
        if not self.present or not self.valid[self.v0 + r]:
            return None
        w = np.dtype(dtype).itemsize
        v = self.v0 + r
        return self.fixed[v * w:(v + 1) * w].view(dtype)[0].item()


def _map_row(kc, vc, r):
    if not kc.present or kc.row_def[r] < kc.rep_def - 1:
        return None
    out = []
    for j in range(int(kc.row_offs[r]), int(kc.row_offs[r + 1])):
        v = vc.string(j) if vc.present and vc.valid[j] else None
        out.append((kc.string(j), v))
    return tuple(out)


class _Absent:
    present = False

    @staticmethod
    def str_row(r):
        return None

    @staticmethod
    def fixed_row(r, dtype):
        return None


def canon_row(cols, r):
    """canon_add_from_cols over RawColumns (cols: leaf -> RawColumn; a leaf that was not requested
    reads as absent)."""
    g = lambda leaf: cols.get(leaf, _Absent)       # noqa: E731
    dvst = g("add.deletionVector.storageType")
    dv = None
    if dvst.present and dvst.row_def[r] >= 2:
        dv = (dvst.str_row(r), g("add.deletionVector.pathOrInlineDv").str_row(r),
              g("add.deletionVector.offset").fixed_row(r, np.int32),
              g("add.deletionVector.sizeInBytes").fixed_row(r, np.int32),
              g("add.deletionVector.cardinality").fixed_row(r, np.int64))
    dc = g("add.dataChange")
    dcv = dc.fixed_row(r, np.uint8) if dc.present else None
    row = (g("add.path").str_row(r),
           _map_row(g("add.partitionValues.key_value.key"), g("add.partitionValues.key_value.value"), r),
           g("add.size").fixed_row(r, np.int64), g("add.modificationTime").fixed_row(r, np.int64),
           None if dcv is None else bool(dcv), dv,
           _map_row(g("add.tags.key_value.key"), g("add.tags.key_value.value"), r),
           g("add.baseRowId").fixed_row(r, np.int64), g("add.defaultRowCommitVersion").fixed_row(r, np.int64))
    if STATS_LEAF in cols:
        row = row + (cols[STATS_LEAF].str_row(r),)
    return row


class RawBatch:
    """What the tests keep of one dk_scan_next batch (copies; the dk_batch itself is released)."""

    def __init__(self, reader, raw, sel, table_root, decode=True):
        b = raw.contents
        self.file, self.n_rows, self.n_cols = int(b.file), int(b.n_rows), int(b.n_cols)
        assert self.n_cols == len(reader.leaves)
        self.row_index = _view(b.row_index, self.n_rows, np.int64).copy()
        assert len(self.row_index) == self.n_rows
        self.selection = _view(sel, self.n_rows, np.uint8).astype(bool) if sel else None
        self.cols = {leaf: RawColumn(b.cols[i], self.n_rows, ) for i, leaf in enumerate(reader.leaves)}
        keep = range(self.n_rows) if self.selection is None else np.nonzero(self.selection)[0]
        self.rows = [canon_row(self.cols, int(r)) + (table_root,) for r in keep] if decode else None
        self.present = {leaf: c.present for leaf, c in self.cols.items()}
        self.cols = None                       # views of the window: not kept past the release


def read_batches(reader, table_root, decode=True):
    """Every remaining batch of a delta_amd.kernel.ScanFileReader as RawBatch, each released."""
    out = []
    while True:
        got = reader.next_raw()
        if got is None:
            return out
        try:
            out.append(RawBatch(reader, got[0], got[1], table_root, decode))
        finally:
            reader.release(got[0])


def scan_rows(batches):
    """The selected rows of the batches, in order (canonical tuples + table root)."""
    return [row for b in batches for row in b.rows]
