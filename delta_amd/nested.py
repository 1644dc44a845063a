"""Leaf views of repeated and nested leaves, in pure Python (tests, a connector's smoke check).

The leaf view of one leaf is, per row, nested Python lists where the schema has lists (or maps) on
the leaf's path, and None where a list, a struct above it or the value itself is null. It is what the
decoded layout says without any Dremel assembly: a `Column` or `BatchColumn` carries, per depth
k = 1..max_rep, `nest[k - 1] = (list_def, parent_def, offs)` (include/dkgpu.h, dk_nest_level), and the
value arrays are dense over the innermost elements.

`pylist_leaf_view` is the same view of an ordinary Python value (pyarrow's `to_pylist()` of the
column), so the two can be compared with `==`."""
import numpy as np

_DTYPES = {0: np.uint8, 1: np.int32, 2: np.int64, 4: np.float32, 5: np.float64}


def _values(col):
    """The leaf's values, one Python object per value slot (entries of a repeated leaf, else rows)."""
    defs = col.entry_def if col.max_rep > 0 else col.row_def
    n = len(defs)
    if col.phys == 6:
        chars, offs = bytes(col.chars), col.offs
        vals = [chars[offs[i]:offs[i + 1]] for i in range(n)]
    elif col.phys in _DTYPES:
        a = np.frombuffer(bytes(col.fixed), dtype=_DTYPES[col.phys])[:n]
        vals = [bool(x) for x in a] if col.phys == 0 else a.tolist()
    else:
        w, raw = col.width, bytes(col.fixed)
        vals = [raw[i * w:(i + 1) * w] for i in range(n)]
    return [v if d == col.max_def else None for v, d in zip(vals, defs.tolist())]


def nest_levels(col):
    """(list_def, parent_def, offs) per depth: `col.nest` of a nested leaf, the row offsets of a leaf
    under one repeated node, nothing for a flat leaf."""
    if col.max_rep > 1:
        if len(col.nest) != col.max_rep:
            raise ValueError("%s: max_rep %d but %d nest levels" % (col.path, col.max_rep, len(col.nest)))
        return col.nest
    if col.max_rep == 1:
        return [(col.rep_def, col.row_def, col.row_offs)]
    return []


def leaf_view(col):
    """One Python object per row of `col` (a Column or BatchColumn): see the module docstring."""
    vals = _values(col)
    levels = [(ld, np.asarray(pd).tolist(), np.asarray(of).tolist()) for ld, pd, of in nest_levels(col)]
    if not levels:
        return vals
    cur = vals                                   # the depth-k elements, innermost first
    for ld, pdef, offs in reversed(levels):
        cur = [cur[offs[j]:offs[j + 1]] if d >= ld else [] if d == ld - 1 else None
               for j, d in enumerate(pdef)]
    return cur


def pylist_leaf_view(value, steps):
    """The leaf view of one row's Python value. steps: the leaf's path as a sequence of "list" (a
    list: every element), ("field", name) (a struct as a dict), "key" / "value" (a map entry as a
    (key, value) pair; the map itself is a "list" step before it)."""
    if value is None:
        return None
    if not steps:
        return value
    s, rest = steps[0], steps[1:]
    if s == "list":
        return [pylist_leaf_view(v, rest) for v in value]
    if s == "key":
        return pylist_leaf_view(value[0], rest)
    if s == "value":
        return pylist_leaf_view(value[1], rest)
    return pylist_leaf_view(value[s[1]], rest)
