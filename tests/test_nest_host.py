"""Nested repetition on the CPU: dk_nest.h's level-to-element rule, compiled into a stand-alone host
program (tests/native/nest_host.cpp, built with -fsanitize=address,undefined and run as a subprocess)
and checked against structures written out by hand; the new accessors are part of the C ABI; and the
pure-Python leaf view (delta_amd/nested.py) on hand-made columns."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "nest_host.cpp")
NEW = ("dk_parquet_column_nest", "dk_batch_nest")

N, E, H = 0, 1, 2          # NEST_NULL, NEST_EMPTY, NEST_HAS (dk_nest.h)

# Each case: the leaf's list_def, its (rep, def) levels, and the expected structure by hand.
CASES = {
    # array<array<int32>>, everything optional: a 1, list 2, element 3, list 4, element 5.
    #  row0 null | row1 [] | row2 [[1]] | row3 [[1,2,3], [], null, [null,4]] | row4 [null] | row5 [[]]
    "r2_lists": dict(
        list_def=[2, 4],
        rep=[0, 0, 0, 0, 2, 2, 1, 1, 1, 2, 0, 0],
        dfn=[0, 1, 5, 5, 5, 5, 3, 2, 4, 5, 2, 3],
        n=[6, 7, 6],
        offs=[[0, 0, 0, 1, 5, 6, 7], [0, 1, 4, 4, 4, 6, 6, 6]],
        defs=[[0, 1, 5, 5, 2, 3], [5, 5, 3, 2, 4, 2, 3]],
        cls=[[N, E, H, H, H, H], [H, H, E, N, H, N, E]]),
    # array<struct<tags: array<string>>>: a 1, list 2, element (struct) 3, tags 4, list 5, element 6.
    #  row0 [{tags:[x,y]}, null, {tags:null}, {tags:[]}, {tags:[null]}] | row1 null | row2 [] | row3 [null]
    "r2_null_struct_between": dict(
        list_def=[2, 5],
        rep=[0, 2, 1, 1, 1, 1, 0, 0, 0],
        dfn=[6, 6, 2, 3, 4, 5, 0, 1, 2],
        n=[4, 6, 3],
        offs=[[0, 5, 5, 5, 6], [0, 2, 2, 2, 2, 3, 3]],
        defs=[[6, 0, 1, 2], [6, 2, 3, 4, 5, 2]],
        cls=[[H, N, E, H], [H, N, N, E, H, N]]),
    # array<array<array<int32>>>: a 1, list 2, element 3, list 4, element 5, list 6, element 7.
    #  row0 [[[1,2],[]], null, [], [null,[null]]] | row1 null | row2 [] | row3 [[[7]]] | row4 [[[1],[2],[3]]]
    "r3_lists": dict(
        list_def=[2, 4, 6],
        rep=[0, 3, 2, 1, 1, 1, 2, 0, 0, 0, 0, 2, 2],
        dfn=[7, 7, 5, 2, 3, 4, 6, 0, 1, 7, 7, 7, 7],
        n=[5, 6, 8, 7],
        offs=[[0, 4, 4, 4, 5, 6], [0, 2, 2, 2, 4, 5, 8], [0, 2, 2, 2, 3, 4, 5, 6, 7]],
        defs=[[7, 0, 1, 7, 7], [7, 2, 3, 4, 7, 7], [7, 5, 4, 6, 7, 7, 7, 7]],
        cls=[[H, N, E, H, H], [H, N, E, H, H, H], [H, E, N, H, H, H, H, H]]),
    # no levels at all
    "r2_empty": dict(list_def=[1, 2], rep=[], dfn=[], n=[0, 0, 0], offs=[[0], [0]], defs=[[], []], cls=[[], []]),
}


def _cases_file(path):
    with open(path, "w") as f:
        for name, c in CASES.items():
            f.write("case %s %d %s %d\n" % (name, len(c["list_def"]), " ".join(map(str, c["list_def"])), len(c["rep"])))
            f.write(" ".join(map(str, c["rep"])) + "\n" + " ".join(map(str, c["dfn"])) + "\n")


def _parse(out):
    got, cur = {}, None
    for line in out.splitlines():
        key, _, rest = line.partition(" " if line.startswith("case") else ":")
        if key == "case":
            cur = got.setdefault(rest.strip(), {})
        else:
            cur[key] = [int(x) for x in rest.split()]
    return got


@pytest.mark.parametrize("sanitize", [True, False], ids=["asan_ubsan", "plain"])
def test_serial_walk_against_hand_written_structures(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "nest_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([cxx, "-std=c++17"] + flags + ["-I", CSRC, SRC, "-o", exe], check=True)
    cf = str(tmp_path / "cases.txt")
    _cases_file(cf)
    run = subprocess.run([exe, cf], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = _parse(run.stdout)
    assert sorted(got) == sorted(CASES)
    for name, c in CASES.items():
        g = got[name]
        assert g["n"] == c["n"], name
        for k in range(1, len(c["list_def"]) + 1):
            assert g["offs%d" % k] == c["offs"][k - 1], (name, k)
            assert g["def%d" % (k - 1)] == c["defs"][k - 1], (name, k)
            assert g["cls%d" % k] == c["cls"][k - 1], (name, k)
            assert len(c["offs"][k - 1]) == c["n"][k - 1] + 1 and c["offs"][k - 1][-1] == c["n"][k]


def test_hand_written_cases_cover_every_shape_at_every_depth():
    """At each depth of the R = 2 and R = 3 cases: a null list, an empty list, one element, many."""
    for name in ("r2_lists", "r3_lists"):
        c = CASES[name]
        for k in range(len(c["list_def"])):
            sizes = np.diff(c["offs"][k]).tolist()
            assert N in c["cls"][k] and E in c["cls"][k], (name, k)
            assert 1 in sizes and max(sizes) >= 2, (name, k)
    assert CASES["r2_null_struct_between"]["defs"][1].count(2) == 2      # the null structs


def test_header_declares_the_accessors():
    with open(os.path.join(ROOT, "include", "dkgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in names
    assert "dk_nest_level" in text and "dk_batch_nest_level" in text


def test_library_exports_the_accessors():
    from delta_amd import _lib
    so = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(so, n)
        assert n in _lib.EXPORTS
    # the existing structs keep their layout: the accessors are additions
    assert ctypes.sizeof(_lib.dk_column) == 96 and ctypes.sizeof(_lib.dk_batch_column) == 96


def _col(case, values, max_def):
    """A Column-like object over a hand-written case (values: one per innermost element)."""
    c = CASES[case]
    R = len(c["list_def"])
    nest = [(c["list_def"][k], np.array(c["defs"][k], np.uint8), np.array(c["offs"][k], np.int64)) for k in range(R)]
    entry_def = np.array([d for r, d in zip(c["rep"], c["dfn"]) if d >= c["list_def"][-1]], np.uint8)
    fixed = np.array(values, np.int32).view(np.uint8)
    return SimpleNamespace(path=case, phys=1, width=4, max_def=max_def, max_rep=R, rep_def=c["list_def"][-1],
                           row_def=nest[0][1], entry_def=entry_def, fixed=fixed, offs=None, chars=None, nest=nest)


def test_leaf_view_of_hand_written_columns():
    from delta_amd.nested import leaf_view, pylist_leaf_view
    want2 = [None, [], [[1]], [[1, 2, 3], [], None, [None, 4]], [None], [[]]]
    assert leaf_view(_col("r2_lists", [1, 1, 2, 3, 0, 4], 5)) == want2
    want3 = [[[[1, 2], []], None, [], [None, [None]]], None, [], [[[7]]], [[[1], [2], [3]]]]
    assert leaf_view(_col("r3_lists", [1, 2, 0, 7, 1, 2, 3], 7)) == want3
    assert [pylist_leaf_view(v, ["list", "list"]) for v in want2] == want2
    rows = [[{"a": 1, "tags": ["x", None]}, None, {"a": None, "tags": None}], None, [(1, [2]), (3, None)]]
    assert pylist_leaf_view(rows[0], ["list", ("field", "tags"), "list"]) == [["x", None], None, None]
    assert pylist_leaf_view(rows[0], ["list", ("field", "a")]) == [1, None, None]
    assert pylist_leaf_view(rows[2], ["list", "value", "list"]) == [[2], None]
    assert pylist_leaf_view(rows[1], ["list", "key"]) is None
