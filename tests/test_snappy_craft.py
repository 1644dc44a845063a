"""The snappy decoder on legal streams Google's encoder never writes, and on malformed ones
(tests/snappy_craft.py; its CPU half, tests/test_snappy_craft_host.py, holds the corpus and the
reference decoder to pyarrow).

Every valid case is decoded in the three modes of tests/test_snappy_modes.py -- one child process per
mode, the mode is read once per process -- and must equal the reference byte for byte. Beside the
bytes, each case states which path has to decode it (ParquetSet.snappy_serial): a tag across a
64 KiB output boundary or a copy reaching back across one sends the page to k_snappy_serial in the two
fragment modes, and nothing else may -- a case that went serial would not have run the fragment path
it is there to test. Page mode decodes every page in order and flags none.

Every malformed case must fail with the reference's "Error reading Parquet file: <path>", and the
engine must scan a clean table afterwards.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from tests import snappy_craft as sc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = [{}, {"DK_SNAPPY_MODE": "frag"}, {"DK_SNAPPY_MODE": "page"}]
MODE_IDS = ["hybrid-bitmap", "frag-no-bitmap", "page"]
TINY_PAGES = 6


def _strings_digest(values):
    h = hashlib.sha256()
    for b in values:
        h.update(len(b).to_bytes(4, "little"))
        h.update(b)
    return h.hexdigest()


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The files, and what each must decode to: written once, shared by the three modes."""
    d = tmp_path_factory.mktemp("snappy_craft")
    files, want = {}, {}
    for case in sc.valid_cases():
        files[case.name] = str(d / (case.name + ".parquet"))
        sc.write_case(files[case.name], case)
        want[case.name] = {"v": hashlib.sha256(case.out).hexdigest(), "serial": [1, case.serial]}
    files["tiny"] = str(d / "tiny.parquet")
    tiny = sc.write_tiny(files["tiny"])
    want["tiny"] = {"v": hashlib.sha256(tiny["v"]).hexdigest(), "s": _strings_digest(tiny["s"]),
                    "serial": [TINY_PAGES, sc.TINY_SERIAL]}
    bad = {}
    for b in sc.malformed_cases():
        bad[b.name] = str(d / ("bad_" + b.name + ".parquet"))
        sc.write_malformed(bad[b.name], b)
    from delta_amd import synth
    clean = str(tmp_path_factory.mktemp("clean"))
    synth.write_table(clean, synth.TableSpec(n_adds=2_000, n_commits=3, compression="snappy"))
    return files, want, bad, clean


def _child_valid(files):
    """Run in a child process: decode every file, digest every column, report the serial pages."""
    from delta_amd import kernel as K
    eng = K.GpuEngine()
    out = {}
    for name, path in files.items():
        leaves = ["v", "s"] if name == "tiny" else ["v"]
        ps = K.ParquetSet(eng, [path], leaves).decode()
        r = {"v": hashlib.sha256(bytes(ps.column(0, "v").fixed)).hexdigest(), "serial": list(ps.snappy_serial())}
        if "s" in leaves:
            c = ps.column(0, "s")
            r["s"] = _strings_digest(bytes(c.chars[c.offs[i]:c.offs[i + 1]]) for i in range(c.n_rows))
        ps.close()
        out[name] = r
    eng.close()
    return out


def _child_malformed(bad, clean):
    """Run in a child process: the error text of every file (None: it decoded), then a clean scan
    with the same engine against the oracle (test_errors._still_usable)."""
    from delta_amd import kernel as K
    from delta_amd._lib import DkError
    from tests.parity_util import assert_same, oracle_scan, product_scan
    eng = K.GpuEngine()
    out = {}
    for name, path in bad.items():
        ps = None
        try:
            ps = K.ParquetSet(eng, [path], ["v"]).decode()
            out[name] = None
        except DkError as e:
            out[name] = str(e)
        if ps is not None:
            ps.close()
    assert_same(product_scan(clean, engine=eng), oracle_scan(clean))
    out["_still_usable"] = True
    eng.close()
    return out


def _run(fn, args, env):
    code = ("import sys, json; sys.path.insert(0, %r); from tests import test_snappy_craft as T; "
            "print(json.dumps(getattr(T, %r)(*json.loads(%r))))" % (ROOT, fn, json.dumps(args)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("env", MODES, ids=MODE_IDS)
def test_gpu_crafted_streams_equal_reference(corpus, env):
    files, want, _, _ = corpus
    got = _run("_child_valid", [files], env)
    page_mode = env.get("DK_SNAPPY_MODE") == "page"
    wrong = {}
    for name, w in want.items():
        w = dict(w, serial=[w["serial"][0], 0]) if page_mode else w
        if got.get(name) != w:
            wrong[name] = {k: (got.get(name, {}).get(k), v) for k, v in w.items() if got.get(name, {}).get(k) != v}
    assert not wrong, "(got, want) per case: %r" % wrong


@pytest.mark.gpu
@pytest.mark.parametrize("env", MODES, ids=MODE_IDS)
def test_gpu_malformed_streams_are_reported(corpus, env):
    _, _, bad, clean = corpus
    got = _run("_child_malformed", [bad, clean], env)
    wrong = {name: got.get(name) for name, path in bad.items()
             if not (got.get(name) or "").startswith("Error reading Parquet file: " + path)}
    assert not wrong, "no such error for: %r" % wrong
    assert got["_still_usable"] is True
