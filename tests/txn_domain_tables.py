"""Hand-written tables for the txn / domainMetadata replay tests: commit JSON written line by line,
checkpoints written with pyarrow in the checkpoint schema's column names."""
import json
import os

import pyarrow as pa
import pyarrow.parquet as pq

from delta_amd import synth

STR = pa.string()
TXN_T = pa.struct([("appId", STR), ("version", pa.int64()), ("lastUpdated", pa.int64())])
DOM_T = pa.struct([("domain", STR), ("configuration", STR), ("removed", pa.bool_())])
ADD_T = pa.struct([("path", STR), ("partitionValues", synth.MAP_SS), ("size", pa.int64()),
                   ("modificationTime", pa.int64()), ("dataChange", pa.bool_())])

PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}
METADATA = {"id": "t", "format": {"provider": "parquet", "options": {}}, "schemaString": synth.SCHEMA_STRING,
            "partitionColumns": [], "configuration": {}, "createdTime": 1}


def txn(app, version, last=None):
    return {"txn": {"appId": app, "version": version, "lastUpdated": last}}


def dom(domain, conf="{}", removed=False):
    return {"domainMetadata": {"domain": domain, "configuration": conf, "removed": removed}}


def add(path):
    return {"add": {"path": path, "partitionValues": {}, "size": 1, "modificationTime": 1, "dataChange": True}}


def pm():
    return [{"protocol": PROTOCOL}, {"metaData": METADATA}]


def write_commit(table, version, actions):
    log = os.path.join(table, "_delta_log")
    os.makedirs(log, exist_ok=True)
    with open(os.path.join(log, "%020d.json" % version), "w", encoding="utf-8") as f:
        for a in actions:
            f.write(json.dumps(a, ensure_ascii=False) + "\n")


def _struct_col(n, rows, typ):
    """n rows of `typ`, null except rows[r] = value dict."""
    vals = [None] * n
    for r, v in rows.items():
        vals[r] = v
    return pa.array(vals, type=typ)


def txn_column(n, rows):
    """n txn rows: rows[r] = (appId or None, version); every other row is a null struct."""
    return _struct_col(n, {r: {"appId": a, "version": v, "lastUpdated": None} for r, (a, v) in rows.items()}, TXN_T)


def write_txn_file(path, n, rows, **kw):
    """A Parquet file with the one column `txn` (what the lookups read of a checkpoint part)."""
    pq.write_table(pa.table({"txn": txn_column(n, rows)}), path, **kw)


def checkpoint_table(n, txns=None, doms=None, with_pm=True, sidecars=None):
    """A checkpoint part of n rows: rows 0 / 1 protocol / metaData (with_pm), txns[r] = (appId,
    version), doms[r] = (domain, configuration, removed), sidecars: paths appended as sidecar rows;
    every other row an add."""
    txns, doms = dict(txns or {}), dict(doms or {})
    taken = set(txns) | set(doms) | ({0, 1} if with_pm else set())
    assert len(taken) == len(txns) + len(doms) + (2 if with_pm else 0) and all(r < n for r in taken)
    side = list(sidecars or [])
    total = n + len(side)
    proto = dict(PROTOCOL, readerFeatures=None, writerFeatures=None)
    meta = dict(METADATA, name=None, description=None, format={"provider": "parquet", "options": []}, configuration=[])
    cols = {
        "txn": _struct_col(total, {r: {"appId": a, "version": v, "lastUpdated": None} for r, (a, v) in txns.items()}, TXN_T),
        "add": _struct_col(total, {r: {"path": "f%d" % r, "partitionValues": [], "size": 1, "modificationTime": 1,
                                       "dataChange": False} for r in range(n) if r not in taken}, ADD_T),
        "metaData": _struct_col(total, {1: meta} if with_pm else {}, synth.METADATA_TYPE),
        "protocol": _struct_col(total, {0: proto} if with_pm else {}, synth.PROTOCOL_TYPE),
        "domainMetadata": _struct_col(total, {r: {"domain": d, "configuration": c, "removed": x}
                                              for r, (d, c, x) in doms.items()}, DOM_T)}
    if sidecars is not None:
        cols["sidecar"] = _struct_col(total, {n + i: {"path": p, "sizeInBytes": 1, "modificationTime": 1, "tags": None}
                                              for i, p in enumerate(side)}, synth.SIDECAR_TYPE)
    return pa.table(cols)


def write_classic(table, version, **kw):
    pq.write_table(checkpoint_table(**kw), os.path.join(table, "_delta_log", "%020d.checkpoint.parquet" % version))


def write_multipart(table, version, parts):
    """parts: one checkpoint_table(...) argument dict per part."""
    for i, kw in enumerate(parts):
        pq.write_table(checkpoint_table(**kw), os.path.join(
            table, "_delta_log", "%020d.checkpoint.%010d.%010d.parquet" % (version, i + 1, len(parts))))
