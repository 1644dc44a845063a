"""Plain-Python restatement of the reference's two "first one wins" replays, over json and
pyarrow.parquet only (no project code): the yardstick of tests/test_txn_domain.py.

Reference (kernel/kernel-api/src/main/java/io/delta/kernel/internal/):
  LogReplay.loadLatestTransactionVersion   replay/LogReplay.java:316-342
  LogReplay.loadDomainMetadataMap          replay/LogReplay.java:356-378
  DomainMetadataUtils.populateDomainMetadataMap   util/DomainMetadataUtils.java:44-54
  LogSegment.allLogFilesReversed           snapshot/LogSegment.java:166-178
  ActionsIterator (sidecars only for add / remove read schemas)   replay/ActionsIterator.java:175-226
"""
import json
import os
import re

import pyarrow.parquet as pq

_DELTA = re.compile(r"^(\d{20})\.json$")
_CLASSIC = re.compile(r"^(\d{20})\.checkpoint\.parquet$")
_MULTI = re.compile(r"^(\d{20})\.checkpoint\.(\d{10})\.(\d{10})\.parquet$")
_V2 = re.compile(r"^(\d{20})\.checkpoint\.([^.]+)\.(json|parquet)$")


def log_files_reversed(table):
    """LogSegment.java:166-178: the commits after the newest complete checkpoint plus that
    checkpoint's top-level files, sorted by file name, descending. (Sidecars are not part of the
    segment; ActionsIterator.java:175-226 opens them only when the read schema holds add / remove.)"""
    log = os.path.join(table, "_delta_log")
    names = os.listdir(log)
    cks = {}
    for n in names:
        m = _CLASSIC.match(n) or _V2.match(n)
        if m:
            cks.setdefault(int(m.group(1)), []).append(n)
            continue
        m = _MULTI.match(n)
        if m:
            cks.setdefault(int(m.group(1)), []).append(n)
    ckv = max(cks) if cks else -1
    commits = [n for n in names if _DELTA.match(n) and int(n[:20]) > ckv]
    return [os.path.join(log, n) for n in sorted(commits + cks.get(ckv, []), reverse=True)]


def _rows(path, action):
    """The `action` value of every row of one log file, in row order (None: null)."""
    if path.endswith(".json"):
        out = []
        with open(path, "rb") as f:
            for line in f.read().decode("utf-8").splitlines():
                if line.strip():
                    out.append(json.loads(line).get(action))
        return out
    if action not in pq.read_schema(path).names:
        return []
    return pq.read_table(path, columns=[action]).column(action).to_pylist()


def latest_transaction_version(table, app_id):
    for path in log_files_reversed(table):                 # LogReplay.java:317-322
        for txn in _rows(path, "txn"):                     # :328
            if txn is None:                                # :329 isNullAt
                continue
            if app_id == txn.get("appId"):                 # :331 applicationId.equals(txn.getAppId())
                return txn["version"]                      # :332
    return None                                            # :341


def domain_metadata_map(table):
    out = {}                                               # LogReplay.java:363
    for path in log_files_reversed(table):                 # :357-362
        for dm in _rows(path, "domainMetadata"):           # DomainMetadataUtils.java:47
            if dm is None:                                 # :48 fromColumnVector -> null
                continue
            if dm["domain"] not in out:                    # :49 first seen wins, removed or not
                out[dm["domain"]] = {"domain": dm["domain"], "configuration": dm["configuration"],
                                     "removed": dm["removed"]}          # :51
    return out                                             # LogReplay.java:374


def file_matches(path, needle: bytes, from_row=0):
    """Rows >= from_row of one Parquet file whose txn is non-null and whose appId equals needle
    (UTF-8 bytes), ascending: what a walk of dk_parquet_find_bytes must list."""
    rows = pq.read_table(path, columns=["txn"]).column("txn").to_pylist()
    return [r for r, t in enumerate(rows)
            if r >= from_row and t is not None and t["appId"] is not None and t["appId"].encode("utf-8") == needle]
