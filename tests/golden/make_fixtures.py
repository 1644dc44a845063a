"""Copies the `_delta_log` of selected reference golden tables into tests/golden/tables/ (data
fixtures: inputs) and records the oracle's answers for them in tests/golden/expected.json (outputs).
The oracle itself is pinned to the answers the reference's tests assert
(tests/test_oracle_golden.py). Run where a checkout of the reference project is at hand:

    python tests/golden/make_fixtures.py REFERENCE_ROOT [tables|oracle|schema ...]

  tables  tests/golden/tables/ + expected.json (the default, with the two below)
  oracle  what tests/test_oracle_golden.py reads beside tests/golden/tables/: the `_delta_log` of the
          golden tables it replays that are not under tables/ (tests/golden/oracle_tables/), and
          data_files.json: each table's data-file names, row counts and `id` values
  schema  checkpoint_schema_fields.json: field names and nullability of the reference's action
          schemas, as tests/test_checkpoint_schema.py restates them
"""
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref  # noqa: E402

REFERENCE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ""
GOLD = os.path.join(REFERENCE, "connectors/golden-tables/src/main/resources/golden")
KDRES = os.path.join(REFERENCE, "kernel/kernel-defaults/src/test/resources")
ACTIONS = os.path.join(REFERENCE, "kernel/kernel-api/src/main/java/io/delta/kernel/internal/actions")
TABLES = {
    "checkpoint": GOLD, "snapshot-data3": GOLD, "snapshot-repartitioned": GOLD, "log-replay-dv-key-cases": GOLD,
    "log-replay-special-characters-a": GOLD, "log-replay-special-characters-b": GOLD,
    "delete-re-add-same-file-different-transactions": GOLD, "multi-part-checkpoint": GOLD,
    "basic-with-inserts-deletes-checkpoint": GOLD, "only-checkpoint-files": GOLD, "v2-checkpoint-parquet": GOLD,
    "v2-checkpoint-json": GOLD,
    "dv-partitioned-with-checkpoint": GOLD, "data-skipping-basic-stats-all-types-checkpoint": GOLD,
    "data-skipping-basic-stats-all-types": GOLD, "data-skipping-basic-stats-all-types-columnmapping-name": GOLD,
    "data-skipping-basic-stats-all-types-columnmapping-id": GOLD,
    "data-skipping-change-stats-collected-across-versions": GOLD, "data-skipping-partition-and-data-column": GOLD,
    "basic-dv-with-checkpoint": KDRES, "basic-with-checkpoint": KDRES,
    "data-reader-partition-values": GOLD, "data-reader-timestamp_ntz": GOLD,
    "data-reader-timestamp_ntz-name-mode": GOLD, "data-reader-timestamp_ntz-id-mode": GOLD,
}


def canon_json(rows):
    """Rows as JSON; the machine-dependent tableRoot prefix becomes ${TABLES} (tests/golden_util.py)."""
    from tests.golden_util import to_json_rows
    return to_json_rows(rows)


# tables of tests/test_oracle_golden.py: replayed from tables/ where that has them, else from
# oracle_tables/; their data files are represented by data_files.json
ORACLE_TABLES = ["checkpoint", "snapshot-data0", "snapshot-data1", "snapshot-data2", "snapshot-data3",
                 "snapshot-data2-deleted", "snapshot-repartitioned", "snapshot-vacuumed", "log-replay-dv-key-cases",
                 "log-replay-special-characters-a", "log-replay-special-characters-b",
                 "delete-re-add-same-file-different-transactions", "basic-with-inserts-deletes-checkpoint",
                 "only-checkpoint-files", "multi-part-checkpoint", "basic-with-inserts-overwrite-restore",
                 "v2-checkpoint-json", "v2-checkpoint-parquet"]

# struct -> (file, constant) of its schema definition (tests/test_checkpoint_schema.py)
JAVA = {"add": ("AddFile.java", "SCHEMA_WITHOUT_STATS"), "remove": ("RemoveFile.java", "FULL_SCHEMA"),
        "deletionVector": ("DeletionVectorDescriptor.java", "READ_SCHEMA"), "metaData": ("Metadata.java", "FULL_SCHEMA"),
        "format": ("Format.java", "FULL_SCHEMA"), "protocol": ("Protocol.java", "FULL_SCHEMA"),
        "txn": ("SetTransaction.java", "FULL_SCHEMA"), "domainMetadata": ("DomainMetadata.java", "FULL_SCHEMA")}


def oracle_fixtures():
    import pyarrow.parquet as pq
    data = {}
    for name in ORACLE_TABLES:
        root = os.path.join(GOLD, name)
        if not os.path.isdir(os.path.join(HERE, "tables", name)):
            dst = os.path.join(HERE, "oracle_tables", name, "_delta_log")
            shutil.rmtree(os.path.dirname(dst), ignore_errors=True)
            shutil.copytree(os.path.join(root, "_delta_log"), dst)
        files = {}
        for d, dirs, names in os.walk(root):
            dirs[:] = sorted(x for x in dirs if x != "_delta_log")
            for f in sorted(names):
                if not f.endswith(".parquet"):
                    continue
                t = pq.read_table(os.path.join(d, f))
                rel = os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/")
                files[rel] = {"num_rows": t.num_rows}
                if "id" in t.column_names:
                    files[rel]["id"] = t.column("id").to_pylist()
        data[name] = {"dir": sorted(f for f in os.listdir(root) if os.path.isfile(os.path.join(root, f))),
                      "files": files}
        print(name, len(data[name]["dir"]), "entries,", len(files), "data files")
    with open(os.path.join(HERE, "data_files.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True))
                                   for k, v in sorted(data.items())) + "\n}\n")     # one table per line


def schema_fixtures():
    """[(field, nullable)] in declaration order, from the `.add("name", TYPE[, nullable])` calls of
    each schema constant (StructType.add(name, type) defaults to nullable)."""
    import re
    out = {}
    for struct, (fname, const) in JAVA.items():
        with open(os.path.join(ACTIONS, fname)) as f:
            text = f.read()
        at = text.index(const + " =")
        body = text[at:text.index(";", at)]
        fields = []
        for seg in body.split(".add(")[1:]:
            args, depth, cur = [], 0, ""
            for ch in seg:
                if ch == ")" and depth == 0:
                    break
                depth += (ch == "(") - (ch == ")")
                if ch == "," and depth == 0:
                    args.append(cur)
                    cur = ""
                else:
                    cur += ch
            args.append(cur)
            args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in args]
            fields.append([re.match(r'"(\w+)"', args[0]).group(1), args[2] == "true" if len(args) > 2 else True])
        out[struct] = {"file": fname, "constant": const, "fields": fields}
    with open(os.path.join(HERE, "checkpoint_schema_fields.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True))
                                   for k, v in sorted(out.items())) + "\n}\n")      # one struct per line


def table_fixtures():
    out = {}
    for name, base in TABLES.items():
        src = os.path.join(base, name, "_delta_log")
        if not os.path.isdir(src):
            print("skip", name)
            continue
        dst = os.path.join(HERE, "tables", name, "_delta_log")
        shutil.rmtree(os.path.dirname(dst), ignore_errors=True)
        shutil.copytree(src, dst, ignore=shutil.ignore_patterns("*.crc", ".*.crc"))
        res = {}
        for bs in (2, 1024):
            for stats in (False, True):
                r = ref.replay(os.path.dirname(dst), json_batch_size=bs, with_stats=stats)
                res["%d-%d" % (bs, int(stats))] = {"version": r.version, "counters": list(r.counters.as_tuple()),
                                                   "rows": canon_json(r.scan_files())}
        out[name] = res
        print(name, res["1024-0"]["version"], len(res["1024-0"]["rows"]), res["1024-0"]["counters"])
    with open(os.path.join(HERE, "expected.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


def main():
    if not os.path.isdir(GOLD):
        raise SystemExit(__doc__)
    what = sys.argv[2:] or ["tables", "oracle", "schema"]
    for w in what:
        {"tables": table_fixtures, "oracle": oracle_fixtures, "schema": schema_fixtures}[w]()


if __name__ == "__main__":
    main()
