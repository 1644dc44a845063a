"""CPU, no device. (1) The NumPy restatement of the DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and
BYTE_STREAM_SPLIT decoders (tests/delta_enc_ref.py: a DBP walk with the last-block rule, the prefix /
suffix reconstruction, the byte-stream transpose) is held to pyarrow on the very files the GPU tests
of tests/test_delta_encodings.py write (their table builders are run here with the twin check
replaced), uncompressed, both page versions; floats by their bits. So the GPU tests' expectations
rest on two independent readers. The restatement reads flat columns; the nullable leaf inside a
struct is checked against pyarrow and the PLAIN twin's oracle read only. (2) synth's optional
per-leaf column_encoding (spec.extra)."""
import pyarrow.parquet as pq
import pytest

from delta_amd import synth
from tests import delta_enc_ref as R
from tests import test_delta_encodings as T

ENC_ID = {T.DLBA: R.DELTA_LENGTH_BYTE_ARRAY, T.DBA: R.DELTA_BYTE_ARRAY, T.BSS: R.BYTE_STREAM_SPLIT}


@pytest.fixture
def host_check(monkeypatch):
    """Replaces the GPU twin check: the restatement over the encoded file (and over the PLAIN twin)
    must give what pyarrow reads back."""
    seen = []

    def check(engine, table, plain, enc):
        back = pq.read_table(enc)
        want_enc = {}
        md = pq.ParquetFile(enc).metadata
        for i in range(md.num_columns):
            c = md.row_group(0).column(i)
            want_enc[c.path_in_schema] = [ENC_ID[e] for e in c.encodings if e in ENC_ID]
        for leaf in T._leaves(table.schema):
            if "." in leaf:
                continue
            want = T._arrow_pylist(T._arrow_leaf(back, leaf))
            got, encs = R.read_column(enc, leaf)
            assert want_enc[leaf] and set(want_enc[leaf]) <= encs, (leaf, encs)
            assert got == want, leaf
            assert R.read_column(plain, leaf)[0] == want, leaf
            seen.append(leaf)
    monkeypatch.setattr(T, "_check_twins", check)
    return seen


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("encoding", [T.DLBA, T.DBA])
def test_restatement_value_counts(tmp_path, host_check, encoding, version):
    T.test_value_counts_per_page(tmp_path, None, encoding, version, "none")
    assert host_check == ["s", "b"]


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("encoding", [T.DLBA, T.DBA])
@pytest.mark.parametrize("kind", ["equal", "empty", "wide"])
def test_restatement_lengths(tmp_path, host_check, kind, encoding, version):
    T.test_lengths(tmp_path, None, kind, encoding, version, "none")
    assert host_check == ["s", "n"]


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_restatement_chains(tmp_path, host_check, version):
    T.test_delta_byte_array_chains(tmp_path, None, version, "none")
    assert host_check == ["p", "raw"]


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_restatement_byte_stream_split(tmp_path, host_check, version):
    T.test_byte_stream_split(tmp_path, None, version, "none")
    assert host_check == ["f", "d", "dense"]


def test_dbp_last_block_rule():
    """150 values: the second block needs one of its four miniblocks; the three unneeded width bytes
    hold garbage and have no data. Hand-built stream, first value 7, every delta 1."""
    buf = bytearray([0x80, 0x01, 0x04, 0x96, 0x01, 14])         # block 128, 4 miniblocks, total, first = zigzag(7)
    buf += bytes([2]) + bytes([0, 0, 0, 0])                      # block 1: min delta 1, widths 0
    buf += bytes([2]) + bytes([0, 0xEE, 0x77, 0x3F])             # block 2: 21 deltas: only miniblock 0 is needed
    buf += b"TAIL"
    vals, end = R.delta_binary_packed(bytes(buf), 0)
    assert vals == list(range(7, 157)) and bytes(buf[end:]) == b"TAIL"


def _encodings(path):
    md = pq.ParquetFile(path).metadata
    return {md.row_group(0).column(i).path_in_schema: set(md.row_group(0).column(i).encodings) for i in range(md.num_columns)}


def test_synth_column_encoding(tmp_path):
    enc = {"add.path": "DELTA_BYTE_ARRAY", "add.stats": "DELTA_LENGTH_BYTE_ARRAY", "no.such.leaf": "DELTA_BYTE_ARRAY",
           "add.partitionValues.key_value.key": "DELTA_BYTE_ARRAY"}
    a = synth.write_table(str(tmp_path / "a"), synth.TableSpec(n_adds=500, n_commits=2, with_stats=True))
    b = synth.write_table(str(tmp_path / "b"), synth.TableSpec(n_adds=500, n_commits=2, with_stats=True,
                                                               extra={"column_encoding": enc}))
    used = _encodings(b["checkpoint_files"][0])
    assert "DELTA_BYTE_ARRAY" in used["add.path"] and "DELTA_LENGTH_BYTE_ARRAY" in used["add.stats"]
    assert "DELTA_BYTE_ARRAY" in used["add.partitionValues.key_value.key"]
    assert "DELTA_BYTE_ARRAY" not in _encodings(a["checkpoint_files"][0])["add.path"]
    assert pq.read_table(b["checkpoint_files"][0]).equals(pq.read_table(a["checkpoint_files"][0]))
