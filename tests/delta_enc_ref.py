"""A small NumPy / plain-Python restatement of three Parquet value decoders, for flat (non-nested)
nullable columns of uncompressed files: DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and
BYTE_STREAM_SPLIT, with the DELTA_BINARY_PACKED walk under the first two. Written from the format
description (parquet-format Encodings.md), not from any reader; tests/test_delta_encodings_host.py
holds it to pyarrow on the files the GPU tests write, so those tests do not rest on pyarrow alone.

read_column(path, leaf) -> (values, encodings): one entry per row (bytes, or the value's bit pattern
as an int for FLOAT / DOUBLE, or None), and the set of data-page encodings met.
"""
import numpy as np
import pyarrow.parquet as pq

PLAIN, DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY, BYTE_STREAM_SPLIT = 0, 5, 6, 7, 9
DATA_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 2, 3


# ---- thrift compact protocol: just enough for PageHeader -------------------------------------------
def _uvarint(buf, at):
    v = s = 0
    while True:
        b = buf[at]
        at += 1
        v |= (b & 0x7F) << s
        if not b & 0x80:
            return v, at
        s += 7


def _zigzag(v):
    return (v >> 1) ^ -(v & 1)


def _value(buf, at, typ):
    if typ in (1, 2):                              # bool in the type nibble
        return typ == 1, at
    if typ == 3:
        return buf[at], at + 1
    if typ in (4, 5, 6):
        v, at = _uvarint(buf, at)
        return _zigzag(v), at
    if typ == 7:
        return None, at + 8
    if typ == 8:
        n, at = _uvarint(buf, at)
        return bytes(buf[at:at + n]), at + n
    if typ in (9, 10):                             # list / set
        h = buf[at]
        at += 1
        n, et = h >> 4, h & 15
        if n == 15:
            n, at = _uvarint(buf, at)
        out = []
        for _ in range(n):
            if et in (1, 2):
                out.append(buf[at] == 1)
                at += 1
            else:
                v, at = _value(buf, at, et)
                out.append(v)
        return out, at
    if typ == 12:
        return _struct(buf, at)
    raise ValueError("thrift type %d" % typ)


def _struct(buf, at):
    out, fid = {}, 0
    while True:
        h = buf[at]
        at += 1
        if h == 0:
            return out, at
        if h >> 4:
            fid += h >> 4
        else:
            v, at = _uvarint(buf, at)
            fid = _zigzag(v)
        out[fid], at = _value(buf, at, h & 15)


# ---- level and value decoders ------------------------------------------------------------------------
def hybrid(buf, at, end, bw, n):
    """n values of an RLE / bit-packed hybrid stream."""
    out = []
    nb = (bw + 7) // 8
    while len(out) < n and at < end:
        h, at = _uvarint(buf, at)
        if h & 1:
            cnt = (h >> 1) * 8
            bits = np.unpackbits(np.frombuffer(buf[at:at + (h >> 1) * bw], np.uint8), bitorder="little")
            bits = bits[:len(bits) // bw * bw].reshape(-1, bw)
            out += (bits.astype(np.int64) << np.arange(bw)).sum(axis=1).tolist()[:cnt]
            at += (h >> 1) * bw
        else:
            out += [int.from_bytes(buf[at:at + nb], "little")] * (h >> 1)
            at += nb
    return out[:n]


def delta_binary_packed(buf, at):
    """One DELTA_BINARY_PACKED stream starting at `at`: (values, first byte behind the stream)."""
    block, at = _uvarint(buf, at)
    minis, at = _uvarint(buf, at)
    total, at = _uvarint(buf, at)
    first, at = _uvarint(buf, at)
    out = [_zigzag(first)]
    per = block // minis if minis else 0
    assert minis and block % minis == 0 and per % 32 == 0
    left = total - 1
    while left > 0:
        md, at = _uvarint(buf, at)
        md = _zigzag(md)
        widths = list(buf[at:at + minis])          # every miniblock's width byte is present ...
        at += minis
        for w in widths:
            if left <= 0:                          # ... but an unneeded miniblock has no data, and its
                break                              # width byte means nothing
            nbytes = per * w // 8                  # the last needed miniblock is whole (padded)
            if w:
                bits = np.unpackbits(np.frombuffer(buf[at:at + nbytes], np.uint8), bitorder="little").reshape(per, w)
                vals = [sum(int(b) << k for k, b in enumerate(row)) for row in bits[:min(per, left)]]
            else:
                vals = [0] * min(per, left)
            at += nbytes
            for d in vals:
                out.append((out[-1] + md + d + (1 << 63)) % (1 << 64) - (1 << 63))   # wrapping 64-bit
            left -= len(vals)
    return out[:total], at


def delta_length_byte_array(buf, at, end):
    lens, at = delta_binary_packed(buf, at)
    out = []
    for ln in lens:
        assert ln >= 0 and at + ln <= end
        out.append(bytes(buf[at:at + ln]))
        at += ln
    return out, at


def delta_byte_array(buf, at, end):
    prefixes, at = delta_binary_packed(buf, at)
    suffixes, at = delta_length_byte_array(buf, at, end)
    assert len(prefixes) == len(suffixes)
    out, prev = [], b""
    for p, s in zip(prefixes, suffixes):
        assert 0 <= p <= len(prev)
        prev = prev[:p] + s
        out.append(prev)
    return out


def byte_stream_split(buf, at, n, width):
    a = np.frombuffer(buf[at:at + n * width], np.uint8).reshape(width, n)     # stream k = byte k of every value
    return np.ascontiguousarray(a.T).view({4: "<u4", 8: "<u8"}[width]).ravel().tolist()


def plain(buf, at, n, phys, width):
    if phys == "BYTE_ARRAY":
        out = []
        for _ in range(n):
            ln = int.from_bytes(buf[at:at + 4], "little")
            out.append(bytes(buf[at + 4:at + 4 + ln]))
            at += 4 + ln
        return out
    return np.frombuffer(buf[at:at + n * width], {4: "<u4", 8: "<u8"}[width]).tolist()


# ---- a flat column of an uncompressed file -----------------------------------------------------------
def read_column(path, leaf):
    pf = pq.ParquetFile(path)
    md = pf.metadata
    idx = next(i for i in range(md.num_columns) if md.schema.column(i).path == leaf)
    sc = md.schema.column(idx)
    assert sc.max_repetition_level == 0 and sc.max_definition_level <= 1, "flat columns only"
    width = {"FLOAT": 4, "DOUBLE": 8, "INT32": 4, "INT64": 8}.get(sc.physical_type, 0)
    with open(path, "rb") as f:
        data = f.read()
    rows, encodings = [], set()
    for g in range(md.num_row_groups):
        c = md.row_group(g).column(idx)
        assert c.compression == "UNCOMPRESSED"
        at = c.dictionary_page_offset if c.has_dictionary_page else c.data_page_offset
        end = at + c.total_compressed_size
        while at < end:
            h, body = _struct(data, at)
            size = h[3]
            at = body + size
            if h[1] == DICTIONARY_PAGE:
                continue
            if h[1] == DATA_PAGE:
                n, enc, p = h[5][1], h[5][2], body
                defs = [1] * n
                if sc.max_definition_level:
                    ln = int.from_bytes(data[p:p + 4], "little")
                    defs = hybrid(data, p + 4, p + 4 + ln, 1, n)
                    p += 4 + ln
            else:
                assert h[1] == DATA_PAGE_V2
                n, enc = h[8][1], h[8][4]
                p = body + h[8][6]
                defs = hybrid(data, p, p + h[8][5], 1, n) if sc.max_definition_level else [1] * n
                p += h[8][5]
            encodings.add(enc)
            nv = sum(defs)
            page_end = body + size
            if nv == 0:
                vals = []
            elif enc == DELTA_LENGTH_BYTE_ARRAY:
                vals, _ = delta_length_byte_array(data, p, page_end)
            elif enc == DELTA_BYTE_ARRAY:
                vals = delta_byte_array(data, p, page_end)
            elif enc == BYTE_STREAM_SPLIT:
                vals = byte_stream_split(data, p, nv, width)
            elif enc == PLAIN:
                vals = plain(data, p, nv, sc.physical_type, width)
            else:
                raise ValueError("encoding %d" % enc)
            assert len(vals) == nv, (len(vals), nv)
            it = iter(vals)
            rows += [next(it) if d else None for d in defs]
    return rows, encodings
