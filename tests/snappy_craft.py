"""Hand-built raw snappy streams for the decoder tests (tests/test_snappy_craft_host.py on the CPU,
tests/test_snappy_craft.py on the GPU), written from the format description (snappy's
format_description.txt), not from any encoder:

  lit / copy / build   a stream from an explicit op list: the builder writes exactly what it is told
                       (non-minimal length forms, 4-byte-offset copies, offset 0, a forced preamble)
  decode               the oracle: one tag at a time, byte by byte; returns the bytes or raises ValueError
  inspect / walk       the tags of a stream as (kind, form, comp_off, out_off, length, offset)
  write_parquet        one row group of required INT64 / BYTE_ARRAY columns, PLAIN, v1 data pages whose
                       compressed bodies (and declared uncompressed sizes) are given
  valid_cases / malformed_cases   the corpus, positions derived from the decoder's own constants

Every stream every other test decodes was written by Google's encoder, which compresses each 64 KiB of
input on its own: no 4-byte-offset copy, no 3- or 4-byte literal length, no non-minimal form, no tag
across a 64 KiB output boundary, no copy reaching back across one. All of these are legal, and the
fragment-parallel decoder (delta_amd/csrc/dk_kernels.hip, k_snap_*) relies on guards that send such
pages to k_snappy_serial; the corpus reaches each of them. Importing this module needs no GPU and no
pyarrow.
"""
import collections
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(name):
    """An integer constant of the decoder, read from its source (so positions move with it)."""
    for f in ("dk_device.h", "dk_kernels.hip"):
        with open(os.path.join(ROOT, "delta_amd", "csrc", f)) as fh:
            m = re.search(r"(?:#define\s+%s\s+|constexpr\s+int\s+%s\s*=\s*)(\d+)" % (name, name), fh.read())
        if m:
            return int(m.group(1))
    raise KeyError(name)


SEG = _const("DK_SNAP_SEG_BYTES")        # compressed bytes per speculative walker
FRAG = _const("SNAP_FRAG")               # output bytes per k_snap_frag wave
STEP = _const("DK_SF_WALK_STEP")         # stream bytes per staged walk round
REC = _const("DK_SNAP_REC")              # tag positions a walker records
BUDGET = _const("DK_SF_LINK_BUDGET")     # k_snap_link tags before the staged relink
RING = _const("DK_SF_RING")              # k_snap_frag's LDS output ring
FLUSH = _const("SNAP_FLUSH")             # ring -> HBM granule
FARQ = _const("SF_FARQ_MAX")             # far copies up to this long are loaded early
BOUT = _const("DK_SF_BOUT")              # a batch stops collecting tags at this many output bytes
BTAGS = 64                               # tags per batch: one per lane of a wave


# ---- stream builder --------------------------------------------------------------------------------
def varint(n, nbytes=None):
    """Little-endian base-128; nbytes forces the byte count (non-minimal when larger than needed)."""
    out = bytearray()
    while True:
        out.append(n & 0x7F)
        n >>= 7
        if not n:
            break
    if nbytes is not None:
        if len(out) > nbytes:
            raise ValueError("%d bytes cannot hold the value" % nbytes)
        out += bytes(nbytes - len(out))
    for i in range(len(out) - 1):
        out[i] |= 0x80
    return bytes(out)


def lit(data, form=None):
    """A literal. form: None = the shortest encoding, 0 = length in the tag byte, 1..4 = that many
    length bytes (non-minimal allowed)."""
    return ("lit", bytes(data), form)


def copy(off, length, kind):
    """A copy with a 1-, 2- or 4-byte offset (kind 1, 2, 3)."""
    return ("copy", off, length, kind)


def encode_op(op):
    if op[0] == "lit":
        _, data, form = op
        n = len(data) - 1
        if n < 0:
            raise ValueError("an empty literal has no encoding")
        if form is None:
            form = 0 if n < 60 else (n.bit_length() + 7) // 8
        if form == 0:
            if n >= 60:
                raise ValueError("inline literal length %d" % (n + 1))
            return bytes([n << 2]) + data
        if form not in (1, 2, 3, 4) or n >> (8 * form):
            raise ValueError("literal length %d in %r bytes" % (n + 1, form))
        return bytes([(59 + form) << 2]) + n.to_bytes(form, "little") + data
    _, off, length, kind = op
    if kind == 1:
        if not (4 <= length <= 11 and 0 <= off < 2048):
            raise ValueError("copy-1 cannot express (%d, %d)" % (off, length))
        return bytes([1 | (length - 4) << 2 | (off >> 8) << 5, off & 0xFF])
    if kind in (2, 3):
        if not (1 <= length <= 64 and 0 <= off < 1 << (16 if kind == 2 else 32)):
            raise ValueError("copy-%d cannot express (%d, %d)" % (kind, off, length))
        return bytes([kind | (length - 1) << 2]) + off.to_bytes(2 if kind == 2 else 4, "little")
    raise ValueError("copy kind %r" % (kind,))


def build(ops, declared, preamble_bytes=None):
    """preamble (varint of `declared`) + the ops, exactly as given."""
    return varint(declared, preamble_bytes) + b"".join(encode_op(o) for o in ops)


# ---- reference decoder and tag walker -------------------------------------------------------------
Tag = collections.namedtuple("Tag", "kind form comp_off out_off length offset")


def preamble(buf):
    """(declared length, first tag's offset). As snappy reads it: at most 5 bytes, 32 bits."""
    v = 0
    for i in range(5):
        if i >= len(buf):
            raise ValueError("preamble cut off")
        b = buf[i]
        if i == 4 and b >= 16:
            raise ValueError("preamble longer than 32 bits")
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return v, i + 1
    raise ValueError("unreachable")


def walk(buf, p, end=None, out_off=0):
    """The tag chain from stream offset p to the first tag at or past `end` (default: the stream's
    end): (tags, status), status "end" or "dead" (a tag or its literal runs past the stream end), the
    way a speculative walker parses. Copies are not resolved."""
    n = len(buf)
    end = n if end is None else min(end, n)
    tags, o = [], out_off
    while p < end:
        t = buf[p]
        kind = t & 3
        if kind == 0:
            form, ln = 0, (t >> 2) + 1
            if ln > 60:
                form = ln - 60
                if p + 1 + form > n:
                    return tags, "dead"
                ln = int.from_bytes(buf[p + 1:p + 1 + form], "little") + 1
            if p + 1 + form + ln > n:
                return tags, "dead"
            tags.append(Tag(0, form, p, o, ln, None))
            p += 1 + form + ln
        else:
            hdr = (2, 3, 5)[kind - 1]
            if p + hdr > n:
                return tags, "dead"
            if kind == 1:
                ln, off = ((t >> 2) & 7) + 4, (t >> 5) << 8 | buf[p + 1]
            else:
                ln, off = (t >> 2) + 1, int.from_bytes(buf[p + 1:p + hdr], "little")
            tags.append(Tag(kind, None, p, o, ln, off))
            p += hdr
        o += ln
    return tags, "end"


def inspect(stream):
    """The tags of a well-formed stream; ValueError otherwise (copies are not resolved)."""
    stream = bytes(stream)
    _, p = preamble(stream)
    tags, status = walk(stream, p)
    if status != "end":
        raise ValueError("a tag runs past the stream end")
    return tags


def decode(stream):
    """The oracle. Returns the uncompressed bytes or raises ValueError."""
    stream = bytes(stream)
    want, p = preamble(stream)
    tags, status = walk(stream, p)
    out = bytearray()
    for t in tags:
        if len(out) + t.length > want:
            raise ValueError("more output than declared")
        if t.kind == 0:
            at = t.comp_off + 1 + t.form
            out += stream[at:at + t.length]
        else:
            if t.offset == 0 or t.offset > len(out):
                raise ValueError("copy offset %d at output %d" % (t.offset, len(out)))
            for _ in range(t.length):               # byte by byte: the source may overlap the copy
                out.append(out[-t.offset])
    if status != "end":
        raise ValueError("a tag runs past the stream end")
    if len(out) != want:
        raise ValueError("%d bytes, %d declared" % (len(out), want))
    return bytes(out)


# ---- minimal Parquet writer --------------------------------------------------------------------------
class _Thrift:
    """Thrift compact protocol, writing side (the reading side: tests/delta_enc_ref.py)."""

    def __init__(self):
        self.b = bytearray()
        self.last = [0]

    def _uv(self, v):
        self.b += varint(v)

    def _zz(self, v):
        self._uv((v << 1) ^ (v >> 63))

    def _field(self, fid, typ):
        d = fid - self.last[-1]
        if 0 < d <= 15:
            self.b.append(d << 4 | typ)
        else:
            self.b.append(typ)
            self._zz(fid)
        self.last[-1] = fid

    def i32(self, fid, v):
        self._field(fid, 5)
        self._zz(v)

    def i64(self, fid, v):
        self._field(fid, 6)
        self._zz(v)

    def binary(self, fid, s):
        self._field(fid, 8)
        self._uv(len(s))
        self.b += s

    def begin(self, fid=None):
        """A struct: a field of the current one, or (fid None) a list element."""
        if fid is not None:
            self._field(fid, 12)
        self.last.append(0)

    def end(self):
        self.b.append(0)
        self.last.pop()

    def list(self, fid, etype, n):
        self._field(fid, 9)
        if n < 15:
            self.b.append(n << 4 | etype)
        else:
            self.b.append(0xF0 | etype)
            self._uv(n)


INT64, BYTE_ARRAY = 2, 6
Page = collections.namedtuple("Page", "body usize num_values")   # compressed body, declared size, values


def _page_header(pg):
    t = _Thrift()
    t.i32(1, 0)                      # DATA_PAGE
    t.i32(2, pg.usize)
    t.i32(3, len(pg.body))
    t.begin(5)
    t.i32(1, pg.num_values)
    t.i32(2, 0)                      # PLAIN
    t.i32(3, 3)                      # definition / repetition levels: RLE (none: the column is required)
    t.i32(4, 3)
    t.end()
    t.end()
    return bytes(t.b)


def write_parquet(path, columns):
    """columns: [(name, INT64 | BYTE_ARRAY, [Page, ...])]. One row group, codec SNAPPY. Every chunk's
    first page body starts at a file offset that is a multiple of 64 (the padding lies before the
    chunk), so the decoder's windows over the stream are aligned the same way every time."""
    f = bytearray(b"PAR1")
    chunks = []
    for name, phys, pages in columns:
        start, unc = None, 0
        for pg in pages:
            h = _page_header(pg)
            if start is None:                       # only the chunk's first page may be preceded by padding
                f += bytes(-(len(f) + len(h)) % 64)
                start = len(f)
            f += h + pg.body
            unc += len(h) + pg.usize
        chunks.append((name, phys, start, len(f) - start, unc, sum(pg.num_values for pg in pages)))
    rows = chunks[0][5]
    assert all(c[5] == rows for c in chunks)
    t = _Thrift()
    t.i32(1, 1)
    t.list(2, 12, 1 + len(chunks))
    t.begin()
    t.binary(4, b"schema")
    t.i32(5, len(chunks))
    t.end()
    for name, phys, *_ in chunks:
        t.begin()
        t.i32(1, phys)
        t.i32(3, 0)                  # REQUIRED
        t.binary(4, name.encode())
        t.end()
    t.i64(3, rows)
    t.list(4, 12, 1)
    t.begin()
    t.list(1, 12, len(chunks))
    for name, phys, start, clen, unc, nv in chunks:
        t.begin()
        t.i64(2, start)
        t.begin(3)
        t.i32(1, phys)
        t.list(2, 5, 2)
        t._zz(0)
        t._zz(3)
        t.list(3, 8, 1)
        t._uv(len(name))
        t.b += name.encode()
        t.i32(4, 1)                  # SNAPPY
        t.i64(5, nv)
        t.i64(6, unc)
        t.i64(7, clen)
        t.i64(9, start)
        t.end()
        t.end()
    t.i64(2, sum(c[4] for c in chunks))
    t.i64(3, rows)
    t.end()
    t.binary(6, b"snappy_craft")
    t.end()
    f += t.b + struct.pack("<I", len(t.b)) + b"PAR1"
    with open(path, "wb") as fh:
        fh.write(f)


def plain_byte_array(values):
    return b"".join(struct.pack("<I", len(v)) + v for v in values)


# ---- corpus ------------------------------------------------------------------------------------------------
class _B:
    """Ops with the running output and compressed position, so a case can place a tag at an exact
    stream or output offset. pre: the preamble's byte count (fixed up front: positions depend on it)."""

    def __init__(self, seed, pre=3):
        self.ops, self.out, self.pre, self.c = [], bytearray(), pre, pre
        self.rng = np.random.default_rng(seed)

    def rnd(self, n):
        return self.rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    def add(self, op):
        self.ops.append(op)
        self.c += len(encode_op(op))
        if op[0] == "lit":
            self.out += op[1]
        else:
            assert 0 < op[1] <= len(self.out), op
            for _ in range(op[2]):
                self.out.append(self.out[-op[1]])
        return self

    def lit(self, data, form=None):
        return self.add(lit(self.rnd(data) if isinstance(data, int) else data, form))

    def copy(self, off, length, kind):
        return self.add(copy(off, length, kind))

    def out_to(self, o):
        """Literals up to output offset o, none of them across a fragment boundary."""
        while len(self.out) < o:
            self.lit(min(o - len(self.out), FRAG - len(self.out) % FRAG, 5000))
        assert len(self.out) == o
        return self

    def room(self, n, back=0):
        """The next n output bytes stay in one fragment, at least `back` bytes after its start."""
        if len(self.out) % FRAG + n > FRAG:
            self.out_to((len(self.out) // FRAG + 1) * FRAG)
        if len(self.out) % FRAG < back:
            self.out_to(len(self.out) - len(self.out) % FRAG + back)
        return self

    def batch_break(self):
        """A literal over 64 bytes runs as a batch of its own: the next tag starts a batch."""
        return self.room(65).lit(65)

    def comp_to(self, c, data=None):
        """One literal that ends at stream offset c (the next tag starts there)."""
        gap = c - self.c
        for form, cap in ((0, 60), (1, 1 << 8), (2, 1 << 16), (3, 1 << 24)):
            n = gap - 1 - form
            if 1 <= n <= cap:
                self.room(n)
                assert self.c + 1 + form + n == c       # (room may not have moved the position)
                return self.lit(self.rnd(n) if data is None else data(n), form)
        raise ValueError("cannot place a literal of %d stream bytes" % gap)

    def done(self, end_copy=False):
        """Pad the output to whole INT64 values; end_copy: the stream's last tag is a copy."""
        pad = -len(self.out) % 8
        if end_copy:
            pad = (-len(self.out) - 5) % 8
        if pad:
            self.room(pad).lit(pad)
        if end_copy:
            self.room(5, 64).copy(33, 5, 3)
        s = build(self.ops, len(self.out), self.pre)
        assert len(s) == self.c and len(self.out) % 8 == 0
        return s, bytes(self.out)


Case = collections.namedtuple("Case", "name stream out serial check")
# serial: pages k_snappy_serial decodes in the two fragment modes (page mode: 0). check(tags, stream):
# the feature the case is named for is there.


def _frag_of(o):
    return o // FRAG * FRAG


def _straddles(t):
    return t.out_off // FRAG != (t.out_off + t.length - 1) // FRAG


def _reaches_back(t):
    return t.kind != 0 and t.out_off - t.offset < _frag_of(t.out_off)


def _fast(tags):
    """Nothing that sends a page to the serial path."""
    return not any(_straddles(t) or _reaches_back(t) for t in tags)


def _copy4_near():
    b = _B(1).lit(3000)
    for i in range(420):
        off = (1, 2047, 2, 63, 64)[i] if i < 5 else 1 + (i * 37) % 2047
        n = (64, 1, 64, 1, 33)[i] if i < 5 else 1 + i % 64
        b.room(n, off).copy(off, n, 3)
        if i % 3 == 0:
            b.room(70).lit(1 + (i * 11) % 70)
    s, o = b.done()
    return Case("copy4_near", s, o, 0, lambda t, s: _fast(t) and
                {x.offset for x in t if x.kind == 3} >= {1, 2047} and
                {x.length for x in t if x.kind == 3} == set(range(1, 65)) and
                all(x.offset < SEG for x in t if x.kind == 3))


def _copy4_far():
    b = _B(2).out_to(FRAG + 900)
    for off in (65536, 65537, FRAG + 900, 66000):    # into fragment 0, to its very first byte too
        b.copy(off, 8, 3).lit(8).copy(off + 16, 64, 3)
    b.out_to(2 * FRAG + 300).copy(2 * FRAG + 300, 9, 3).copy(2 * FRAG - 100, 40, 3).lit(100)
    s, o = b.done()
    return Case("copy4_far", s, o, 1, lambda t, s: any(x.kind == 3 and x.offset > 65535 and _reaches_back(x) for x in t)
                and not any(_straddles(x) for x in t))


def _lit_forms():
    b = _B(3)
    for form in (0, 1, 2, 3, 4):
        for n in (1, 5, 59, 60, 61, 64, 65, 255, 256, 257, 300, 4000):
            if n <= 60 or (form and n <= 1 << 8 * form):
                b.room(n).lit(n, form)
                b.room(8, 8).copy(7, 6, 1)
    b.out_to(FRAG - 3000)
    b.lit(3000, 3)                                   # ends exactly on the fragment boundary
    assert len(b.out) == FRAG
    b.copy(70, 20, 2).lit(65536, 2).copy(5, 64, 2)   # the longest 2-byte form, across fragments 1 and 2
    b.lit(FRAG + 4464, 3)                            # longer than a fragment
    s, o = b.done()
    forms = {(0, 5), (1, 5), (2, 5), (3, 5), (4, 5), (1, 60), (0, 60), (4, 300), (3, 4000), (2, 65536), (3, FRAG + 4464)}
    return Case("lit_forms", s, o, 1, lambda t, s: {(x.form, x.length) for x in t if x.kind == 0} >= forms and
                any(x.kind == 0 and x.out_off + x.length == FRAG for x in t) and
                any(x.kind == 0 and x.length > FRAG and _straddles(x) for x in t))


def _lit_inside():
    """lit_forms without the literal that crosses fragments: the forms on the fragment path."""
    b = _B(4)
    for form in (0, 1, 2, 3, 4):
        for n in (1, 5, 59, 60, 61, 64, 65, 255, 256, 257, 300, 4000):
            if n <= 60 or (form and n <= 1 << 8 * form):
                b.room(n).lit(n, form)
                b.room(8, 8).copy(7, 6, 1)
    b.out_to(FRAG - 3000)
    b.lit(3000, 3)
    b.lit(70).copy(70, 20, 2).lit(FRAG - 90, 4).lit(5).copy(5, 64, 2).lit(300, 4)
    s, o = b.done()
    forms = {(0, 5), (1, 5), (2, 5), (3, 5), (4, 5), (1, 60), (0, 60), (4, 300), (3, 4000), (4, FRAG - 90)}
    return Case("lit_inside", s, o, 0, lambda t, s: _fast(t) and {(x.form, x.length) for x in t if x.kind == 0} >= forms
                and sum(x.out_off + x.length in (FRAG, 2 * FRAG) for x in t) == 2)


def _straddle_copy():
    b = _B(5).out_to(FRAG - 1).copy(200, 10, 2).lit(500)     # the boundary 1 byte into the tag
    b.out_to(2 * FRAG - 11).copy(3, 12, 2).lit(500)         # ... and len - 1 bytes into it
    s, o = b.done()
    return Case("straddle_copy", s, o, 1, lambda t, s: sorted(FRAG * (x.out_off // FRAG + 1) - x.out_off
                for x in t if x.kind and _straddles(x)) == [1, 11] and not any(_reaches_back(x) for x in t))


def _back(across):
    b = _B(6 + across)
    for f in (1, 2):
        for d in (1, 100, 700, 5000, 65000):
            # the copy's output position is d bytes into fragment f; its offset is d and d - 1
            # (the source starts on and just after the fragment's first byte) or d + 1 (one byte before)
            for rel in ((1,) if across else (0, -1)):
                b.out_to(f * FRAG + d).copy(d + rel, 24, 2)
                d += 30
    if across:
        b.out_to(3 * FRAG + 40000).copy(65535, 64, 2)
    b.lit(40)
    s, o = b.done()
    rel = {x.offset - (x.out_off - _frag_of(x.out_off)) for x in t_copies(s)}
    assert rel == ({1, 65535 - 40000} if across else {0, -1}), rel
    if across:
        return Case("back_across", s, o, 1, lambda t, s: sum(_reaches_back(x) for x in t) == 11 and
                    any(x.out_off - x.offset == _frag_of(x.out_off) - 1 for x in t if x.kind == 2) and
                    not any(_straddles(x) for x in t))
    return Case("back_inside", s, o, 0, lambda t, s: _fast(t) and
                any(x.kind == 2 and x.out_off - x.offset == _frag_of(x.out_off) >= FRAG for x in t))


def t_copies(stream):
    return [t for t in inspect(stream) if t.kind]


def _periods(dep):
    """Every overlapping (offset, length): the source is one literal of the copy's batch (resolved to
    a window read with a period, small_mod_f), or -- dep -- two literals (a source straddling tags
    stays dependent: small_mod in the ordered stage)."""
    b = _B(8 + dep).lit(64)
    for off in range(1, 64):
        for n in range(1, 65):
            b.room(off + n + 6)
            if dep and off == 1:
                b.lit(1).copy(1, 5, 2)               # a one-byte source cannot straddle: inside a periodic copy
            elif dep:
                b.lit(off - off // 2).lit(off // 2)
            else:
                b.lit(off)
            b.copy(off, n, 1 if 4 <= n <= 11 else 2)
    s, o = b.done()

    def check(t, s):
        pairs = set()
        for i, x in enumerate(t):
            if x.kind and x.offset < 64:
                src = t[i - 1]
                one = src.kind == 0 and src.length == x.offset
                if one != bool(dep):
                    pairs.add((x.offset, x.length))
        return _fast(t) and pairs >= {(a, n) for a in range(1, 64) for n in range(1, 65)} and \
            {x.kind for x in t} == {0, 1, 2}
    return Case("periods_dep" if dep else "periods", s, o, 0, check)


def _short_copy2():
    b = _B(10).lit(5000)
    for i in range(300):
        n = 1 + i % 3
        off = (1, 2, 3, 4, 63, 64, 65, 2047, 2048, 4095, 4096, 4097)[i % 12]
        b.room(n, off).copy(off, n, 2)
        if i % 5 == 0:
            b.room(9).lit(1 + i % 9)
    s, o = b.done()
    return Case("short_copy2", s, o, 0, lambda t, s: _fast(t) and
                {x.length for x in t if x.kind == 2} == {1, 2, 3})


def _chains():
    b = _B(11)
    for depth in range(1, 9):                        # copy k's source is copy k - 1's output, all in one batch:
        b.batch_break().room(16 * (depth + 1))       # 6 rounds of pointer jumping, then `stuck`
        b.lit(16)
        for _ in range(depth):
            b.copy(16, 16, 2)
    for depth in range(1, 9):                        # the same with a shift, so every hop lands mid-tag
        b.batch_break().room(24 + 12 * depth)
        b.lit(24)
        for _ in range(depth):
            b.copy(14, 12, 2)
    b.batch_break().room(24).lit(8).copy(8, 8, 1).copy(12, 8, 1)      # a source across a literal / copy pair
    b.batch_break().room(24).lit(6).lit(6).copy(9, 6, 1)              # ... and across two literals
    b.batch_break().room(BTAGS)
    for _ in range(BTAGS):
        b.lit(1)                                     # a batch of 64 one-byte tags
    b.batch_break().room(BTAGS)
    for i in range(BTAGS):
        b.copy(70 + i % 5, 1, 2)
    b.batch_break().room(BTAGS)
    for i in range(BTAGS):
        b.copy(1 + i % 2, 1, 2)                      # each one's source is the tag before it
    s, o = b.done()

    def check(t, s):
        runs = best = 0
        for x in t:
            runs = runs + 1 if x.kind == 2 and (x.offset, x.length) == (16, 16) else 0
            best = max(best, runs)
        ones = "".join("1" if x.length == 1 else "0" for x in t)
        return _fast(t) and best == 8 and "1" * BTAGS in ones
    return Case("chains", s, o, 0, check)


def _ring_edge():
    b = _B(12).lit(3 * RING)
    lens = (FARQ, FARQ + 1, 20, 1)
    i = 0
    for off in list(range(RING - BOUT - 72, RING + 10)) + list(range(RING + 10, RING + FLUSH + 16, 7)):
        b.room(20, off).copy(off, lens[i % 4], 2)    # every distance about the ring's reach, so whatever the
        i += 1                                       # batch's first output byte, RING - 1 / RING / RING + 1 from
        if i % 9 == 0:                               # it occur; far sources at all four alignments, 8 and 9 long
            b.room(30).lit(1 + i % 30)
    # (the granule flushed last lies within 2 * FLUSH <= RING of the cursor, so a source in it is a ring
    # read, never a far one: the nearest far sources are those the ring has just dropped)
    assert 2 * FLUSH <= RING
    b.room(100 + 2 * FLUSH, 3 * RING).lit(FLUSH + 7, 2)               # a long literal flushes as it goes:
    for k in range(8):                                                # far sources just behind it
        b.copy(RING + 1 + 3 * k, FARQ + (k & 1), 2)
    s, o = b.done()
    return Case("ring_edge", s, o, 0, lambda t, s: _fast(t) and
                {x.offset for x in t if x.kind} >= {RING - 1, RING, RING + 1} and
                {x.length for x in t if x.kind and x.offset > RING} >= {FARQ, FARQ + 1} and
                {(x.out_off - x.offset) % 4 for x in t if x.kind and x.offset > RING and x.length <= FARQ} == {0, 1, 2, 3})


def _header_cuts():
    b = _B(13).lit(200)
    combos = [(d, k) for d in range(6) for k in ("copy4", "lit4")]
    for j, (d, k) in enumerate(combos):
        for bound in (SEG * (j + 1), SEG * (j + 1) + 3 * STEP + (j % 8) * STEP):
            b.comp_to(bound - 5 + d)                 # d = 5: the tag starts exactly on the boundary
            b.room(12, 200)
            b.copy(100 + j, 7, 3) if k == "copy4" else b.lit(9, 4)
    s, o = b.done(end_copy=True)

    def check(t, s):
        at = {(x.comp_off, "copy4" if x.kind == 3 else "lit4") for x in t if x.kind == 3 or x.form == 4}
        want = {(bound - 5 + d, k) for j, (d, k) in enumerate(combos)
                for bound in (SEG * (j + 1), SEG * (j + 1) + 3 * STEP + (j % 8) * STEP)}
        return _fast(t) and at >= want and t[-1].kind == 3 and t[-1].comp_off + 5 == len(s)
    return Case("header_cuts", s, o, 0, check)


# decoy literal bytes: what a walker that starts inside the literal parses
def _stride2(n, at):
    """00 xx ...: one-byte literals at the even stream offsets (at = the first byte's offset)."""
    return bytes(0 if (at + i) % 2 == 0 else 0xA5 for i in range(n))


def _decoys(b, many=False):
    """Long literals that span segments; returns [(kind, first stream byte, end)] of their data."""
    spans = []

    def put(kind, n, data):
        b.room(n + 1)
        at = b.c + 1 + ((n - 1).bit_length() + 7) // 8
        if kind == "late_join":
            n += at % 2                              # the data ends on an even offset: the chain lands there
        data = data(n, at)
        b.lit(data)
        spans.append((kind, at, at + n))
        b.room(12, 100).copy(50, 6, 1)
    reps = 19 if many else 1
    for _ in range(reps):
        put("stride2", 3 * SEG + 1, _stride2)
        put("copy4s", 2 * SEG + 3, lambda n, at: b"\xff" * n)
        # the walker's chain meets the true one only after more than REC / BUDGET tags: stride 2 for a
        # whole segment, ending so that the chain lands exactly on the next true tag
        put("late_join", 2 * SEG, _stride2)
        for _ in range(2 * BUDGET):                  # more true tags in the next segment than the link's budget
            b.room(12, 100).copy(9, 5, 1).lit(3)
    # a walker that starts on f4 / f8 / fc with a huge length runs off the stream's end and dies
    def dies(n, at):
        data = bytearray(b.rnd(n))
        for k, lead in zip(range((at + SEG - 1) // SEG, (at + n - 8) // SEG + 1),
                           (b"\xfc\xff\xff\xff\x7f", b"\xf8\xff\xff\xff", b"\xf4\xff\xff")):
            data[k * SEG - at:k * SEG - at + len(lead)] = lead
        return bytes(data)
    put("dies", 3 * SEG + 5, dies)
    return spans


def _decoy_check(spans, kinds):
    def check(t, s):
        true_at = {x.comp_off for x in t}
        seen = set()
        for kind, a, e in spans:
            for k in range((a + SEG - 1) // SEG, (e - 1) // SEG + 1):       # walkers that start inside the literal
                if not a <= k * SEG < e:
                    continue
                tags, status = walk(s, k * SEG, min((k + 1) * SEG, e))
                inside = [x for x in tags if x.comp_off < e - 5]
                if kind in ("stride2", "late_join") and len(inside) > REC and \
                        all(x.kind == 0 and x.length == 1 for x in inside) and not true_at & {x.comp_off for x in inside}:
                    if kind == "late_join" and (k + 1) * SEG >= e:
                        full, _ = walk(s, k * SEG, (k + 1) * SEG)               # ... and then joins the true chain
                        if e in {x.comp_off for x in full} and e in true_at:
                            seen.add(kind)
                    elif kind == "stride2":
                        seen.add(kind)
                if kind == "copy4s" and inside and all(x.kind == 3 and x.length == 64 for x in inside):
                    seen.add(kind)
                if kind == "dies" and status == "dead" and not tags:
                    seen.add(kind)
        return _fast(t) and seen >= set(kinds)
    return check


def _decoy_literals():
    b = _B(14).lit(100)
    spans = _decoys(b)
    b.lit(40)
    s, o = b.done()
    assert {k for k, _, _ in spans if k == "dies"} and len(s) - max(e for _, _, e in spans) < 4000
    return Case("decoy_literals", s, o, 0, _decoy_check(spans, ("stride2", "copy4s", "late_join", "dies")))


def _many_segments():
    b = _B(15).lit(100)
    spans = _decoys(b, many=True)
    b.lit(40)
    s, o = b.done()
    chk = _decoy_check(spans, ("stride2", "copy4s", "late_join", "dies"))
    return Case("many_segments", s, o, 0, lambda t, s: chk(t, s) and len(s) > 2 * 64 * SEG)


def valid_cases():
    """Each: one INT64 page whose raw values are the stream's output."""
    return [_copy4_near(), _copy4_far(), _lit_forms(), _lit_inside(), _straddle_copy(), _back(0), _back(1),
            _periods(0), _periods(1), _short_copy2(), _chains(), _ring_edge(), _header_cuts(),
            _decoy_literals(), _many_segments()]


def write_case(path, case):
    write_parquet(path, [("v", INT64, [Page(case.stream, len(case.out), len(case.out) // 8)])])


TINY_SERIAL = 0


def write_tiny(path):
    """Pages of no output, of one byte, a non-minimal preamble, and a crafted page next to one from
    Google's encoder (pyarrow) in the same chunk. Returns {"v": raw INT64 bytes, "s": [bytes, ...]}."""
    import pyarrow as pa
    rng = np.random.default_rng(16)
    v0 = rng.integers(0, 256, size=128, dtype=np.uint8).tobytes()
    v1 = rng.integers(0, 256, size=40, dtype=np.uint8).tobytes()
    raw = v1 * 50
    strs0 = [b"date=2024-01-%02d/part-%05d.snappy.parquet" % (i % 28 + 1, i) for i in range(8)]
    strs1 = [b"date=2024-02-%02d/part-%05d.snappy.parquet" % (i % 28 + 1, i) * (1 + i % 3) for i in range(250)]
    p0 = plain_byte_array(strs0)
    ops, at = [lit(p0[:40])], 40
    while at < len(p0):                              # the rest by hand: short literals and copies of the first row
        n = min(7, len(p0) - at)
        ops.append(lit(p0[at:at + n], 1 if at % 2 else None))
        at += n
    for at in range(0, len(p0), 64):                 # rows 8..15 = rows 0..7
        ops.append(copy(len(p0), min(64, len(p0) - at), 3 if at == 0 else 2))
    p1 = plain_byte_array(strs1)
    google = pa.Codec("snappy")
    vpages = [Page(build([lit(v0[:60], 4), lit(v0[60:])], 128, 4), 128, 16),  # non-minimal preamble (4 bytes for 128)
              Page(google.compress(raw, asbytes=True), len(raw), len(raw) // 8),
              # (a page without values ends pyarrow's read of the chunk: these two come last)
              Page(build([], 0), 0, 0),                                        # the preamble alone
              Page(build([lit(b"x")], 1), 1, 0)]                               # one byte of output, no value
    spages = [Page(build(ops, 2 * len(p0)), 2 * len(p0), 16),
              Page(google.compress(p1, asbytes=True), len(p1), 250)]
    for pg in vpages + spages[:1]:
        assert len(decode(pg.body)) == pg.usize
    write_parquet(path, [("v", INT64, vpages), ("s", BYTE_ARRAY, spages)])
    return {"v": v0 + raw, "s": strs0 + strs0 + strs1}


Bad = collections.namedtuple("Bad", "name stream usize stream_ok")


def malformed_cases():
    """Each names, in the comment beside it, the check that rejects it: `fix` = k_snap_fix (fragment
    and hybrid modes, and page mode's bitmap pass), `frag` = k_snap_frag, `serial` = k_snappy_serial,
    which decides for every page the others flag. The walkers read a window past the page: the file
    image is padded (dk_host.cpp: dfile alloc + 256) and snap_parse_d compares against clen before it
    uses a length."""
    r = np.random.default_rng(17).integers(0, 256, size=64, dtype=np.uint8).tobytes()
    c = []
    # frag: `off == 0 || off > ot - o0`; serial: `off == 0 || off > o`
    c.append(Bad("offset_zero", build([lit(r[:16]), copy(0, 8, 2), lit(r[:8])], 32), 32, False))
    c.append(Bad("first_tag_copy", build([copy(1, 8, 1), lit(r[:8])], 16), 16, False))
    c.append(Bad("offset_past_start", build([lit(r[:16]), copy(17, 8, 2)], 24), 24, False))
    # snap_tag / k_snap_frag clamp offsets over 2^31 - 1 to it, then the same comparison; serial holds 64 bits
    c.append(Bad("copy4_offset_2g", build([lit(r[:16]), copy(1 << 31, 8, 3)], 24), 24, False))
    c.append(Bad("copy4_offset_max", build([lit(r[:16]), copy((1 << 32) - 1, 8, 3)], 24), 24, False))
    # fix: `running != ulen`; frag (page mode): `o + total > o1` / `o + biglen > o1` before any store;
    # serial: `o + len > ulen` before the copy loop
    c.append(Bad("one_byte_more", build([lit(r[:17])], 16), 16, False))
    c.append(Bad("one_byte_more_copy", build([lit(r[:12]), copy(4, 5, 1)], 16), 16, False))
    # fix: `running != ulen`; serial: `o != ulen` after the last tag
    c.append(Bad("one_byte_less", build([lit(r[:15])], 16), 16, False))
    # fix, frag (page mode), serial: the preamble's value against pg.usize
    c.append(Bad("preamble_vs_header", build([lit(r[:16])], 16), 24, True))
    # walkers / link / fix: snap_parse(_d) `p + hdr + l > clen` -> exit -1 -> fix: `tex < 0`;
    # serial: `p + len > clen`
    c.append(Bad("literal_past_end", build([lit(r[:17])], 17)[:-1], 16, False))
    # snap_parse(_d): `p + hdr > clen` (copies), `p + hdr + l > clen` (literal); serial: `p + nb > clen`,
    # `p + 1 / 2 / 4 > clen`
    ok8 = build([lit(r[:8])], 8)
    c.append(Bad("cut_literal_header", ok8 + b"\xf4\x10", 8, False))
    c.append(Bad("cut_copy1_header", ok8 + b"\x01", 8, False))
    c.append(Bad("cut_copy2_header", ok8 + b"\x02\x04", 8, False))
    c.append(Bad("cut_copy4_header", ok8 + b"\x03\x04\x00\x00", 8, False))
    # snap_preamble: -1 after five bytes with the continuation bit (fix: `b0 < 0`; serial the same). The
    # low bits spell the page header's size, so only the length of the varint is wrong.
    c.append(Bad("preamble_five_continuations", b"\x90\x80\x80\x80\x80" + encode_op(lit(r[:16])), 16, False))
    c.append(Bad("preamble_33_bits", b"\x90\x80\x80\x80\x10" + encode_op(lit(r[:16])), 16, False))
    return c


def write_malformed(path, bad):
    """The bad page follows a good one in its chunk (an off-by-one before the page's output stays
    inside the decoder's arena)."""
    good = np.arange(16, dtype="<i8").tobytes()
    write_parquet(path, [("v", INT64, [Page(build([lit(good[:100]), lit(good[100:])], 128), 128, 16),
                                        Page(bad.stream, bad.usize, bad.usize // 8)])])
