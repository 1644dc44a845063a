"""A small Zstandard (RFC 8878) frame walker for the tests. It decodes nothing: it reads the frame,
block, literals-section and sequences-section headers of a buffer and reports which forms occur, so
that a test can assert its corpus really holds each mode the decoder (delta_amd/csrc/dk_zstd.h)
claims to handle. Only well-formed input is expected; anything else raises ValueError."""

MODES = ("predefined", "rle", "fse", "repeat")


def inspect(buf):
    """A set of tags over every frame in `buf`:
    frame:skippable, frame:single_segment, frame:windowed, frame:checksum, frame:dict_id, frame:fcsN
    (N = field bytes 0/1/2/4/8), frames:N, block:raw|rle|compressed, blocks:many (a frame with > 1
    block), lit:raw|rle|huffman|treeless, lit:streams1|streams4, huf:direct|fse, seq:count0|count1|
    count2|count3 (bytes of the count; count0 = no sequences), ll:|of:|ml: + MODES."""
    buf = bytes(buf)
    tags, p, frames = set(), 0, 0
    while p < len(buf):
        if len(buf) - p < 4:
            raise ValueError("truncated magic")
        magic = int.from_bytes(buf[p:p + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            tags.add("frame:skippable")
            p += 8 + int.from_bytes(buf[p + 4:p + 8], "little")
            continue
        if magic != 0xFD2FB528:
            raise ValueError("bad magic at %d" % p)
        frames += 1
        d = buf[p + 4]
        p += 5
        single, fcs_flag, did_flag = (d >> 5) & 1, d >> 6, d & 3
        tags.add("frame:single_segment" if single else "frame:windowed")
        if d & 4:
            tags.add("frame:checksum")
        if not single:
            p += 1
        did_len = (0, 1, 2, 4)[did_flag]
        if int.from_bytes(buf[p:p + did_len], "little"):
            tags.add("frame:dict_id")
        p += did_len
        fcs_len = (single, 2, 4, 8)[fcs_flag]
        tags.add("frame:fcs%d" % fcs_len)
        p += fcs_len
        nblocks = 0
        while True:
            h = int.from_bytes(buf[p:p + 3], "little")
            if len(buf) - p < 3:
                raise ValueError("truncated block header")
            p += 3
            last, btype, size = h & 1, (h >> 1) & 3, h >> 3
            nblocks += 1
            if btype == 0:
                tags.add("block:raw")
                p += size
            elif btype == 1:
                tags.add("block:rle")
                p += 1
            elif btype == 2:
                tags.add("block:compressed")
                _block(buf, p, size, tags)
                p += size
            else:
                raise ValueError("reserved block type")
            if last:
                break
        if nblocks > 1:
            tags.add("blocks:many")
        if d & 4:
            p += 4
    if p != len(buf):
        raise ValueError("trailing or missing bytes")
    tags.add("frames:%d" % frames)
    return tags


def _block(buf, p, size, tags):
    end = p + size
    b0 = buf[p]
    ltype, sf = b0 & 3, (b0 >> 2) & 3
    tags.add("lit:" + ("raw", "rle", "huffman", "treeless")[ltype])
    if ltype < 2:
        hl = 2 if sf == 1 else 3 if sf == 3 else 1
        regen = int.from_bytes(buf[p:p + hl], "little") >> (3 if hl == 1 else 4)
        tags.add("litsize:%d" % hl)
        p += hl + (regen if ltype == 0 else 1)
    else:
        hl = 3 if sf < 2 else 4 if sf == 2 else 5
        nb = 10 if sf < 2 else 14 if sf == 2 else 18
        v = int.from_bytes(buf[p:p + hl], "little") >> 4
        comp = (v >> nb) & ((1 << nb) - 1)
        tags.add("lit:streams1" if sf == 0 else "lit:streams4")
        tags.add("litsize:%d" % hl)
        if ltype == 2:
            tags.add("huf:direct" if buf[p + hl] >= 128 else "huf:fse")
        p += hl + comp
    if p >= end:
        raise ValueError("no sequences section")
    s0 = buf[p]
    if s0 == 0:
        tags.add("seq:count0")
        return
    if s0 < 128:
        tags.add("seq:count1"); p += 1
    elif s0 < 255:
        tags.add("seq:count2"); p += 2
    else:
        tags.add("seq:count3"); p += 3
    m = buf[p]
    tags.add("ll:" + MODES[m >> 6])
    tags.add("of:" + MODES[(m >> 4) & 3])
    tags.add("ml:" + MODES[(m >> 2) & 3])
