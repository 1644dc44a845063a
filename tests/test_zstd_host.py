"""The shared ZSTD decoder (delta_amd/csrc/dk_zstd.h) on the host: tests/native/zstd_host.cpp drives
the same frame walk, table construction, sequence decode and bound checks the GPU kernel runs with a
serial executor, built with -fsanitize=address,undefined as a stand-alone binary.

Corpus: pyarrow's bundled encoder at levels -5, 1, 3, 9, 19 over inputs chosen so that every mode it
can be made to emit is present (tests/zstd_inspect.py asserts each), plus hand-assembled frames for
the modes it does not emit -- each of those first proven through pyarrow's own decompressor.
Damaged input: every prefix of three small frames, single-byte flips, and hand-built invalid frames.
A prefix must be refused; a flip must be refused or decode in bounds (a flipped payload byte decodes
to other bytes of the same length: only the content checksum, which is not verified, could tell)."""
import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pytest

from tests import zstd_inspect

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "delta_amd", "csrc")
SRC = os.path.join(HERE, "native", "zstd_host.cpp")
LEVELS = (-5, 1, 3, 9, 19)
MAGIC = b"\x28\xb5\x2f\xfd"


def corpus_inputs():
    rng = np.random.default_rng(1)
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9)).astype(np.uint8)) for _ in range(300)]

    def text(n):
        out, t = [], 0
        while t < n:
            w = words[int(rng.zipf(1.3)) % 300]
            out.append(w)
            t += len(w) + 1
        return b" ".join(out)[:n]
    return {
        "empty": b"", "rand": rng.bytes(5000), "zeros": bytes(300_000), "text2k": text(2000), "text400k": text(400_000),
        "paths": b"".join(b"part-%05d-abcdef-%d.c000.snappy.parquet\n" % (i, i * 7919) for i in range(5000)),
        "arange": np.arange(50_000, dtype=np.int64).tobytes(),
        "skew": bytes(rng.choice([65, 66, 67, 68], 200_000, p=[.7, .2, .07, .03]).astype(np.uint8)),
        "ab": (b"a" * 100 + b"b") * 50, "xyzw": rng.bytes(3) + b"XYZW" * 5000,
        "mix": rng.bytes(200_000) + bytes(200_000) + b"ABCDEFGH" * 30_000,
        "rand64": bytes(rng.integers(0, 64, 60_000).astype(np.uint8)),       # Huffman literals, no sequences
    }


# ---- hand-assembled frames --------------------------------------------------------------------------

def xxh64(data, seed=0):
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda a, v: (rotl((a + v * P2) & M, 31) * P1) & M
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while p + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[p + 8 * k:p + 8 * k + 8], "little"))
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(data[p:p + 4], "little") * P1 & M), 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5 & M), 11) * P1) & M
        p += 1
    h = ((h ^ (h >> 33)) * P2) & M
    h = ((h ^ (h >> 29)) * P3) & M
    return h ^ (h >> 32)


def block(btype, body, last=True, size=None):
    size = len(body) if size is None else size
    return (size << 3 | btype << 1 | int(last)).to_bytes(3, "little") + body


def frame(blocks, fcs=None, checksum_of=None):
    """Single-segment frame with a 4-byte Frame_Content_Size (or none: a window descriptor instead)."""
    if fcs is None:
        hdr = MAGIC + bytes([0x04 if checksum_of is not None else 0x00, 0x58])
    else:
        hdr = MAGIC + bytes([0xA0 | (0x04 if checksum_of is not None else 0)]) + fcs.to_bytes(4, "little")
    out = hdr + b"".join(blocks)
    if checksum_of is not None:
        out += (xxh64(checksum_of) & 0xFFFFFFFF).to_bytes(4, "little")
    return out


def backward_bits(bits):
    """A backward bit stream: `bits` ('0'/'1' in the order the decoder reads them) under its end mark."""
    v = int("1" + bits, 2)
    return v.to_bytes((v.bit_length() + 7) // 8, "little")


def rle_seq_block(lits, n_seq, ll_code, of_code, of_bits="00", ml_code=0):
    """Compressed block: raw literals, n_seq sequences with all three tables in RLE mode (states take no
    bits), so each sequence is its offset's extra bits alone."""
    n = len(lits)
    lh = (0 | 3 << 2 | n << 4).to_bytes(3, "little")                     # raw, 20-bit size
    if n_seq < 128:
        cnt = bytes([n_seq])
    elif n_seq < 0x7F00:
        cnt = bytes([128 + (n_seq >> 8), n_seq & 255])
    else:
        cnt = b"\xff" + (n_seq - 0x7F00).to_bytes(2, "little")
    modes = bytes([1 << 6 | 1 << 4 | 1 << 2, ll_code, of_code, ml_code])
    return block(2, lh + lits + cnt + modes + backward_bits(of_bits * n_seq))


def valid_frames():
    """name -> (frame bytes, expected bytes, tags zstd_inspect must report)."""
    out = {}
    out["rle_literals"] = (frame([block(2, bytes([10 << 3 | 1, 0x41, 0]))], 10), b"A" * 10, {"lit:rle", "seq:count0"})
    # direct weights: symbol 0 weight 2, symbol 1 weight 1, symbol 2 (implied) weight 1 -> codes 1, 00, 01
    syms = [0, 0, 1, 2, 0, 0, 0, 2]
    stream = backward_bits("".join({0: "1", 1: "00", 2: "01"}[s] for s in syms))
    tree = bytes([129, 0x21])
    lh = (2 | 0 << 2 | len(syms) << 4 | (len(tree) + len(stream)) << 14).to_bytes(3, "little")
    out["direct_weights"] = (frame([block(2, lh + tree + stream + b"\x00")], len(syms)), bytes(syms),
                             {"lit:huffman", "lit:streams1", "huf:direct"})
    # 0x7F00 sequences in one block: one literal, then a 3-byte match at offset 1 (offset code 2, bits 00)
    lits = bytes(i * 37 % 251 for i in range(0x7F00))
    big = b"".join(bytes([b]) * 4 for b in lits)
    out["count3"] = (frame([rle_seq_block(lits, 0x7F00, 1, 2)], len(big)), big, {"seq:count3", "ll:rle", "of:rle", "ml:rle"})
    small = frame([block(0, b"hello ")], 6)
    out["skippable"] = (b"\x53\x2a\x4d\x18" + (5).to_bytes(4, "little") + b"12345" + small, b"hello ", {"frame:skippable"})
    out["checksum"] = (frame([block(0, b"checked")], 7, checksum_of=b"checked"), b"checked", {"frame:checksum"})
    out["two_frames"] = (small + frame([block(1, b"z", size=9)], 9), b"hello " + b"z" * 9, {"frames:2", "block:rle"})
    # no Frame_Content_Size at all (a window descriptor instead): pyarrow's one-shot encoder always
    # writes the size, so this form is hand-built too
    out["no_fcs"] = (frame([block(0, b"sizeless")]), b"sizeless", {"frame:fcs0", "frame:windowed"})
    return out


def invalid_frames():
    """name -> (frame bytes, usize, 'bad' | 'unsup')."""
    out = {}
    treeless = (3 | 0 << 2 | 4 << 4 | 2 << 14).to_bytes(3, "little") + b"\x01\x01" + b"\x00"
    out["treeless_first"] = (frame([block(2, treeless)], 4), 4, "bad")
    rep = (0 | 3 << 2 | 4 << 4).to_bytes(3, "little") + b"abcd" + bytes([1, 3 << 6 | 3 << 4 | 3 << 2]) + b"\x01"
    out["repeat_first"] = (frame([block(2, rep)], 7), 7, "bad")
    out["offset_before_start"] = (frame([rle_seq_block(b"", 1, 0, 2)], 3), 3, "bad")
    out["offset_past_history"] = (frame([rle_seq_block(b"ab", 1, 2, 3, "000")], 5), 5, "bad")      # offset 5 after 2 bytes
    out["block_too_large"] = (frame([block(0, b"x" * 16, size=131073)], 131073), 131073, "bad")
    out["reserved_block"] = (frame([block(3, b"abc")], 3), 3, "bad")
    out["content_size"] = (frame([block(0, b"0123456789")], 11), 10, "bad")
    out["usize_short"] = (frame([block(0, b"0123456789")], 10), 9, "bad")
    out["usize_long"] = (frame([block(0, b"0123456789")], 10), 11, "bad")
    acc = (0 | 3 << 2 | 4 << 4).to_bytes(3, "little") + b"abcd" + bytes([1, 2 << 6, 0x05, 0xff, 0xff]) + b"\x01"
    out["accuracy_log"] = (frame([block(2, acc)], 7), 7, "bad")
    out["bad_magic"] = (b"\x29" + frame([block(0, b"abc")], 3)[1:], 3, "bad")
    out["reserved_bit"] = (MAGIC + bytes([0xA8]) + (3).to_bytes(4, "little") + block(0, b"abc"), 3, "bad")
    out["dictionary_id"] = (MAGIC + bytes([0x01, 0x58, 0x07]) + block(0, b"abc"), 3, "unsup")
    out["dictionary_id_zero"] = (MAGIC + bytes([0x01, 0x58, 0x00]) + block(0, b"abc"), 3, "ok")
    return out


REQUIRED_FROM_PYARROW = {
    "block:raw", "block:rle", "block:compressed", "blocks:many",
    "lit:raw", "lit:huffman", "lit:treeless", "lit:streams1", "lit:streams4", "huf:fse",
    "seq:count0", "seq:count1", "seq:count2",
    "frame:single_segment", "frame:windowed", "frame:fcs1", "frame:fcs2", "frame:fcs4",
} | {t + ":" + m for t in ("ll", "of", "ml") for m in zstd_inspect.MODES}
REQUIRED_BY_HAND = {"lit:rle", "huf:direct", "seq:count3", "frame:skippable", "frame:checksum", "frames:2", "frame:fcs0"}


def _pyarrow_corpus():
    out = {}
    for name, data in corpus_inputs().items():
        for lv in LEVELS:
            out["%s_L%d" % (name, lv)] = (pa.Codec("zstd", compression_level=lv).compress(data, asbytes=True), data)
    return out


def test_corpus_holds_every_mode():
    seen = set()
    for comp, _ in _pyarrow_corpus().values():
        seen |= zstd_inspect.inspect(comp)
    assert REQUIRED_FROM_PYARROW <= seen, sorted(REQUIRED_FROM_PYARROW - seen)
    hand = set()
    for name, (fr, want, tags) in valid_frames().items():
        got = zstd_inspect.inspect(fr)
        assert tags <= got, (name, sorted(tags - got))
        hand |= got
        # the fixture is proven by pyarrow's decoder before ours sees it
        assert pa.Codec("zstd").decompress(fr, len(want), asbytes=True) == want, name
    assert REQUIRED_BY_HAND <= hand, sorted(REQUIRED_BY_HAND - hand)
    assert "frame:dict_id" in zstd_inspect.inspect(invalid_frames()["dictionary_id"][0])


def _write_manifest(d):
    lines = []

    def put(name, data):
        p = os.path.join(d, name)
        with open(p, "wb") as f:
            f.write(data)
        return p
    for name, (comp, data) in _pyarrow_corpus().items():
        lines.append("ok %s %s" % (put(name + ".zst", comp), put(name + ".bin", data)))
    for name, (fr, want, _) in valid_frames().items():
        lines.append("ok %s %s" % (put(name + ".zst", fr), put(name + ".bin", want)))
    for name, (fr, usize, kind) in invalid_frames().items():
        lines.append("%s %s %s" % (kind, put(name + ".zst", fr), put(name + ".bin", bytes(usize))
                                   if kind != "ok" else put(name + ".bin", b"abc")))
    for name in ("text2k_L3", "ab_L3", "xyzw_L3"):
        for kind in ("trunc", "flip"):
            lines.append("%s %s %s" % (kind, os.path.join(d, name + ".zst"), os.path.join(d, name + ".bin")))
    for name in ("mix_L3", "count3", "direct_weights", "two_frames"):
        lines.append("flip %s %s" % (os.path.join(d, name + ".zst"), os.path.join(d, name + ".bin")))
    mf = os.path.join(d, "manifest")
    with open(mf, "w") as f:
        f.write("\n".join(lines) + "\n")
    n_ok = sum(ln.startswith("ok ") for ln in lines)
    n_bad = sum(ln.startswith(("bad ", "unsup ")) for ln in lines)
    return mf, n_ok, n_bad


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_decoder(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "zstd_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run([cxx, "-std=c++17"] + flags + ["-I", CSRC, SRC, "-o", exe], check=True)
    mf, n_ok, n_bad = _write_manifest(str(tmp_path))
    out = subprocess.run([exe, mf], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    decoded, refused, survived, altered = map(int, out.stdout.split()[1:5])
    assert decoded == n_ok
    assert refused > n_bad + 1000        # the prefixes and most flips
