// Zstandard frame decoding (RFC 8878) shared by the device kernel (dk_zstd.hip) and a host executor
// (tests/native/zstd_host.cpp): everything that does not depend on lane cooperation. One executor
// walks the frames and blocks of a page body; per compressed block it
//   1. zs_literals_plan   parses the literals header, builds the Huffman table, lays out the streams
//   2. zs_huf_stream      decodes one Huffman stream (the device runs the 4 streams on 4 lanes)
//   3. zs_sequences       parses the sequences header, builds the FSE tables and decodes every
//                         sequence once into a list of (literal length, match length, offset) with
//                         the repeat-offset rules applied and EVERY bound checked: literal cursor,
//                         output cursor, offset against the bytes the frame has produced
//   4. the executor copies literals and matches; it has nothing left to check.
// Every read is bounded by the section it belongs to, every loop by a count from a header that was
// checked against the bytes that remain, so damaged input ends in ZS_CORRUPT, never out of bounds.
#pragma once
#include <stdint.h>
#include "dk_thrift.h"

namespace dk {

enum : int32_t { ZS_OK = 0, ZS_CORRUPT = 1, ZS_UNSUPPORTED = 2 };
constexpr int ZS_BLOCK_MAX = 128 * 1024;      // Block_Maximum_Size
constexpr int ZS_HUF_LOG_MAX = 11;
constexpr int ZS_LL_LOG_MAX = 9, ZS_OF_LOG_MAX = 8, ZS_ML_LOG_MAX = 9;
constexpr int ZS_LL_MAXSYM = 35, ZS_OF_MAXSYM = 31, ZS_ML_MAXSYM = 52;

// per-page scratch sized from the page header: the literals of one block and its
// sequence list. A block regenerates at most min(body, 128 KiB) bytes and a match takes >= 3 of them.
DK_HD int64_t zs_lit_cap(int64_t body) { return body < ZS_BLOCK_MAX ? body : ZS_BLOCK_MAX; }
DK_HD int64_t zs_seq_cap(int64_t body) { return zs_lit_cap(body) / 3 + 1; }
struct ZSeq { uint32_t ll, ml, off; };
DK_HD int64_t zs_scratch_bytes(int64_t body) {
  return ((zs_lit_cap(body) + 15) & ~(int64_t)15) + 16 + zs_seq_cap(body) * (int64_t)sizeof(ZSeq);
}

struct ZFse { uint16_t base; uint8_t sym, nbits; };

// Tables and per-frame state: in LDS on the device (about 10 KiB), one per page being decoded.
struct ZWork {
  uint16_t huf[1 << ZS_HUF_LOG_MAX];     // symbol | code length << 8, indexed by the next huf_log bits
  ZFse ll[1 << ZS_LL_LOG_MAX], of[1 << ZS_OF_LOG_MAX], ml[1 << ZS_ML_LOG_MAX];
  ZFse wt[64];                           // FSE table of compressed Huffman weights (log <= 6)
  int16_t norm[256];                     // normalised distribution being read
  uint16_t next[256];                    // FSE build: next state per symbol
  uint8_t weights[256];
  int32_t huf_log, ll_log, of_log, ml_log;
  int32_t have_huf, have_ll, have_of, have_ml;
  uint32_t rep[3];
  // plan of the current block, read by every lane after a barrier
  int32_t status;
  int32_t lit_mode;                      // 0: literals in the input at lit_in, 1: RLE byte lit_byte, 2: Huffman streams
  int32_t lit_byte, n_streams;
  int64_t lit_in, lit_size;
  int64_t st_in[4], st_len[4], st_out[4], st_n[4];
  int32_t st_bad[4];
  int64_t seq_in;                        // first byte of the sequences section
  int32_t n_seq;
  int64_t lit_tail;                      // literals left after the last sequence
  int64_t block_out;                     // bytes the block regenerates
};

DK_HD int zs_highbit(uint32_t v) {       // v > 0
  int r = 0;
  while (v >>= 1) r++;
  return r;
}

// 8 bytes little-endian from p[off ..], bytes outside [0, n) read as zero
DK_HD uint64_t zs_load64(const uint8_t* p, int64_t n, int64_t off) {
  uint64_t w = 0;
  if (off >= 0 && off + 8 <= n) {
    __builtin_memcpy(&w, p + off, 8);
    return w;
  }
  for (int k = 0; k < 8; k++) {
    const int64_t i = off + k;
    if (i >= 0 && i < n) w |= (uint64_t)p[i] << (8 * k);
  }
  return w;
}

// ---- frame / block headers ---------------------------------------------------------------------
struct ZFrameHdr {
  int32_t skippable, hdr_len, checksum, has_fcs;
  int64_t skip_len;      // skippable: bytes after the 8-byte header
  uint64_t fcs;
};
// the frame header at in[0 .. n): ZS_OK and h filled, or an error
DK_HD int zs_frame_header(const uint8_t* in, int64_t n, ZFrameHdr& h) {
  h.skippable = 0; h.hdr_len = 0; h.checksum = 0; h.has_fcs = 0; h.skip_len = 0; h.fcs = 0;
  if (n < 5) return ZS_CORRUPT;
  const uint32_t magic = (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16 | (uint32_t)in[3] << 24;
  if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
    if (n < 8) return ZS_CORRUPT;
    h.skippable = 1; h.hdr_len = 8;
    h.skip_len = (int64_t)((uint32_t)in[4] | (uint32_t)in[5] << 8 | (uint32_t)in[6] << 16 | (uint32_t)in[7] << 24);
    if (h.skip_len > n - 8) return ZS_CORRUPT;
    return ZS_OK;
  }
  if (magic != 0xFD2FB528u) return ZS_CORRUPT;
  const uint8_t d = in[4];
  const int fcs_flag = d >> 6, single = (d >> 5) & 1, did_flag = d & 3;
  if (d & 8) return ZS_CORRUPT;                                  // reserved bit
  h.checksum = (d >> 2) & 1;
  const int did_len = did_flag == 3 ? 4 : did_flag;
  const int fcs_len = fcs_flag == 0 ? single : (fcs_flag == 1 ? 2 : (fcs_flag == 2 ? 4 : 8));
  const int len = 5 + (single ? 0 : 1) + did_len + fcs_len;
  if (n < len) return ZS_CORRUPT;
  int p = 5;
  if (!single) {
    // Window_Descriptor: offsets are checked against the bytes produced, so only its range matters
    if ((in[p] >> 3) > 31 - 10) return ZS_UNSUPPORTED;           // window above 2 GiB
    p++;
  }
  uint32_t did = 0;
  for (int k = 0; k < did_len; k++) did |= (uint32_t)in[p + k] << (8 * k);
  p += did_len;
  if (did != 0) return ZS_UNSUPPORTED;                           // Parquet carries no dictionary
  uint64_t fcs = 0;
  for (int k = 0; k < fcs_len; k++) fcs |= (uint64_t)in[p + k] << (8 * k);
  if (fcs_len == 2) fcs += 256;
  h.has_fcs = fcs_len > 0; h.fcs = fcs; h.hdr_len = len;
  return ZS_OK;
}

struct ZBlockHdr { int32_t last, type, size; };
DK_HD int zs_block_header(const uint8_t* in, int64_t n, ZBlockHdr& b) {
  b.last = 0; b.type = 0; b.size = 0;
  if (n < 3) return ZS_CORRUPT;
  const uint32_t v = (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16;
  b.last = v & 1; b.type = (v >> 1) & 3; b.size = (int32_t)(v >> 3);
  if (b.type == 3 || b.size > ZS_BLOCK_MAX) return ZS_CORRUPT;
  return ZS_OK;
}

// ---- FSE ---------------------------------------------------------------------------------------
// Normalised distribution at in[0 .. n) into norm[0 .. max_sym]; *consumed = its bytes.
DK_HD int zs_fse_read_dist(const uint8_t* in, int64_t n, int max_log, int max_sym, int16_t* norm, int* log_out,
                           int64_t* consumed) {
  if (n < 1) return ZS_CORRUPT;
  for (int i = 0; i <= max_sym; i++) norm[i] = 0;
  const int log = (in[0] & 15) + 5;
  if (log > max_log) return ZS_CORRUPT;
  int64_t bit = 4;
  int remaining = (1 << log) + 1, threshold = 1 << log, nb = log + 1, sym = 0;
  while (remaining > 1 && sym <= max_sym) {
    if ((bit >> 3) >= n) return ZS_CORRUPT;
    const int max = (2 * threshold - 1) - remaining;
    const uint32_t v = (uint32_t)(zs_load64(in, n, bit >> 3) >> (bit & 7));
    int count;
    if ((int)(v & (threshold - 1)) < max) {
      count = (int)(v & (threshold - 1));
      bit += nb - 1;
    } else {
      count = (int)(v & (2 * threshold - 1));
      if (count >= threshold) count -= max;
      bit += nb;
    }
    count--;                                                     // -1: "less than 1"
    remaining -= count < 0 ? 1 : count;
    if (remaining < 1) return ZS_CORRUPT;
    norm[sym++] = (int16_t)count;
    if (count == 0) {                                            // 2-bit repeat flags: further zeroes
      for (;;) {
        if ((bit >> 3) >= n) return ZS_CORRUPT;
        const int r = (int)((zs_load64(in, n, bit >> 3) >> (bit & 7)) & 3);
        bit += 2;
        sym += r;
        if (sym > max_sym + 1) return ZS_CORRUPT;
        if (r != 3) break;
      }
    }
    while (remaining < threshold && nb > 1) { nb--; threshold >>= 1; }
  }
  if (remaining != 1 || sym > max_sym + 1) return ZS_CORRUPT;
  const int64_t used = (bit + 7) >> 3;
  if (used > n) return ZS_CORRUPT;
  *log_out = log; *consumed = used;
  return ZS_OK;
}

// Decoding table of 1 << log states from norm[0 .. max_sym] (sums to 1 << log, -1 counting as 1).
DK_HD int zs_fse_build(const int16_t* norm, int max_sym, int log, ZFse* t, uint16_t* next) {
  const int size = 1 << log;
  int high = size - 1, total = 0;
  for (int s = 0; s <= max_sym; s++) {
    if (norm[s] == -1) {
      if (high < 0) return ZS_CORRUPT;
      t[high--].sym = (uint8_t)s; next[s] = 1; total += 1;
    } else {
      if (norm[s] < 0) return ZS_CORRUPT;
      next[s] = (uint16_t)norm[s]; total += norm[s];
    }
  }
  if (total != size) return ZS_CORRUPT;
  const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  int pos = 0;
  for (int s = 0; s <= max_sym; s++) {
    for (int i = 0; i < norm[s]; i++) {                          // (norm[s] <= size: bounded)
      t[pos].sym = (uint8_t)s;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;              // (high >= 0 here: a positive count is left)
    }
  }
  if (pos != 0) return ZS_CORRUPT;
  for (int u = 0; u < size; u++) {
    const int s = t[u].sym;
    const uint32_t x = next[s]++;
    const int nbits = log - zs_highbit(x);
    t[u].nbits = (uint8_t)nbits;
    t[u].base = (uint16_t)((x << nbits) - size);
  }
  return ZS_OK;
}

DK_HD void zs_default_dist(int which, int16_t* norm) {           // 0 LL, 1 OF, 2 ML
  const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                         1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  if (which == 0) for (int i = 0; i < 36; i++) norm[i] = ll[i];
  else if (which == 1) for (int i = 0; i < 29; i++) norm[i] = of[i];
  else for (int i = 0; i < 53; i++) norm[i] = ml[i];
}

// literal-length / match-length code -> (baseline, extra bits)
DK_HD void zs_ll_code(int c, uint32_t* base, int* bits) {
  const uint8_t xb[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  const uint32_t bl[20] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
  *bits = xb[c];
  *base = c < 16 ? (uint32_t)c : bl[c - 16];
}
DK_HD void zs_ml_code(int c, uint32_t* base, int* bits) {
  const uint8_t xb[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  const uint32_t bl[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
  if (c < 32) { *bits = 0; *base = (uint32_t)c + 3; }
  else { *bits = xb[c - 32]; *base = bl[c - 32]; }
}

// ---- backward bit reader -------------------------------------------------------------------------
// The stream is in[0 .. n); its last byte holds the end mark (highest set bit). `bits` unread bits
// remain, bit k being bit (k & 7) of byte k >> 3. A read past the start sets bad.
struct ZBits { const uint8_t* p; int64_t n, bits; int32_t bad; };
DK_HD ZBits zs_bits_init(const uint8_t* in, int64_t n) {
  ZBits b{in, n, 0, 0};
  if (n < 1 || in[n - 1] == 0) { b.bad = 1; b.n = 0; return b; }
  b.bits = 8 * (n - 1) + zs_highbit(in[n - 1]);
  return b;
}
DK_HD uint32_t zs_bits_read(ZBits& b, int nb) {                  // nb <= 32
  if (nb == 0) return 0;
  b.bits -= nb;
  if (b.bits < 0) { b.bad = 1; b.bits = 0; return 0; }
  const uint64_t w = zs_load64(b.p, b.n, b.bits >> 3) >> (b.bits & 7);
  return (uint32_t)(w & ((1ull << nb) - 1));
}
// the next nb bits without consuming them, zero-padded below the start of the stream (nb <= 16)
DK_HD uint32_t zs_bits_peek(const ZBits& b, int nb) {
  const int64_t lo = b.bits - nb;
  if (lo >= 0) return (uint32_t)((zs_load64(b.p, b.n, lo >> 3) >> (lo & 7)) & ((1u << nb) - 1));
  return (uint32_t)((zs_load64(b.p, b.n, 0) << (-lo)) & ((1u << nb) - 1));
}

// ---- Huffman -------------------------------------------------------------------------------------
// Weights at in[0 .. n) (direct 4-bit or FSE-compressed) into W.weights and the decoding table.
DK_HD int zs_huf_read(const uint8_t* in, int64_t n, ZWork& W, int64_t* consumed) {
  if (n < 1) return ZS_CORRUPT;
  const int h = in[0];
  int ns = 0;
  if (h >= 128) {
    ns = h - 127;
    const int nbytes = (ns + 1) / 2;
    if (1 + nbytes > n) return ZS_CORRUPT;
    for (int i = 0; i < ns; i++) W.weights[i] = (i & 1) ? (in[1 + i / 2] & 15) : (in[1 + i / 2] >> 4);
    *consumed = 1 + nbytes;
  } else {
    if (h == 0 || 1 + h > n) return ZS_CORRUPT;
    int log = 0;
    int64_t used = 0;
    int rc = zs_fse_read_dist(in + 1, h, 6, 255, W.norm, &log, &used);
    if (rc) return rc;
    int top = 255;                                               // symbols above the last non-zero count are unused
    while (top > 0 && W.norm[top] == 0) top--;
    if (top > 11) return ZS_CORRUPT;                             // a weight above 11
    rc = zs_fse_build(W.norm, top, log, W.wt, W.next);
    if (rc) return rc;
    ZBits b = zs_bits_init(in + 1 + used, h - used);
    if (b.bad) return ZS_CORRUPT;
    uint32_t s1 = zs_bits_read(b, log), s2 = zs_bits_read(b, log);
    if (b.bad) return ZS_CORRUPT;
    for (;;) {                                                   // two interleaved states; at most 255 weights
      if (ns > 253) return ZS_CORRUPT;
      W.weights[ns++] = W.wt[s1].sym;
      if (b.bits < W.wt[s1].nbits) { W.weights[ns++] = W.wt[s2].sym; break; }
      s1 = W.wt[s1].base + zs_bits_read(b, W.wt[s1].nbits);
      if (ns > 253) return ZS_CORRUPT;
      W.weights[ns++] = W.wt[s2].sym;
      if (b.bits < W.wt[s2].nbits) { W.weights[ns++] = W.wt[s1].sym; break; }
      s2 = W.wt[s2].base + zs_bits_read(b, W.wt[s2].nbits);
    }
    *consumed = 1 + h;
  }
  // the last weight completes the sum of 2^(w-1) to a power of two
  uint32_t sum = 0;
  for (int i = 0; i < ns; i++) {
    if (W.weights[i] > ZS_HUF_LOG_MAX) return ZS_CORRUPT;
    if (W.weights[i]) sum += 1u << (W.weights[i] - 1);
  }
  if (sum == 0) return ZS_CORRUPT;
  const int log = zs_highbit(sum) + 1;
  if (log > ZS_HUF_LOG_MAX) return ZS_CORRUPT;
  const uint32_t rest = (1u << log) - sum;
  if (rest & (rest - 1)) return ZS_CORRUPT;                      // (rest > 0: sum < 1 << log)
  W.weights[ns++] = (uint8_t)(zs_highbit(rest) + 1);
  // codes in order of weight, then of symbol: weight w takes 2^(w-1) entries of log - w + 1 bits
  int pos = 0;
  for (int w = 1; w <= log; w++)
    for (int s = 0; s < ns; s++)
      if (W.weights[s] == w) {
        const int len = 1 << (w - 1);
        if (pos + len > (1 << log)) return ZS_CORRUPT;
        const uint16_t e = (uint16_t)(s | (log + 1 - w) << 8);
        for (int k = 0; k < len; k++) W.huf[pos + k] = e;
        pos += len;
      }
  if (pos != (1 << log)) return ZS_CORRUPT;
  W.huf_log = log; W.have_huf = 1;
  return ZS_OK;
}

// One Huffman stream in[0 .. n) into out[0 .. out_n): 0, or 1 when the stream is damaged.
DK_HD int zs_huf_stream(const uint8_t* in, int64_t n, const uint16_t* tab, int log, uint8_t* out, int64_t out_n) {
  ZBits b = zs_bits_init(in, n);
  if (b.bad) return 1;
  for (int64_t o = 0; o < out_n; o++) {
    const uint16_t e = tab[zs_bits_peek(b, log)];
    b.bits -= e >> 8;
    if (b.bits < 0) return 1;
    out[o] = (uint8_t)e;
  }
  return b.bits != 0;
}

// Literals section of a compressed block body in[0 .. n): fills W's plan (lit_mode, streams) and
// *consumed (offsets are relative to the page body, in_base being in's). lit_cap: the page's literals scratch.
DK_HD int zs_literals_plan(const uint8_t* in, int64_t n, int64_t in_base, int64_t lit_cap, ZWork& W, int64_t* consumed) {
  if (n < 1) return ZS_CORRUPT;
  const int type = in[0] & 3, sf = (in[0] >> 2) & 3;
  int64_t regen = 0, comp = 0;
  int hl;
  if (type < 2) {
    hl = sf == 1 ? 2 : (sf == 3 ? 3 : 1);
    if (n < hl) return ZS_CORRUPT;
    if (hl == 1) regen = in[0] >> 3;
    else if (hl == 2) regen = (in[0] >> 4) | (int64_t)in[1] << 4;
    else regen = (in[0] >> 4) | (int64_t)in[1] << 4 | (int64_t)in[2] << 12;
  } else {
    hl = sf < 2 ? 3 : (sf == 2 ? 4 : 5);
    if (n < hl) return ZS_CORRUPT;
    uint64_t v = 0;
    for (int k = 0; k < hl; k++) v |= (uint64_t)in[k] << (8 * k);
    v >>= 4;
    const int nb = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
    regen = (int64_t)(v & ((1u << nb) - 1));
    comp = (int64_t)((v >> nb) & ((1u << nb) - 1));
  }
  if (regen > lit_cap || regen > ZS_BLOCK_MAX) return ZS_CORRUPT;
  W.lit_size = regen; W.n_streams = 0;
  if (type == 0) {
    if (hl + regen > n) return ZS_CORRUPT;
    W.lit_mode = 0; W.lit_in = in_base + hl;
    *consumed = hl + regen;
    return ZS_OK;
  }
  if (type == 1) {
    if (hl + 1 > n) return ZS_CORRUPT;
    W.lit_mode = 1; W.lit_byte = in[hl];
    *consumed = hl + 1;
    return ZS_OK;
  }
  if (hl + comp > n) return ZS_CORRUPT;
  const uint8_t* p = in + hl;
  int64_t left = comp;
  if (type == 2) {
    int64_t used = 0;
    const int rc = zs_huf_read(p, left, W, &used);
    if (rc) return rc;
    p += used; left -= used;
  } else if (!W.have_huf) return ZS_CORRUPT;                     // Treeless with no previous table
  W.lit_mode = 2;
  const int ns = sf == 0 ? 1 : 4;
  W.n_streams = ns;
  if (ns == 1) {
    if (left < 1) return ZS_CORRUPT;
    W.st_in[0] = in_base + (p - in); W.st_len[0] = left; W.st_out[0] = 0; W.st_n[0] = regen;
  } else {
    if (left < 6) return ZS_CORRUPT;
    const int64_t s1 = p[0] | p[1] << 8, s2 = p[2] | p[3] << 8, s3 = p[4] | p[5] << 8;
    const int64_t s4 = left - 6 - s1 - s2 - s3;
    if (s4 < 1 || s1 < 1 || s2 < 1 || s3 < 1) return ZS_CORRUPT;
    const int64_t q = (regen + 3) / 4;
    if (regen < 3 * q) return ZS_CORRUPT;
    const int64_t base = in_base + (p - in) + 6;
    W.st_in[0] = base; W.st_in[1] = base + s1; W.st_in[2] = base + s1 + s2; W.st_in[3] = base + s1 + s2 + s3;
    W.st_len[0] = s1; W.st_len[1] = s2; W.st_len[2] = s3; W.st_len[3] = s4;
    for (int k = 0; k < 4; k++) { W.st_out[k] = q * k; W.st_n[k] = k < 3 ? q : regen - 3 * q; }
  }
  *consumed = hl + comp;
  return ZS_OK;
}

// ---- sequences -------------------------------------------------------------------------------------
// One of the three tables, per its mode; *p advances over what it reads.
DK_HD int zs_seq_table(int mode, int which, const uint8_t* in, int64_t n, int64_t* p, ZWork& W) {
  ZFse* t = which == 0 ? W.ll : (which == 1 ? W.of : W.ml);
  int32_t& have = which == 0 ? W.have_ll : (which == 1 ? W.have_of : W.have_ml);
  int32_t& tlog = which == 0 ? W.ll_log : (which == 1 ? W.of_log : W.ml_log);
  const int max_sym = which == 0 ? ZS_LL_MAXSYM : (which == 1 ? ZS_OF_MAXSYM : ZS_ML_MAXSYM);
  const int max_log = which == 0 ? ZS_LL_LOG_MAX : (which == 1 ? ZS_OF_LOG_MAX : ZS_ML_LOG_MAX);
  if (mode == 3) return have ? ZS_OK : ZS_CORRUPT;               // Repeat with no previous table
  if (mode == 1) {
    if (*p >= n) return ZS_CORRUPT;
    const int s = in[(*p)++];
    if (s > max_sym) return ZS_CORRUPT;
    t[0].sym = (uint8_t)s; t[0].nbits = 0; t[0].base = 0;
    tlog = 0; have = 1;
    return ZS_OK;
  }
  int log;
  if (mode == 0) {
    zs_default_dist(which, W.norm);
    log = which == 1 ? 5 : 6;
  } else {
    int64_t used = 0;
    const int rc = zs_fse_read_dist(in + *p, n - *p, max_log, max_sym, W.norm, &log, &used);
    if (rc) return rc;
    *p += used;
  }
  const int rc = zs_fse_build(W.norm, mode == 0 ? (which == 0 ? 35 : (which == 1 ? 28 : 52)) : max_sym, log, t, W.next);
  if (rc) return rc;
  tlog = log; have = 1;
  return ZS_OK;
}

// The sequences section in[0 .. n) of a block: tables, then every sequence into seq[0 .. seq_cap).
// frame_out: bytes this frame produced before the block; out_left: bytes the page may still take.
// On ZS_OK: W.n_seq, W.lit_tail and W.block_out are set, and for every sequence the literal cursor
// stays within W.lit_size, the output within min(out_left, 128 KiB) and 1 <= off <= the bytes the
// frame has produced at that point.
DK_HD int zs_sequences(const uint8_t* in, int64_t n, ZWork& W, ZSeq* seq, int64_t seq_cap, int64_t frame_out,
                       int64_t out_left) {
  if (n < 1) return ZS_CORRUPT;
  const int64_t out_max = out_left < ZS_BLOCK_MAX ? out_left : ZS_BLOCK_MAX;
  int64_t p = 0;
  int64_t ns;
  const int b0 = in[p++];
  if (b0 < 128) ns = b0;
  else if (b0 < 255) { if (n < 2) return ZS_CORRUPT; ns = ((int64_t)(b0 - 128) << 8) + in[p++]; }
  else { if (n < 3) return ZS_CORRUPT; ns = (int64_t)in[p] + ((int64_t)in[p + 1] << 8) + 0x7F00; p += 2; }
  W.n_seq = 0;
  if (ns == 0) {
    if (p != n) return ZS_CORRUPT;
    if (W.lit_size > out_max) return ZS_CORRUPT;
    W.lit_tail = W.lit_size; W.block_out = W.lit_size;
    return ZS_OK;
  }
  if (ns > seq_cap) return ZS_CORRUPT;                           // more matches than the block has bytes for
  if (p >= n) return ZS_CORRUPT;
  const int modes = in[p++];
  if (modes & 3) return ZS_CORRUPT;
  const int m_ll = modes >> 6, m_of = (modes >> 4) & 3, m_ml = (modes >> 2) & 3;
  int rc;
  if ((rc = zs_seq_table(m_ll, 0, in, n, &p, W))) return rc;
  if ((rc = zs_seq_table(m_of, 1, in, n, &p, W))) return rc;
  if ((rc = zs_seq_table(m_ml, 2, in, n, &p, W))) return rc;
  ZBits b = zs_bits_init(in + p, n - p);
  if (b.bad) return ZS_CORRUPT;
  uint32_t s_ll = zs_bits_read(b, W.ll_log), s_of = zs_bits_read(b, W.of_log), s_ml = zs_bits_read(b, W.ml_log);
  if (b.bad) return ZS_CORRUPT;
  int64_t lit = 0, out = 0;
  uint32_t r0 = W.rep[0], r1 = W.rep[1], r2 = W.rep[2];
  for (int64_t i = 0; i < ns; i++) {
    const ZFse e_ll = W.ll[s_ll], e_of = W.of[s_of], e_ml = W.ml[s_ml];
    const int oc = e_of.sym;                                     // <= 31 (table symbols are bounded)
    uint32_t lb, mb;
    int lx, mx;
    zs_ll_code(e_ll.sym, &lb, &lx);
    zs_ml_code(e_ml.sym, &mb, &mx);
    const uint64_t ov = (1ull << oc) + zs_bits_read(b, oc);
    const uint32_t ml = mb + zs_bits_read(b, mx);
    const uint32_t ll = lb + zs_bits_read(b, lx);
    if (b.bad) return ZS_CORRUPT;
    uint64_t off;
    if (ov > 3) {
      off = ov - 3;
      if (off > 0x7FFFFFFFull) return ZS_CORRUPT;
      r2 = r1; r1 = r0; r0 = (uint32_t)off;
    } else {
      const int idx = (int)ov + (ll == 0 ? 1 : 0);               // 1..4
      if (idx == 1) off = r0;
      else if (idx == 2) { off = r1; r1 = r0; r0 = (uint32_t)off; }
      else {
        off = idx == 3 ? r2 : (uint64_t)r0 - 1;
        if (off == 0) return ZS_CORRUPT;
        r2 = r1; r1 = r0; r0 = (uint32_t)off;
      }
    }
    lit += ll;
    if (lit > W.lit_size) return ZS_CORRUPT;
    out += ll;
    if (off == 0 || off > (uint64_t)(frame_out + out)) return ZS_CORRUPT;   // before the frame's first byte
    out += ml;
    if (out > out_max) return ZS_CORRUPT;
    seq[i].ll = ll; seq[i].ml = ml; seq[i].off = (uint32_t)off;
    if (i + 1 < ns) {                                            // state updates: LL, ML, OF
      s_ll = e_ll.base + zs_bits_read(b, e_ll.nbits);
      s_ml = e_ml.base + zs_bits_read(b, e_ml.nbits);
      s_of = e_of.base + zs_bits_read(b, e_of.nbits);
      if (b.bad) return ZS_CORRUPT;
    }
  }
  if (b.bits != 0) return ZS_CORRUPT;                            // the stream is consumed exactly
  W.lit_tail = W.lit_size - lit;
  out += W.lit_tail;
  if (out > out_max) return ZS_CORRUPT;
  W.rep[0] = r0; W.rep[1] = r1; W.rep[2] = r2;
  W.n_seq = (int32_t)ns; W.block_out = out;
  return ZS_OK;
}

DK_HD void zs_frame_reset(ZWork& W) {
  W.have_huf = W.have_ll = W.have_of = W.have_ml = 0;
  W.rep[0] = 1; W.rep[1] = 4; W.rep[2] = 8;
}

// ---- the walk over a page body ---------------------------------------------------------------------
// One executor X decodes in[0 .. clen) (any number of frames, skippable ones included) into
// out[0 .. ulen). The walk is the same on the host (a serial executor) and on the device (one wave):
// headers are parsed by every lane from the same bytes, the leader fills W's plan between barriers,
// and X supplies the cooperative parts:
//   leader()                     one lane of the executor
//   barrier()                    W and the scratch written before it are visible after it
//   copy(dst, src, n)            input bytes to the output (raw blocks)
//   fill(dst, byte, n)           RLE blocks
//   literals(W, in, lits)        the block's Huffman streams (or its RLE byte) into lits; 0 when sound
//   execute(W, lsrc, seq, out, op)   the literal / match copies of a block whose sequence list
//                                zs_sequences has checked
template <class X>
DK_HD int zs_decode_body(X& x, const uint8_t* in, int64_t clen, uint8_t* out, int64_t ulen, ZWork& W, uint8_t* lits,
                         ZSeq* seq) {
  const int64_t lit_cap = zs_lit_cap(ulen), seq_cap = zs_seq_cap(ulen);
  int64_t ip = 0, op = 0;
  while (ip < clen) {                                            // frames: each takes >= 5 input bytes
    ZFrameHdr fh;
    int rc = zs_frame_header(in + ip, clen - ip, fh);
    if (rc) return rc;
    ip += fh.hdr_len;
    if (fh.skippable) { ip += fh.skip_len; continue; }
    const int64_t frame0 = op;
    if (x.leader()) zs_frame_reset(W);
    x.barrier();
    for (;;) {                                                   // blocks: each takes >= 3 input bytes
      ZBlockHdr bh;
      rc = zs_block_header(in + ip, clen - ip, bh);
      if (rc) return rc;
      ip += 3;
      if (bh.type == 0) {
        if (bh.size > clen - ip || bh.size > ulen - op) return ZS_CORRUPT;
        x.copy(out + op, in + ip, bh.size);
        ip += bh.size; op += bh.size;
      } else if (bh.type == 1) {
        if (clen - ip < 1 || bh.size > ulen - op) return ZS_CORRUPT;
        x.fill(out + op, in[ip], bh.size);
        ip += 1; op += bh.size;
      } else {
        if (bh.size > clen - ip) return ZS_CORRUPT;
        if (x.leader()) {
          int64_t used = 0;
          W.status = zs_literals_plan(in + ip, bh.size, ip, lit_cap, W, &used);
          W.seq_in = ip + used;
        }
        x.barrier();
        if (W.status) return W.status;
        if (x.literals(W, in, lits)) return ZS_CORRUPT;
        if (x.leader())
          W.status = zs_sequences(in + W.seq_in, ip + bh.size - W.seq_in, W, seq, seq_cap, op - frame0, ulen - op);
        x.barrier();
        if (W.status) return W.status;
        const int64_t produced = W.block_out;
        x.execute(W, W.lit_mode == 0 ? in + W.lit_in : lits, seq, out, op);
        ip += bh.size; op += produced;
      }
      if (bh.last) break;
    }
    if (fh.checksum) {                                           // Content_Checksum: skipped, not verified
      if (clen - ip < 4) return ZS_CORRUPT;
      ip += 4;
    }
    if (fh.has_fcs && fh.fcs != (uint64_t)(op - frame0)) return ZS_CORRUPT;
  }
  return op == ulen ? ZS_OK : ZS_CORRUPT;
}

}  // namespace dk
