// Host executor for delta_amd/csrc/dk_zstd.h: the same frame walk, table construction, sequence
// decode and bound checks the device kernel (dk_zstd.hip) runs, driven by a plain serial executor.
// tests/test_zstd_host.py builds it (with and without -fsanitize=address,undefined) and runs it over
// a manifest of lines "<kind> <frame file> <expected bytes file>":
//   ok     the frame decodes to the expected bytes
//   bad    the frame is refused (ZS_CORRUPT)
//   unsup  the frame is refused as unsupported (ZS_UNSUPPORTED)
//   trunc  every proper prefix of the frame is refused or gives the expected bytes
//   flip   every single-byte damage of a deterministic set is refused, gives the expected bytes, or
//          (payload bytes, which only the unverified content checksum covers) other bytes in bounds
// Input, output and scratch are heap blocks of exactly the sizes the device gives a page, so a read or
// write outside them is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "dk_zstd.h"

using namespace dk;

struct HostX {
  bool leader() const { return true; }
  void barrier() {}
  void copy(uint8_t* dst, const uint8_t* src, int64_t n) { if (n) memcpy(dst, src, (size_t)n); }
  void fill(uint8_t* dst, uint8_t b, int64_t n) { if (n) memset(dst, b, (size_t)n); }
  int literals(ZWork& W, const uint8_t* in, uint8_t* lits) {
    if (W.lit_mode == 1) fill(lits, (uint8_t)W.lit_byte, W.lit_size);
    else if (W.lit_mode == 2)
      for (int k = 0; k < W.n_streams; k++)
        if (zs_huf_stream(in + W.st_in[k], W.st_len[k], W.huf, W.huf_log, lits + W.st_out[k], W.st_n[k])) return 1;
    return 0;
  }
  void execute(ZWork& W, const uint8_t* ls, const ZSeq* seq, uint8_t* out, int64_t op) {
    int64_t o = op, lp = 0;
    for (int i = 0; i < W.n_seq; i++) {
      const ZSeq q = seq[i];
      copy(out + o, ls + lp, q.ll);
      o += q.ll; lp += q.ll;
      for (uint32_t k = 0; k < q.ml; k++) out[o + k] = out[o + k - q.off];
      o += q.ml;
    }
    copy(out + o, ls + lp, W.lit_tail);
  }
};

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// decode in[0 .. n) as a page body of `want.size()` bytes: rc, and whether the bytes are right
static int decode(const uint8_t* src, size_t n, const std::vector<uint8_t>& want, bool* same) {
  const int64_t ulen = (int64_t)want.size();
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(in, src, n);
  uint8_t* out = (uint8_t*)malloc(ulen ? ulen : 1);
  uint8_t* scratch = (uint8_t*)malloc((size_t)zs_scratch_bytes(ulen));
  ZSeq* seq = (ZSeq*)(scratch + ((zs_lit_cap(ulen) + 15) & ~(int64_t)15) + 16);
  ZWork* W = (ZWork*)malloc(sizeof(ZWork));
  memset(W, 0, sizeof(ZWork));
  HostX x;
  const int rc = zs_decode_body(x, in, (int64_t)n, out, ulen, *W, scratch, seq);
  *same = rc == ZS_OK && (ulen == 0 || memcmp(out, want.data(), (size_t)ulen) == 0);
  free(W); free(scratch); free(out); free(in);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: zstd_host <manifest>\n"); return 2; }
  std::ifstream mf(argv[1]);
  std::string line;
  long decoded = 0, refused = 0, survived = 0, altered = 0;
  while (std::getline(mf, line)) {
    std::istringstream ls(line);
    std::string kind, fpath, epath;
    if (!(ls >> kind >> fpath >> epath)) continue;
    const std::vector<uint8_t> frame = slurp(fpath), want = slurp(epath);
    bool same = false;
    if (kind == "ok") {
      const int rc = decode(frame.data(), frame.size(), want, &same);
      if (rc != ZS_OK || !same) { printf("FAIL ok %s: rc %d same %d\n", fpath.c_str(), rc, (int)same); return 1; }
      decoded++;
    } else if (kind == "bad" || kind == "unsup") {
      const int rc = decode(frame.data(), frame.size(), want, &same);
      if (rc != (kind == "bad" ? ZS_CORRUPT : ZS_UNSUPPORTED)) { printf("FAIL %s %s: rc %d\n", kind.c_str(), fpath.c_str(), rc); return 1; }
      refused++;
    } else if (kind == "trunc") {
      for (size_t n = 0; n < frame.size(); n++) {
        const int rc = decode(frame.data(), n, want, &same);
        if (rc == ZS_OK && !same) { printf("FAIL trunc %s at %zu: wrong bytes accepted\n", fpath.c_str(), n); return 1; }
        if (rc == ZS_OK) survived++; else refused++;
      }
    } else if (kind == "flip") {
      // every byte of a short frame, a stride through a long one; three damages per position
      const size_t step = frame.size() <= 2048 ? 1 : frame.size() / 1024;
      const uint8_t masks[3] = {0x01, 0x80, 0xFF};
      std::vector<uint8_t> d = frame;
      for (size_t i = 0; i < frame.size(); i += step)
        for (uint8_t m : masks) {
          d[i] = frame[i] ^ m;
          const int rc = decode(d.data(), d.size(), want, &same);
          // a damaged raw literal or in-range offset decodes to other bytes of the same length: the
          // format cannot tell without the content checksum (not verified); such
          // cases are counted apart. What this run proves is that they all stayed in bounds.
          if (rc == ZS_OK && !same) altered++;
          else if (rc == ZS_OK) survived++; else refused++;
          d[i] = frame[i];
        }
    } else { printf("FAIL unknown kind %s\n", kind.c_str()); return 1; }
  }
  printf("ok %ld %ld %ld %ld\n", decoded, refused, survived, altered);
  return 0;
}
