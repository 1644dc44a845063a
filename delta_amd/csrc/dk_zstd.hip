// ZSTD-compressed Parquet pages: one wave decodes one page body into the arena at
// pg.unc_off, where snappy's kernels put theirs. The walk over frames and blocks, the table
// construction, the sequence decode and every bound check are dk_zstd.h's (shared with the host
// executor the tests sanitise); this file adds the wave executor:
//   - the block's 4 Huffman streams decode on 4 lanes (a single stream on one),
//   - lane 0 decodes the FSE sequences once into the page's sequence list,
//   - literal and match copies run 64 bytes per step across the wave.
// Tables and per-frame state (ZWork, ~11 KiB) live in LDS; literals and the sequence list in the
// per-page scratch prepare() sized from the page header.
#include <hip/hip_runtime.h>
#include "dk_device.h"
#include "dk_thrift.h"
#include "dk_zstd.h"

namespace dk {

struct WaveX {
  int lane;
  int64_t fenced;          // output bytes below this offset are visible to every lane

  __device__ bool leader() const { return lane == 0; }
  __device__ void barrier() { __syncthreads(); }
  __device__ void copy(uint8_t* dst, const uint8_t* src, int64_t n) {
    for (int64_t i = lane; i < n; i += 64) dst[i] = src[i];
  }
  __device__ void fill(uint8_t* dst, uint8_t b, int64_t n) {
    for (int64_t i = lane; i < n; i += 64) dst[i] = b;
  }
  __device__ int literals(ZWork& W, const uint8_t* in, uint8_t* lits) {
    const int mode = W.lit_mode, ns = W.n_streams;
    if (mode == 1) {
      fill(lits, (uint8_t)W.lit_byte, W.lit_size);
    } else if (mode == 2 && lane < ns) {
      W.st_bad[lane] = zs_huf_stream(in + W.st_in[lane], W.st_len[lane], W.huf, W.huf_log, lits + W.st_out[lane], W.st_n[lane]);
    }
    __syncthreads();
    int bad = 0;
    if (mode == 2) for (int k = 0; k < ns; k++) bad |= W.st_bad[k];
    return bad;
  }
  // Sequences checked by zs_sequences: literal cursor, output cursor and offsets are in range. A match
  // reads bytes other lanes stored, so a workgroup-scope release / acquire pair orders them whenever
  // the source reaches past the last fenced output position (as k_snappy_serial does).
  __device__ void execute(ZWork& W, const uint8_t* ls, const ZSeq* seq, uint8_t* out, int64_t op) {
    const int ns = W.n_seq;
    const int64_t tail = W.lit_tail;
    int64_t o = op, lp = 0;
    for (int i = 0; i < ns; i++) {
      const ZSeq q = seq[i];
      for (int64_t k = lane; k < (int64_t)q.ll; k += 64) out[o + k] = ls[lp + k];
      o += q.ll; lp += q.ll;
      const int64_t off = q.off, len = q.ml, src = o - off;
      if (src + (off < len ? off : len) > fenced) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        fenced = o;
      }
      if (off >= len) {
        for (int64_t k = lane; k < len; k += 64) out[o + k] = out[src + k];
      } else {
        for (int64_t k = lane; k < len; k += 64) out[o + k] = out[src + (k % off)];
      }
      o += len;
    }
    for (int64_t k = lane; k < tail; k += 64) out[o + k] = ls[lp + k];
    __syncthreads();         // W's plan and the scratch are free for the next block
  }
};

// zpage[i]: page index; zoff[i]: the page's offset in the scratch (zs_scratch_bytes of its body)
__global__ __launch_bounds__(64) void k_zstd_page(const DChunk* __restrict__ chunks, DPage* __restrict__ pages,
                                                  uint8_t* __restrict__ arena, const int32_t* __restrict__ zpage,
                                                  const int64_t* __restrict__ zoff, uint8_t* __restrict__ scratch) {
  __shared__ ZWork W;
  DPage& pgw = pages[zpage[blockIdx.x]];
  const DPage pg = pgw;                            // by value: byte stores below may alias
  if (pg.unc_off < 0 || pg.status != PS_OK) return;
  const DChunk ck = chunks[pg.chunk];
  const int lane = threadIdx.x;
  const uint8_t* in = ck.file + pg.data_off;
  int64_t clen = pg.csize;
  uint8_t* out = arena + pg.unc_off;
  int64_t ulen = pg.usize;
  const int64_t lv = (pg.ptype == PAGE_DATA_V2) ? (int64_t)pg.rl_len + pg.dl_len : 0;
  if (lv < 0 || lv > clen || lv > ulen) { if (lane == 0) pgw.status = PS_BAD_ZSTD; return; }
  for (int64_t i = lane; i < lv; i += 64) out[i] = in[i];   // v2: the levels are not compressed
  in += lv; clen -= lv; out += lv; ulen -= lv;
  uint8_t* lits = scratch + zoff[blockIdx.x];
  ZSeq* seq = (ZSeq*)(lits + ((zs_lit_cap(ulen) + 15) & ~(int64_t)15) + 16);
  WaveX x{lane, 0};
  const int rc = zs_decode_body(x, in, clen, out, ulen, W, lits, seq);
  if (rc && lane == 0) pgw.status = rc == ZS_UNSUPPORTED ? PS_UNSUPPORTED : PS_BAD_ZSTD;
}

void launch_zstd(const DChunk* chunks, DPage* pages, uint8_t* arena, const int32_t* zpage, const int64_t* zoff,
                 uint8_t* scratch, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_zstd_page, dim3(n), dim3(64), 0, s, chunks, pages, arena, zpage, zoff, scratch);
}

}  // namespace dk
