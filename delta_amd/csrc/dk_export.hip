// Scan-file batch reader, device half (dk_replay_scan_open / dk_scan_next, include/dkgpu.h; DESIGN.md
// "Scan-file batch reader").
//
// A finished replay leaves one selection byte per checkpoint row in HBM beside the decoded columns.
// The compacting reader ships only the selected rows to the host:
//   selected-row list  once per file: ballot over the selection bytes (one u64 per wave), popcount per
//                      wave, the shared three-pass exclusive scan (enc_exscan, dk_encode.hip) over the
//                      wave counts, then each selected row lands at wave base + popcount of the lower
//                      lanes -> an ordered int32 list of file rows
//   windows            ranges of that list; per leaf and window: count entries / chars per selected
//                      row (k_exp_count), scan the counts, then gather row levels, int32
//                      offsets, values and validity bits (k_exp_rows, k_exp_entries) and the chars
//                      (k_exp_chars) into device staging laid out as the host window, which goes to
//                      pinned memory in one stream-ordered copy.
// Validity words are written by ballot, one u64 per 64 output values, the last word included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dk_device.h"

namespace dk {

// the device exclusive scan shared with the checkpoint writer (dk_encode.hip)
void enc_exscan(const long long* in, long long n, long long* out, long long* sums, long long* total, hipStream_t s);

constexpr int EXP = 256;

// ---- selected-row list ----
__global__ __launch_bounds__(EXP) void k_exp_sel_count(const uint8_t* __restrict__ sel, long long n,
                                                       long long* __restrict__ wcnt) {
  const long long i = (long long)blockIdx.x * EXP + threadIdx.x;
  const unsigned long long m = __ballot(i < n && sel[i] != 0);
  if ((threadIdx.x & 63) == 0 && i < n) wcnt[i >> 6] = __popcll(m);
}

__global__ __launch_bounds__(EXP) void k_exp_sel_rows(const uint8_t* __restrict__ sel, long long n,
                                                      const long long* __restrict__ wbase, int32_t* __restrict__ rows) {
  const long long i = (long long)blockIdx.x * EXP + threadIdx.x;
  const bool on = i < n && sel[i] != 0;
  const unsigned long long m = __ballot(on);
  if (on) rows[wbase[i >> 6] + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1))] = (int32_t)i;
}

// ---- per leaf and window ----
__global__ __launch_bounds__(EXP) void k_exp_count(ExportLeaf L) {
  const long long j = (long long)blockIdx.x * EXP + threadIdx.x;
  if (j >= L.nr) return;
  const long long r = L.rows[j];
  if (L.repeated) {
    const long long e0 = L.row_offs[r], e1 = L.row_offs[r + 1];
    L.cnt_e[j] = e1 - e0;
    if (L.is_str) L.cnt_c[j] = L.offs[e1] - L.offs[e0];
  } else {
    L.cnt_c[j] = L.offs[r + 1] - L.offs[r];
  }
}

__device__ __forceinline__ void exp_copy_fixed(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int w) {
  if (w == 8) *(uint64_t*)dst = *(const uint64_t*)src;
  else if (w == 4) *(uint32_t*)dst = *(const uint32_t*)src;
  else for (int k = 0; k < w; k++) dst[k] = src[k];
}

// one thread per output row (and one more for the closing offsets): row levels; non-repeated leaves:
// validity, values or offsets; repeated leaves: row offsets and the source of every output entry
__global__ __launch_bounds__(EXP) void k_exp_rows(ExportLeaf L) {
  const long long j = (long long)blockIdx.x * EXP + threadIdx.x;
  bool nn = false;
  if (j < L.nr) {
    const long long r = L.rows[j];
    const int d = L.row_def[r];
    L.o_rowdef[j] = (uint8_t)d;
    if (!L.null_only) {
      if (L.repeated) {
        const long long e0 = L.row_offs[r], n = L.row_offs[r + 1] - e0, b = L.eb[j];
        L.o_rowoffs[j] = (int32_t)b;
        for (long long k = 0; k < n; k++) { L.esrc[b + k] = e0 + k; L.erow[b + k] = (int32_t)j; }
      } else {
        nn = d == L.max_def;
        if (L.is_str) L.o_offs[j] = (int32_t)L.cb[j];
        else exp_copy_fixed(L.o_fixed + j * L.width, L.fixed + r * L.width, L.width);
      }
    }
  } else if (j == L.nr && !L.null_only) {
    if (L.repeated) L.o_rowoffs[j] = (int32_t)L.nv;
    else if (L.is_str) L.o_offs[j] = (int32_t)L.nc;
  }
  if (L.null_only || L.repeated) return;
  const unsigned long long m = __ballot(nn);
  if ((threadIdx.x & 63) == 0 && j < L.nr) L.o_bits[j >> 6] = m;     // (the tail word too)
}

// repeated leaves: one thread per output entry (and one more for the closing offset)
__global__ __launch_bounds__(EXP) void k_exp_entries(ExportLeaf L) {
  const long long e = (long long)blockIdx.x * EXP + threadIdx.x;
  bool nn = false;
  if (e < L.nv) {
    const long long s = L.esrc[e];
    const int d = L.entry_def[s];
    L.o_entdef[e] = (uint8_t)d;
    nn = d == L.max_def;
    if (L.is_str) {
      const long long j = L.erow[e];
      L.o_offs[e] = (int32_t)(L.cb[j] + (L.offs[s] - L.offs[L.row_offs[L.rows[j]]]));
    } else {
      exp_copy_fixed(L.o_fixed + e * L.width, L.fixed + s * L.width, L.width);
    }
  } else if (e == L.nv && L.is_str) {
    L.o_offs[e] = (int32_t)L.nc;
  }
  const unsigned long long m = __ballot(nn);
  if ((threadIdx.x & 63) == 0 && e < L.nv) L.o_bits[e >> 6] = m;
}

// Chars: one wave per 64 consecutive output values, whose destination bytes are one contiguous run.
// The lanes stride that run in 16-byte destination chunks; a chunk inside one value whose source is
// 16-byte aligned too moves as one 16-byte load and store, any other chunk is assembled from byte
// loads (neighbouring lanes read neighbouring bytes) and stored whole, or byte by byte at the two
// ends of the run, which share their chunks with the neighbouring waves.
__global__ __launch_bounds__(EXP) void k_exp_chars(ExportLeaf L) {
  __shared__ int32_t s_dst[EXP / 64][65];
  __shared__ long long s_src[EXP / 64][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long v0 = ((long long)blockIdx.x * (EXP / 64) + wv) * 64;
  const int cnt = (int)(L.nv - v0 < 64 ? (L.nv - v0 > 0 ? L.nv - v0 : 0) : 64);
  if (lane < cnt) {
    const long long v = v0 + lane;
    s_dst[wv][lane] = L.o_offs[v];
    s_src[wv][lane] = L.offs[L.repeated ? L.esrc[v] : (long long)L.rows[v]];
  }
  if (lane == 0 && cnt > 0) s_dst[wv][cnt] = L.o_offs[v0 + cnt];
  __syncthreads();
  if (cnt == 0) return;
  const int32_t* dst = s_dst[wv];
  const long long* src = s_src[wv];
  const long long D0 = dst[0], D1 = dst[cnt];
  if (D1 <= D0) return;
  const long long c0 = D0 >> 4, c1 = (D1 - 1) >> 4;
  for (long long c = c0 + lane; c <= c1; c += 64) {
    const long long base = c << 4;
    const long long lo = base > D0 ? base : D0, hi = base + 16 < D1 ? base + 16 : D1;
    // the last value starting at or before lo (empty values before it are skipped)
    int a = 0, b = cnt - 1;
    while (a < b) { const int mid = (a + b + 1) >> 1; if (dst[mid] <= lo) a = mid; else b = mid - 1; }
    int v = a;
    const bool whole = lo == base && hi == base + 16;
    if (whole && dst[v + 1] >= hi) {
      const uint8_t* sp = L.chars + src[v] + (lo - dst[v]);
      if (((uintptr_t)sp & 15) == 0) { *(uint4*)(L.o_chars + base) = *(const uint4*)sp; continue; }
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const long long p = base + k;
      uint32_t byte = 0;
      if (p >= lo && p < hi) {
        while (p >= dst[v + 1]) v++;
        byte = L.chars[src[v] + (p - dst[v])];
      }
      w[k >> 2] |= byte << ((k & 3) * 8);
    }
    if (whole) {
      *(uint4*)(L.o_chars + base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const long long p = base + k;
        if (p >= lo && p < hi) L.o_chars[p] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
      }
    }
  }
}

__global__ __launch_bounds__(EXP) void k_exp_rowidx(const int32_t* __restrict__ rows, long long n, int64_t* __restrict__ out) {
  const long long j = (long long)blockIdx.x * EXP + threadIdx.x;
  if (j < n) out[j] = rows[j];
}

// ---- launchers (grids sized from the window) ----
static unsigned exp_grid(long long n) { return (unsigned)((n + EXP - 1) / EXP); }

long long exp_sel_waves(long long n) { return (n + 63) / 64; }
// rows[0 .. *total) = the rows of sel[0 .. n) with a non-zero byte, ascending; wcnt, wbase:
// exp_sel_waves(n) values each, sums: enc_scan_blocks(waves) values, total: one value (device)
void exp_sel_rows(const uint8_t* sel, long long n, long long* wcnt, long long* wbase, long long* sums, long long* total,
                  int32_t* rows, hipStream_t s) {
  if (n <= 0) { hipMemsetAsync(total, 0, 8, s); return; }
  hipLaunchKernelGGL(k_exp_sel_count, dim3(exp_grid(n)), dim3(EXP), 0, s, sel, n, wcnt);
  enc_exscan(wcnt, exp_sel_waves(n), wbase, sums, total, s);
  hipLaunchKernelGGL(k_exp_sel_rows, dim3(exp_grid(n)), dim3(EXP), 0, s, sel, n, wbase, rows);
}
void exp_count(const ExportLeaf& L, hipStream_t s) {
  if (L.nr > 0) hipLaunchKernelGGL(k_exp_count, dim3(exp_grid(L.nr)), dim3(EXP), 0, s, L);
}
void exp_gather(const ExportLeaf& L, hipStream_t s) {
  hipLaunchKernelGGL(k_exp_rows, dim3(exp_grid(L.nr + 1)), dim3(EXP), 0, s, L);
  if (L.null_only) return;
  if (L.repeated) hipLaunchKernelGGL(k_exp_entries, dim3(exp_grid(L.nv + 1)), dim3(EXP), 0, s, L);
  if (L.is_str && L.nv > 0 && L.nc > 0)
    hipLaunchKernelGGL(k_exp_chars, dim3((unsigned)((L.nv + EXP - 1) / EXP)), dim3(EXP), 0, s, L);
}
void exp_rowidx(const int32_t* rows, long long n, int64_t* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_exp_rowidx, dim3(exp_grid(n)), dim3(EXP), 0, s, rows, n, out);
}

}  // namespace dk
