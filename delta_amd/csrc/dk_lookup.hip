// Row lookups over a decoded column (dk_parquet_find_bytes / dk_parquet_nonnull_rows, include/dkgpu.h;
// DESIGN.md §4.8): the device half of the two "first one wins" replays behind
// Snapshot.getLatestTransactionVersion and Snapshot.getDomainMetadataMap
// (internal/replay/LogReplay.java:316-342, :356-378).
//
//   k_find_bytes     first row >= from_row whose string is non-null and byte-equal to a needle: one
//                    lane per row, tiles of 256 rows taken grid-stride in ascending order; the length
//                    is compared first, only lanes whose length matches read chars; a wave that holds
//                    a match publishes its lowest row with one atomicMin and stops, and every wave
//                    stops at the first tile that starts beyond the row published so far.
//   k_lk_count/rows  ascending list of the rows >= from_row whose definition level is >= min_def:
//                    ballot + popcount per wave over the level bytes, the shared exclusive scan
//                    (enc_exscan, dk_encode.hip) over the wave counts, then each row lands at wave
//                    base + popcount of the lower lanes; rows past the caller's capacity are counted
//                    but not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dk {

void enc_exscan(const long long* in, long long n, long long* out, long long* sums, long long* total, hipStream_t s);

constexpr int LK = 256;
constexpr int LK_NEEDLE_LDS = 1024;   // needles up to this many bytes are compared out of LDS

__global__ __launch_bounds__(LK) void k_find_bytes(const uint8_t* __restrict__ row_def, const int64_t* __restrict__ offs,
                                                   const uint8_t* __restrict__ chars, long long n_rows, int max_def,
                                                   long long from_row, const uint8_t* __restrict__ needle, int n,
                                                   unsigned long long* out) {
  __shared__ uint8_t s_needle[LK_NEEDLE_LDS];
  const bool lds = n <= LK_NEEDLE_LDS;
  if (lds) for (int k = threadIdx.x; k < n; k += LK) s_needle[k] = needle[k];
  __syncthreads();
  const uint8_t* nd = lds ? s_needle : needle;
  const int lane = threadIdx.x & 63;
  for (long long t0 = from_row + (long long)blockIdx.x * LK; t0 < n_rows; t0 += (long long)gridDim.x * LK) {
    // the row published so far, read by lane 0 for the whole wave (the loop stays wave-uniform)
    unsigned long long cur = lane == 0 ? __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    cur = __shfl(cur, 0);
    if ((unsigned long long)t0 > cur) break;
    const long long r = t0 + threadIdx.x;
    bool hit = false;
    if (r < n_rows && row_def[r] >= max_def) {
      const long long a = offs[r];
      if (offs[r + 1] - a == n) {
        int k = 0;
        while (k < n && chars[a + k] == nd[k]) k++;
        hit = k == n;
      }
    }
    const unsigned long long m = __ballot(hit);
    if (m) {
      if (lane == 0) atomicMin(out, (unsigned long long)(r + (__ffsll((long long)m) - 1)));
      break;
    }
  }
}

__global__ __launch_bounds__(LK) void k_lk_count(const uint8_t* __restrict__ def, long long n, int min_def,
                                                 long long* __restrict__ wcnt) {
  const long long i = (long long)blockIdx.x * LK + threadIdx.x;
  const unsigned long long m = __ballot(i < n && def[i] >= min_def);
  if ((threadIdx.x & 63) == 0 && i < n) wcnt[i >> 6] = __popcll(m);
}

__global__ __launch_bounds__(LK) void k_lk_rows(const uint8_t* __restrict__ def, long long n, int min_def, long long row0,
                                                const long long* __restrict__ wbase, int64_t* __restrict__ rows,
                                                long long cap) {
  const long long i = (long long)blockIdx.x * LK + threadIdx.x;
  const bool on = i < n && def[i] >= min_def;
  const unsigned long long m = __ballot(on);
  if (!on) return;
  const long long pos = wbase[i >> 6] + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1));
  if (pos < cap) rows[pos] = row0 + i;
}

// *out (preset to ~0 by the caller) = the first matching row of [from_row, n_rows); needle: n device bytes
void launch_find_bytes(const uint8_t* row_def, const int64_t* offs, const uint8_t* chars, long long n_rows, int max_def,
                       long long from_row, const uint8_t* needle, int n, unsigned long long* out, hipStream_t s) {
  const long long want = (n_rows - from_row + LK - 1) / LK;
  if (want <= 0) return;
  const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
  hipLaunchKernelGGL(k_find_bytes, dim3(grid), dim3(LK), 0, s, row_def, offs, chars, n_rows, max_def, from_row, needle, n,
                     out);
}

// rows[0 .. min(*total, cap)) = row0 + i for the i in [0, n) with def[i] >= min_def, ascending; wcnt,
// wbase: (n + 63) / 64 values each, sums: enc_scan_blocks of that many, total: one value (device)
void lk_nonnull_rows(const uint8_t* def, long long n, int min_def, long long row0, long long* wcnt, long long* wbase,
                     long long* sums, long long* total, int64_t* rows, long long cap, hipStream_t s) {
  if (n <= 0) { hipMemsetAsync(total, 0, 8, s); return; }
  const unsigned grid = (unsigned)((n + LK - 1) / LK);
  hipLaunchKernelGGL(k_lk_count, dim3(grid), dim3(LK), 0, s, def, n, min_def, wcnt);
  enc_exscan(wcnt, (n + 63) / 64, wbase, sums, total, s);
  if (cap > 0) hipLaunchKernelGGL(k_lk_rows, dim3(grid), dim3(LK), 0, s, def, n, min_def, row0, wbase, rows, cap);
}

}  // namespace dk
