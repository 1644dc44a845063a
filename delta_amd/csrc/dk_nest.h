// Nested repetition (a leaf under more than one repeated node): the level-to-element rule, in one
// place for the device kernels (k_nest_count / k_nest_fill, dk_kernels.hip), the host runtime and a
// stand-alone host program (tests/native/nest_host.cpp).
//
// A leaf has max_rep = R repeated nodes on its path; list_def[k], k = 1..R, is the definition level
// of the k-th of them (the non-required nodes from the root through that node). A level (rep r,
// def d) of the leaf's level streams
//   starts a row                 iff r == 0                      (depth 0)
//   is a depth-k element         iff r <= k && d >= list_def[k]  (k = 1..R)
// so a level that is a depth-k element is the FIRST level of that element, and a depth-(k-1) element
// whose first level is no depth-k element holds no depth-k element at all: its def tells whether the
// list is empty (list_def[k] - 1) or the list or one of its ancestors is null (below that).
//
// The structure is one offset array per depth (Arrow's ListArray nesting):
//   offs_k[j], j <= n_{k-1}   depth-k elements before the j-th depth-(k-1) element (offs_k[n_{k-1}] = n_k)
//   def_{k-1}[j], j < n_{k-1} the definition level at that parent's first level (def_0 = row_def)
// with n_0 the rows and n_R the entries the value arrays are dense over.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DK_NEST_HD __host__ __device__ __forceinline__
#else
#define DK_NEST_HD inline
#endif

namespace dk {

constexpr int DK_NEST_MAX = 4;    // deepest supported max_rep

enum : int32_t { NEST_NULL = 0, NEST_EMPTY = 1, NEST_HAS = 2 };

// is the level (rep, def) a depth-k element? k = 0: a row; k >= 1: list_def_k = list_def[k]
DK_NEST_HD bool nest_is_elem(int rep, int def, int k, int list_def_k) {
  return k == 0 ? rep == 0 : (rep <= k && def >= list_def_k);
}

// what a depth-(k-1) element whose first level has definition level `def` holds at depth k
DK_NEST_HD int32_t nest_classify(int def, int list_def_k) {
  return def >= list_def_k ? NEST_HAS : def == list_def_k - 1 ? NEST_EMPTY : NEST_NULL;
}

// The serial reference: n levels -> n_k (k = 0..R), offs_k (k = 1..R, at offs[k - 1], n_{k-1} + 1
// entries each) and def_k (k = 0..R-1, at defs[k], n_k entries each). Null output pointers count
// only. list_def[k - 1] holds list_def[k].
DK_NEST_HD void nest_walk(const uint8_t* rep, const uint8_t* def, int64_t n, int R, const int32_t* list_def,
                          int64_t* n_out, int64_t* const* offs, uint8_t* const* defs) {
  int64_t cnt[DK_NEST_MAX + 1];
  for (int k = 0; k <= R; k++) cnt[k] = 0;
  for (int64_t i = 0; i < n; i++) {
    const int r = rep[i], d = def[i];
    bool is[DK_NEST_MAX + 1];
    for (int k = 0; k <= R; k++) is[k] = nest_is_elem(r, d, k, k ? list_def[k - 1] : 0);
    for (int k = 0; k < R; k++)
      if (is[k]) {
        if (offs && offs[k]) offs[k][cnt[k]] = cnt[k + 1];
        if (defs && defs[k]) defs[k][cnt[k]] = (uint8_t)d;
      }
    for (int k = 0; k <= R; k++) cnt[k] += is[k];
  }
  for (int k = 0; k < R; k++)
    if (offs && offs[k]) offs[k][cnt[k]] = cnt[k + 1];
  for (int k = 0; k <= R; k++) n_out[k] = cnt[k];
}

}  // namespace dk
