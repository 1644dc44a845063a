// Stand-alone host program over dk_nest.h (the level-to-element rule the device kernels compile):
// reads cases of (rep, def) levels, runs the serial reference walk twice -- counting only, then into
// buffers of exactly the counted sizes (so a sanitizer sees any index past them) -- and prints n_k,
// offs_k, def_k and the classification of every parent. tests/test_nest_host.py compares the output
// with values written out by hand.
//
// Input, one case per block:
//   case <name> <R> <list_def[1]> .. <list_def[R]> <n>
//   <n rep levels>
//   <n def levels>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "dk_nest.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: nest_host CASES\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string word, name;
  while (in >> word) {
    if (word != "case") { fprintf(stderr, "bad input near '%s'\n", word.c_str()); return 2; }
    int R = 0;
    long n = 0;
    in >> name >> R;
    if (!in || R < 1 || R > dk::DK_NEST_MAX) { fprintf(stderr, "%s: bad R\n", name.c_str()); return 2; }
    int32_t list_def[dk::DK_NEST_MAX] = {0, 0, 0, 0};
    for (int k = 0; k < R; k++) in >> list_def[k];
    in >> n;
    if (!in || n < 0) { fprintf(stderr, "%s: bad header\n", name.c_str()); return 2; }
    std::vector<uint8_t> rep((size_t)n), def((size_t)n);
    for (long i = 0; i < n; i++) { int v; in >> v; rep[(size_t)i] = (uint8_t)v; }
    for (long i = 0; i < n; i++) { int v; in >> v; def[(size_t)i] = (uint8_t)v; }
    if (!in) { fprintf(stderr, "%s: short levels\n", name.c_str()); return 2; }
    int64_t cnt[dk::DK_NEST_MAX + 1] = {0, 0, 0, 0, 0};
    dk::nest_walk(rep.data(), def.data(), n, R, list_def, cnt, nullptr, nullptr);
    // exactly sized outputs: offs_k has n_{k-1} + 1 entries, def_k has n_k
    std::vector<std::vector<int64_t>> offs((size_t)R);
    std::vector<std::vector<uint8_t>> defs((size_t)R);
    int64_t* op[dk::DK_NEST_MAX] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t* dp[dk::DK_NEST_MAX] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < R; k++) {
      offs[(size_t)k].assign((size_t)cnt[k] + 1, -1);
      defs[(size_t)k].assign((size_t)cnt[k], 255);
      op[k] = offs[(size_t)k].data();
      dp[k] = defs[(size_t)k].data();
    }
    int64_t cnt2[dk::DK_NEST_MAX + 1] = {0, 0, 0, 0, 0};
    dk::nest_walk(rep.data(), def.data(), n, R, list_def, cnt2, op, dp);
    for (int k = 0; k <= R; k++)
      if (cnt[k] != cnt2[k]) { fprintf(stderr, "%s: the two walks disagree at depth %d\n", name.c_str(), k); return 1; }
    std::cout << "case " << name << "\nn:";
    for (int k = 0; k <= R; k++) std::cout << ' ' << cnt[k];
    std::cout << '\n';
    for (int k = 1; k <= R; k++) {
      std::cout << "offs" << k << ':';
      for (int64_t v : offs[(size_t)k - 1]) std::cout << ' ' << v;
      std::cout << "\ndef" << k - 1 << ':';
      for (uint8_t v : defs[(size_t)k - 1]) std::cout << ' ' << (int)v;
      std::cout << "\ncls" << k << ':';
      for (uint8_t v : defs[(size_t)k - 1]) std::cout << ' ' << dk::nest_classify(v, list_def[k - 1]);
      std::cout << '\n';
    }
  }
  return 0;
}
