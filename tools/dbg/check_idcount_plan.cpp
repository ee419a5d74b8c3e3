// tools/dbg/check_idcount_plan.cpp -- walks the launch arithmetic of k_idcount (youtokentome_amd/csrc/idcount_plan.h) over its whole input
// range on the host, under the sanitizers (needs no GPU):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iyoutokentome_amd/csrc tools/dbg/check_idcount_plan.cpp -o /tmp/check_idcount_plan
//   /tmp/check_idcount_plan
// For every (n_ids, n_bins, hook) of a grid that holds every power of two and its neighbours up to the ends of the ranges, and the builds'
// windows and their neighbours: the window is min(hook, n_bins, largest build), the build is the smallest that holds it, the grid lies within
// [1, CUs x workgroups per CU] and covers the units or is capped; and the cut of an array of any length into launches covers every id once
// with at most IDC_LAUNCH_MAX ids to a launch, so that no uint32 bin or tally of a launch can reach 2^32.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "idcount_plan.h"

using namespace yttm;

static unsigned long long checked = 0;
#define CHECK(c)                                                                                                            \
  do {                                                                                                                      \
    if (!(c)) {                                                                                                             \
      fprintf(stderr, "FAILED %s at n_ids %llu n_bins %llu hook %llu (line %d)\n", #c, n_ids, n_bins, hook, __LINE__); \
      exit(1);                                                                                                              \
    }                                                                                                                       \
    checked++;                                                                                                              \
  } while (0)

static std::vector<unsigned long long> edges(unsigned long long lo, unsigned long long hi) {
  std::set<unsigned long long> s{lo, hi};
  for (int b = 0; b < 64; b++)
    for (long long d = -2; d <= 2; d++) {
      const unsigned long long v = (1ull << b) + (unsigned long long)d;
      if (v >= lo && v <= hi) s.insert(v);
    }
  for (int k = 0; k < IDC_BUILDS; k++)
    for (long long d = -1; d <= 1; d++) {
      const unsigned long long v = IDC_WINDOW[k] + (unsigned long long)d;
      if (v >= lo && v <= hi) s.insert(v);
    }
  for (unsigned long long v : {600ull, 32000ull, 40000ull, 100000ull, 381144006ull})
    if (v >= lo && v <= hi) s.insert(v);
  return std::vector<unsigned long long>(s.begin(), s.end());
}

int main() {
  const std::vector<unsigned long long> ids = edges(1, IDC_LAUNCH_MAX), bins = edges(1, IDC_BINS_MAX), hooks = edges(0, ~0ull);
  for (unsigned long long n_ids : ids)
    for (unsigned long long n_bins : bins)
      for (unsigned long long hook : hooks) {
        const IdcPlan p = idcount_plan(n_ids, n_bins, hook);
        unsigned long long w = hook < n_bins ? hook : n_bins;
        if (w > IDC_WINDOW[IDC_BUILDS - 1]) w = IDC_WINDOW[IDC_BUILDS - 1];
        CHECK(p.window == w);
        CHECK(p.build >= 0 && p.build < IDC_BUILDS);
        CHECK(IDC_WINDOW[p.build] >= p.window);
        CHECK(p.build == 0 || IDC_WINDOW[p.build - 1] < p.window);
        const unsigned long long cap = (unsigned long long)IDC_CUS * IDC_PER_CU[p.build];
        CHECK(p.grid >= 1 && p.grid <= cap);
        const unsigned long long units = n_ids / 4 + 1, per_block = (unsigned long long)IDC_WAVES * IDC_UNITS_PER_WAVE;
        CHECK(p.grid == cap || (unsigned long long)p.grid * per_block >= units);  // one step covers the array, or the grid is full
        CHECK(p.grid == 1 || (unsigned long long)(p.grid - 1) * per_block < units);  // ... and no workgroup is launched for nothing
        CHECK((unsigned long long)p.window * 4 * IDC_PER_CU[p.build] <= 160ull * 1024);
      }
  // the cut into launches (launch_idcount's loop), for lengths up to 2^64 - 1
  const unsigned long long n_bins = 600, hook = 0;
  for (unsigned long long n_ids : edges(0, ~0ull)) {
    unsigned long long covered = 0, launches = 0;
    for (unsigned long long left = n_ids, n; left; left -= n) {
      n = idcount_launch_ids(left);
      CHECK(n >= 1 && n <= left && n <= IDC_LAUNCH_MAX && n < (1ull << 32));
      CHECK(n_ids - left == covered);  // (where the launch starts)
      covered += n;
      if (++launches == 64 && left > 128 * IDC_LAUNCH_MAX) {  // (up to 2^33 launches, the middle ones all alike: a whole number of them at once)
        const unsigned long long skip = (left - n) / IDC_LAUNCH_MAX - 64;
        left -= skip * IDC_LAUNCH_MAX;
        covered += skip * IDC_LAUNCH_MAX;
      }
    }
    CHECK(covered == n_ids);
  }
  printf("idcount_plan: %llu checks passed (%zu x %zu x %zu plans)\n", checked, ids.size(), bins.size(), hooks.size());
  return 0;
}
