// idcount_plan.h -- the launch arithmetic of k_idcount (k_idcount.h): which built window, how many workgroups, how many ids to a launch.
// Plain C++ without HIP, so that tools/dbg/check_idcount_plan.cpp can walk it over its whole input range under the host sanitizers.
#pragma once
#include <stdint.h>

#include "yttm_config.h"

namespace yttm {

constexpr int IDC_BLOCK = 1024;  // 16 wavefronts: the largest window leaves room for one workgroup per CU, which must hide the loads' latency alone
constexpr int IDC_WAVES = IDC_BLOCK / 64;
constexpr int IDC_UNITS_PER_WAVE = 128;  // 16-byte units a wavefront takes per step: two per lane, both loaded before the first is counted
// The windows the kernel is built with and the workgroups per CU their LDS leaves room for (160 KiB per CU): 16 KiB x 2 (capped by the 2048
// threads of a CU), 64 KiB x 2, 128 KiB x 1.
constexpr int IDC_BUILDS = 3;
constexpr uint32_t IDC_WINDOW[IDC_BUILDS] = {4096, 16384, YTTM_IDCOUNT_WINDOW_BUILT};
constexpr unsigned int IDC_PER_CU[IDC_BUILDS] = {2, 2, 1};
constexpr unsigned int IDC_CUS = 256;
static_assert(IDC_WINDOW[0] < IDC_WINDOW[1] && IDC_WINDOW[1] < IDC_WINDOW[2], "the builds are in the order of their windows");
static_assert((unsigned long long)IDC_WINDOW[2] * 4 * IDC_PER_CU[2] <= 160ull * 1024 && (unsigned long long)IDC_WINDOW[1] * 4 * IDC_PER_CU[1] <= 160ull * 1024,
              "the workgroups of a CU fit its LDS");
// Ids of ONE launch.  A uint32 LDS bin counts ids of its own workgroup's share of one launch and is flushed at the launch's end, and the lanes'
// out-of-range tallies are uint32 too: a launch of at most 2^31 ids can wrap neither, whatever the grid.  launch_idcount cuts a longer array
// into launches of this many ids.
constexpr unsigned long long IDC_LAUNCH_MAX = 1ull << 31;
static_assert(IDC_LAUNCH_MAX < (1ull << 32), "a bin of one launch stays below 2^32");
static inline unsigned long long idcount_launch_ids(unsigned long long left) { return left < IDC_LAUNCH_MAX ? left : IDC_LAUNCH_MAX; }  // of the ids still to count
constexpr uint32_t IDC_BINS_MAX = 1u << 31;  // ids are int32: no bin above this one can be hit

struct IdcPlan {
  uint32_t window;    // bins in LDS: min(hook, n_bins, the largest built window)
  int build;          // index into IDC_WINDOW: the smallest build that holds `window`
  unsigned int grid;  // workgroups: a step's worth of units each at least, at most what the CUs hold at once
};
// n_ids: of one launch, within [1, IDC_LAUNCH_MAX]; n_bins within [1, IDC_BINS_MAX]; hook: any value
static inline IdcPlan idcount_plan(unsigned long long n_ids, unsigned long long n_bins, unsigned long long hook) {
  IdcPlan p;
  unsigned long long w = hook < n_bins ? hook : n_bins;
  if (w > IDC_WINDOW[IDC_BUILDS - 1]) w = IDC_WINDOW[IDC_BUILDS - 1];
  p.window = (uint32_t)w;
  p.build = 0;
  while (IDC_WINDOW[p.build] < p.window) p.build++;
  const unsigned long long units = n_ids / 4 + 1, per_block = (unsigned long long)IDC_WAVES * IDC_UNITS_PER_WAVE,
                           blocks = (units + per_block - 1) / per_block, cap = (unsigned long long)IDC_CUS * IDC_PER_CU[p.build];
  p.grid = (unsigned int)(blocks > cap ? cap : blocks);
  return p;
}

}  // namespace yttm
