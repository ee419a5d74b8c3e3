// k_idcount.h -- token frequencies on the device: int32 ids[n_ids] -> uint64 counts[n_bins + 1], counts[v] the ids equal to v, counts[n_bins] the
// ids outside [0, n_bins) (the rule is in include/yttm_mi355x.h).  Included at the end of k_encode.hip like its siblings.
//
// A skewed histogram: BPE ids are handed out in merge order, so the low ids take nearly all the traffic.  A workgroup keeps uint32 bins for the
// ids [0, window) in LDS, zeroed before and added to the global array -- the non-zero ones -- behind its share of the launch; ids of
// [window, n_bins) go to the global uint64 array by atomics, the out-of-range ids to a register tally per lane that a wavefront sums and adds
// once.  Integer sums: the result is exact in any order.
// Hot bins: 64 lanes adding to one LDS address serialise, so the first IDC_COMBINE distinct ids of a wavefront's step are added once each, by
// their first lane, with the number of lanes that hold them (a ballot on that lane's id and a popcount); what is left adds 1 per lane.  All lanes
// equal: one add per step instead of 64.
// The ids' address is only 4-byte aligned: the body is read in aligned 16-byte units, the up to three ids in front of the first unit and behind
// the last one by the first wavefront, a lane each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "idcount_plan.h"
#include "yttm_device.h"
#include "yttm_kernels.h"

namespace yttm {

constexpr int IDC_COMBINE = 2;

struct IdcWave {  // what the lanes of a wavefront count into
  uint32_t *bins;
  unsigned long long *counts;
  uint32_t n_bins, window;
  int lane;
  uint32_t outside;  // this lane's ids outside [0, n_bins)
  __device__ void add(uint32_t v, uint32_t c) {
    if (v < window) atomicAdd(&bins[v], c);
    else atomicAdd(&counts[v], (unsigned long long)c);
  }
  // one id per lane (have: the lane holds one); every lane of the wavefront calls it
  __device__ void count(uint32_t v, bool have) {
    bool pend = have && v < n_bins;  // (unsigned: a negative id is outside)
    outside += (have && !pend) ? 1u : 0u;
    for (int r = 0; r < IDC_COMBINE; r++) {
      const unsigned long long open = ballot_b(pend);
      if (!open) return;
      const int first = __ffsll((long long)open) - 1;
      const uint32_t hot = (uint32_t)__builtin_amdgcn_readlane((int)v, first);
      const bool mine = pend && v == hot;
      const unsigned long long same = ballot_b(mine);
      if (lane == first) add(hot, (uint32_t)__popcll(same));
      pend = pend && !mine;
    }
    if (pend) add(v, 1u);
  }
};

template <int W>
__global__ __launch_bounds__(IDC_BLOCK) void k_idcount(const int32_t *__restrict__ ids, unsigned long long n_ids, uint32_t n_bins, uint32_t window,
                                                       unsigned long long *__restrict__ counts) {
  __shared__ uint32_t bins[W];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < window; i += IDC_BLOCK) bins[i] = 0;
  __syncthreads();
  IdcWave w{bins, counts, n_bins, window, lane_id(), 0u};
  // ids[0 .. head) in front of the first aligned unit, `units` units, ids[tail0 .. n_ids) behind the last
  unsigned long long head = ((16u - (unsigned int)((uintptr_t)ids & 15u)) & 15u) >> 2;
  if (head > n_ids) head = n_ids;
  const unsigned long long units = (n_ids - head) >> 2, tail0 = head + 4 * units;
  const uint4 *body = reinterpret_cast<const uint4 *>(ids + head);
  const unsigned long long wave = (unsigned long long)blockIdx.x * IDC_WAVES + (tid >> 6), n_waves = (unsigned long long)gridDim.x * IDC_WAVES;
  for (unsigned long long base = wave * IDC_UNITS_PER_WAVE; base < units; base += n_waves * IDC_UNITS_PER_WAVE) {
    const unsigned long long u0 = base + (unsigned long long)w.lane, u1 = u0 + 64;
    const bool h0 = u0 < units, h1 = u1 < units;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const uint4 a = h0 ? body[u0] : zero, b = h1 ? body[u1] : zero;
    w.count(a.x, h0);
    w.count(a.y, h0);
    w.count(a.z, h0);
    w.count(a.w, h0);
    w.count(b.x, h1);
    w.count(b.y, h1);
    w.count(b.z, h1);
    w.count(b.w, h1);
  }
  if (wave == 0) {  // the peeled head in lanes 0 .. 2, the tail in lanes 4 .. 6
    const unsigned long long l = (unsigned long long)w.lane;
    const bool hv = l < head, tv = l >= 4 && l < 8 && tail0 + (l - 4) < n_ids;
    const int32_t v = hv ? ids[l] : tv ? ids[tail0 + (l - 4)] : 0;
    w.count((uint32_t)v, hv || tv);
  }
  uint32_t outside = w.outside;  // (below 2^31 for the whole launch: idcount_plan.h)
  for (int o = 32; o > 0; o >>= 1) outside += __shfl_down(outside, o);
  if (w.lane == 0 && outside) atomicAdd(&counts[n_bins], (unsigned long long)outside);
  __syncthreads();
  for (uint32_t i = tid; i < window; i += IDC_BLOCK) {
    const uint32_t c = bins[i];
    if (c) atomicAdd(&counts[i], (unsigned long long)c);
  }
}

// counts[n_bins + 1] += the histogram of ids[n_ids] (any 4-byte aligned address); 1 <= n_bins <= IDC_BINS_MAX.  The window is the hook's
// (YTTM_IDCOUNT_WINDOW), clamped to n_bins and to the largest build; a launch takes at most IDC_LAUNCH_MAX ids, so that no uint32 bin can wrap.
void launch_idcount(const int32_t *ids, unsigned long long n_ids, unsigned long long n_bins, unsigned long long *counts, hipStream_t st) {
  const unsigned long long hook = cfg()->idcount_window.u;
  for (unsigned long long left = n_ids, n; left; left -= n) {
    n = idcount_launch_ids(left);
    const IdcPlan p = idcount_plan(n, n_bins, hook);
    const dim3 grid(p.grid), block(IDC_BLOCK);
    const int32_t *from = ids + (n_ids - left);
    if (p.build == 0) hipLaunchKernelGGL((k_idcount<(int)IDC_WINDOW[0]>), grid, block, 0, st, from, n, (uint32_t)n_bins, p.window, counts);
    else if (p.build == 1) hipLaunchKernelGGL((k_idcount<(int)IDC_WINDOW[1]>), grid, block, 0, st, from, n, (uint32_t)n_bins, p.window, counts);
    else hipLaunchKernelGGL((k_idcount<(int)IDC_WINDOW[2]>), grid, block, 0, st, from, n, (uint32_t)n_bins, p.window, counts);
  }
}

}  // namespace yttm
