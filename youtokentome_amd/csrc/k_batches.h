// k_batches.h -- batches by length under a token budget on the device: sentence lengths -> a stable order by length, the greedy cuts of that order
// into batches, and the batches of one side as padded matrices (the rule is in include/yttm_mi355x.h).  Included at the end of k_encode.hip like
// its siblings.
//
// The plan (all passes on one stream, no kernel waits for another workgroup, no global atomic per sentence):
//   k_bat_keys     key[i] = l(i) of a kept sentence, cap + 1 of a left-out one; the smallest index of a negative length or of a kept sentence
//                  longer than T by one atomicMin per workgroup, the kept sentences by one atomicAdd per workgroup (a sum: any order gives it)
//   k_bat_hist     per pass of 8 bits: a workgroup counts the digits of its tile of BAT_TILE sentences in LDS -> hist[digit][tile]
//                  -> launch_exclusive_scan -> where the tile's sentences of a digit start in the output
//   k_bat_scatter  the workgroup ranks its tile stably, 256 sentences a round: the lanes of a wavefront that hold the same digit are found by
//                  ballots over the digit's 8 bits, a lane's rank among them is the popcount of that mask below it, and the wavefronts take their
//                  turns in order through the tile's 256 LDS counters.  Where a sentence lands depends on the scan and on its place in the tile
//                  only, never on the order in which workgroups run.  The first pass takes the index from the position, the last writes order only.
//   k_bat_skey     skey[p] = key[order[p]] over the kept prefix: the lengths in sorted order, which the cuts search
//   k_bat_orbit    next(a) = the end of a batch that starts at position a, by binary search ((b - a) skey[b - 1] does not decrease in b); and per
//                  workgroup of `orbit` positions (BAT_ORBIT = 8192, eight a thread), by pointer doubling in LDS, every position's exit from
//                  its block and the batches on the way
//   k_bat_chain    one lane hops from block to block: the entry of every block the orbit of position 0 visits and the batches in front of it.
//                  Serial in n_kept / orbit, one dependent load a hop -- an eighth of the hops the training blocks' chain takes.
//   k_bat_walk     a workgroup per visited block copies the block's next() into LDS, and one lane walks from the entry to the exit there and
//                  writes batch_first[batches in front + k]
// The gather of one side:
//   k_bat_measure  a wavefront per batch: the longest sentence of this side -> widths[b], rows * width -> launch_exclusive_scan -> batch_off;
//                  the exact total by one atomicAdd per wavefront (the scan's counts saturate)
//   k_bat_write    the flat output in chunks of BAT_CHUNK elements, a wavefront per chunk in steps of 256 (64 lanes x 4 elements, one 16-byte
//                  store per lane).  The chunk's first batch comes from one binary search over batch_off; a lane whose elements lie behind that
//                  batch searches for its own.  (row, column) by division; four ids of one row are one load at a 4-byte aligned address.
// Algorithmic bytes: plan 4 S read, 4 S + 8 (B + 1) written; gather 4 K + 8 (S + 1) + 4 S + 8 (B + 1) read, 4 E + 4 B + 8 (B + 1) written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_blocks.h"
#include "yttm_device.h"
#include "yttm_kernels.h"

namespace yttm {

constexpr unsigned int BAT_ORBIT_THREADS = 1024;
constexpr unsigned int BAT_PER_THREAD = BAT_ORBIT / BAT_ORBIT_THREADS;  // positions of a block a thread of k_bat_orbit resolves
static_assert(BLOCK == 256, "a thread per digit in k_bat_hist and k_bat_scatter");

__global__ __launch_bounds__(BLOCK) void k_bat_keys(BatIn in, BatRule r, uint32_t *__restrict__ key, unsigned long long *__restrict__ info) {
  __shared__ unsigned long long s_bad[NWAVES], s_kept[NWAVES];
  unsigned long long bad = ~0ull, kept = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < in.n; i += (unsigned long long)gridDim.x * BLOCK) {
    uint32_t k = (uint32_t)(r.cap + 1);
    if (in.negative(i)) {
      if (i < bad) bad = i;
    } else {
      const unsigned long long l = in.l(i);
      if (l >= r.min_len && (r.max_len == 0 || l <= r.max_len)) {
        if (l > r.T) {
          if (i < bad) bad = i;
        } else {
          k = (uint32_t)l;
          kept++;
        }
      }
    }
    key[i] = k;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long b2 = __shfl_down(bad, o), k2 = __shfl_down(kept, o);
    if (b2 < bad) bad = b2;
    kept += k2;
  }
  if (lane_id() == 0) {
    s_bad[threadIdx.x >> 6] = bad;
    s_kept[threadIdx.x >> 6] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NWAVES; w++) {
      if (s_bad[w] < bad) bad = s_bad[w];
      kept += s_kept[w];
    }
    if (bad != ~0ull) atomicMin(info, bad);
    if (kept) atomicAdd(info + 1, kept);
  }
}

__global__ __launch_bounds__(BLOCK) void k_bat_hist(const uint32_t *__restrict__ key, unsigned long long n, unsigned int shift, unsigned long long tiles,
                                                    uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long t0 = (unsigned long long)blockIdx.x * BAT_TILE;
  for (unsigned int j = threadIdx.x; j < BAT_TILE && t0 + j < n; j += BLOCK) atomicAdd(&h[(key[t0 + j] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(unsigned long long)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(BLOCK) void k_bat_scatter(const uint32_t *__restrict__ key, const uint32_t *__restrict__ idx, unsigned long long n,
                                                       unsigned int shift, unsigned long long tiles, const unsigned long long *__restrict__ hist_off,
                                                       uint32_t *__restrict__ key_out, uint32_t *__restrict__ idx_out) {
  __shared__ uint32_t at[256];  // where the tile's next sentence of a digit goes (n < 2^32)
  const int w = uni((int)(threadIdx.x >> 6));
  at[threadIdx.x] = (uint32_t)hist_off[(unsigned long long)threadIdx.x * tiles + blockIdx.x];
  __syncthreads();
  const unsigned long long t0 = (unsigned long long)blockIdx.x * BAT_TILE;
  for (unsigned int j0 = 0; j0 < BAT_TILE && t0 + j0 < n; j0 += BLOCK) {
    const unsigned long long i = t0 + j0 + threadIdx.x;
    const bool active = i < n;
    const uint32_t k = active ? key[i] : 0u, d = (k >> shift) & 255u;
    unsigned long long same = ballot_b(active);  // the active lanes of this wavefront that hold digit d
    for (unsigned int bit = 0; bit < 8; bit++) {
      const bool one = (d >> bit) & 1u;
      const unsigned long long m = ballot_b(one);
      same &= one ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(same & lanemask_lt()), count = (uint32_t)__popcll(same);
    uint32_t to = 0;
    for (int turn = 0; turn < NWAVES; turn++) {
      if (turn == w) {
        if (active) to = at[d] + rank;
        wave_sync();
        if (active && rank == 0) at[d] += count;
      }
      __syncthreads();
    }
    if (active) {
      if (key_out) key_out[to] = k;
      idx_out[to] = idx ? idx[i] : (uint32_t)i;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_bat_skey(const uint32_t *__restrict__ key, const uint32_t *__restrict__ order, unsigned long long n_kept,
                                                    uint32_t *__restrict__ skey) {
  for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_kept; p += (unsigned long long)gridDim.x * BLOCK)
    skey[p] = key[order[p]];
}

// The end of the batch that starts at position a < n: the largest b of (a, min(n, a + M)] with (b - a) skey[b - 1] <= T.  b = a + 1 holds it: no
// kept sentence is longer than T.
__device__ inline unsigned long long bat_next(const uint32_t *__restrict__ skey, unsigned long long n, const BatRule &r, unsigned long long a) {
  unsigned long long lo = a + 1, hi = r.M && a + r.M < n ? a + r.M : n;
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo + 1) >> 1);
    if ((mid - a) * skey[mid - 1] <= r.T) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(BAT_ORBIT_THREADS) void k_bat_orbit(const uint32_t *__restrict__ skey, unsigned long long n, BatRule r, unsigned int orbit,
                                                                 uint32_t *__restrict__ nxt, unsigned long long *__restrict__ hop) {
  __shared__ uint32_t tgt[BAT_ORBIT];
  __shared__ uint16_t hops[BAT_ORBIT];  // (at most `orbit` batches start inside a block)
  const uint32_t t = threadIdx.x;
  const unsigned long long b0 = (unsigned long long)blockIdx.x * orbit, b1 = b0 + orbit;
  uint32_t to[BAT_PER_THREAD], h[BAT_PER_THREAD];
  for (unsigned int k = 0; k < BAT_PER_THREAD; k++) {
    const uint32_t j = t + k * BAT_ORBIT_THREADS;
    const unsigned long long i = b0 + j;
    to[k] = (uint32_t)n;
    h[k] = 0;
    if (j < orbit && i < n) {
      to[k] = (uint32_t)bat_next(skey, n, r, i);
      h[k] = 1;
      nxt[i] = to[k];
    }
    if (j < orbit) {
      tgt[j] = to[k];
      hops[j] = (uint16_t)h[k];
    }
  }
  __syncthreads();
  for (unsigned int reach = 1; reach < orbit; reach <<= 1) {  // after a round every entry is 2 reach hops on, or outside the block
    uint32_t t2[BAT_PER_THREAD], h2[BAT_PER_THREAD];
    bool inside[BAT_PER_THREAD];
    for (unsigned int k = 0; k < BAT_PER_THREAD; k++) {
      const uint32_t j = t + k * BAT_ORBIT_THREADS;
      inside[k] = j < orbit && to[k] < n && to[k] < b1;
      const uint32_t u = inside[k] ? (uint32_t)(to[k] - b0) : 0u;
      t2[k] = tgt[u];
      h2[k] = hops[u];
    }
    __syncthreads();
    for (unsigned int k = 0; k < BAT_PER_THREAD; k++) {
      const uint32_t j = t + k * BAT_ORBIT_THREADS;
      if (inside[k]) {
        to[k] = t2[k];
        h[k] += h2[k];
      }
      if (j < orbit) {
        tgt[j] = to[k];
        hops[j] = (uint16_t)h[k];
      }
    }
    __syncthreads();
  }
  for (unsigned int k = 0; k < BAT_PER_THREAD; k++) {
    const uint32_t j = t + k * BAT_ORBIT_THREADS;
    if (j < orbit && b0 + j < n) hop[b0 + j] = to[k] | ((unsigned long long)h[k] << 32);
  }
}

// entry[] holds BAT_NONE before the launch.  info[2] = the batches of the orbit of position 0.
__global__ void k_bat_chain(const unsigned long long *__restrict__ hop, unsigned long long n, unsigned int orbit, uint32_t *__restrict__ entry,
                            uint32_t *__restrict__ base, unsigned long long *__restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned long long cur = 0, batches = 0;
  while (cur < n) {
    const unsigned long long blk = cur / orbit;  // (a block a batch jumps over is never entered)
    entry[blk] = (uint32_t)cur;
    base[blk] = (uint32_t)batches;
    const unsigned long long h = hop[cur];
    batches += h >> 32;
    cur = h & 0xffffffffull;
  }
  info[2] = batches;
}

__global__ __launch_bounds__(BLOCK) void k_bat_walk(const uint32_t *__restrict__ nxt, unsigned long long n, unsigned int orbit, const uint32_t *__restrict__ entry,
                                                    const uint32_t *__restrict__ base, unsigned long long *__restrict__ batch_first) {
  __shared__ uint32_t nx[BAT_ORBIT];
  const uint32_t e = entry[blockIdx.x];
  if (e == BAT_NONE) return;  // (the whole workgroup)
  const unsigned long long b0 = (unsigned long long)blockIdx.x * orbit, end = b0 + orbit < n ? b0 + orbit : n;
  for (unsigned int j = threadIdx.x; b0 + j < end; j += BLOCK) nx[j] = nxt[b0 + j];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long cur = e, k = base[blockIdx.x];
  while (cur < end) {
    batch_first[k++] = cur;
    cur = nx[cur - b0];
  }
  if (cur >= n) batch_first[k] = n;
}

// ---- the gather ----
__global__ __launch_bounds__(BLOCK) void k_bat_measure(BatPlan p, const unsigned long long *__restrict__ off, uint32_t *__restrict__ widths,
                                                       uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total) {
  const unsigned long long lane = (unsigned long long)lane_id();
  unsigned long long sum = 0;
  for (unsigned long long b = (unsigned long long)blockIdx.x * NWAVES + (threadIdx.x >> 6); b < p.n_batches; b += (unsigned long long)gridDim.x * NWAVES) {
    const unsigned long long a = p.batch_first[b], e = p.batch_first[b + 1];
    unsigned long long m = 0;
    for (unsigned long long q = a + lane; q < e; q += 64) {
      const unsigned long long s = p.order[q], l = off[s + 1] - off[s];
      if (l > m) m = l;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long m2 = __shfl_down(m, o);
      if (m2 > m) m = m2;
    }
    if (lane == 0) {  // (a width or a product beyond 32 bits saturates: the call is refused by the exact total)
      const unsigned long long wd = m < 0xffffffffull ? m : 0xffffffffull, prod = (e - a) * wd;
      widths[b] = (uint32_t)wd;
      cnt[b] = (uint32_t)(prod < 0xffffffffull ? prod : 0xffffffffull);
      sum += prod < 0xffffffffull ? prod : 0xffffffffull;
    }
  }
  if (lane == 0 && sum) atomicAdd(total, sum);
}

struct BatOut {
  BatPlan p;
  const int32_t *ids;
  const unsigned long long *off;
  const uint32_t *widths;
  const unsigned long long *batch_off;
  unsigned long long n_elems;
  int32_t pad;
  bool left;
};

// the batch that holds element e < n_elems: the largest b with batch_off[b] <= e (a batch without elements holds none)
__device__ inline unsigned long long bat_batch_of(const BatOut &o, unsigned long long e) {
  unsigned long long lo = 0, hi = o.p.n_batches;
  while (hi - lo > 1) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    if (o.batch_off[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct BatRow {  // a row of a batch: where its ids are and which columns hold them
  unsigned long long src;
  uint32_t c0, c1;  // the ids sit in columns [c0, c1)
};
__device__ inline BatRow bat_row(const BatOut &o, unsigned long long first, uint32_t row, uint32_t width) {
  const unsigned long long s = o.p.order[first + row], a = o.off[s];
  const uint32_t len = (uint32_t)(o.off[s + 1] - a), c0 = o.left ? width - len : 0u;
  return BatRow{a, c0, c0 + len};
}

__global__ __launch_bounds__(BLOCK) void k_bat_write(BatOut o, int32_t *__restrict__ out) {
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long c0 = ((unsigned long long)blockIdx.x * NWAVES + (unsigned long long)w) * BAT_CHUNK;
  if (c0 >= o.n_elems) return;
  const unsigned long long c1 = c0 + BAT_CHUNK < o.n_elems ? c0 + BAT_CHUNK : o.n_elems;
  unsigned long long hint = bat_batch_of(o, c0);
  for (unsigned long long bs = c0; bs < c1; bs += 256) {
    const unsigned long long e0 = bs + 4 * lane;
    const bool active = e0 < o.n_elems;
    unsigned long long b = hint;
    if (active) {
      if (o.batch_off[b] > e0 || e0 >= o.batch_off[b + 1]) b = bat_batch_of(o, e0);
      unsigned long long base = o.batch_off[b], first = o.p.batch_first[b];
      uint32_t width = o.widths[b], rows = (uint32_t)(o.p.batch_first[b + 1] - first);
      uint32_t row = (uint32_t)(e0 - base) / width, col = (uint32_t)(e0 - base) - row * width;
      BatRow R = bat_row(o, first, row, width);
      int32_t v[4];
      if (col + 3 < width) {  // four elements of one row
        if (col >= R.c0 && col + 3 < R.c1) {
          const BlkQuad q = *reinterpret_cast<const BlkQuad *>(o.ids + (R.src + (col - R.c0)));
          for (int k = 0; k < 4; k++) v[k] = q.v[k];
        } else {
          for (uint32_t k = 0; k < 4; k++) v[k] = col + k >= R.c0 && col + k < R.c1 ? o.ids[R.src + (col + k - R.c0)] : o.pad;
        }
      } else {
        for (uint32_t k = 0; k < 4; k++) {
          if (e0 + k >= o.n_elems) {
            v[k] = o.pad;  // (behind the output: the array's own slack)
            continue;
          }
          if (col == width) {  // the next row, or the next batch that holds an element
            col = 0;
            if (++row == rows) {
              b = bat_batch_of(o, e0 + k);
              base = o.batch_off[b];
              first = o.p.batch_first[b];
              width = o.widths[b];
              rows = (uint32_t)(o.p.batch_first[b + 1] - first);
              row = 0;
            }
            R = bat_row(o, first, row, width);
          }
          v[k] = col >= R.c0 && col < R.c1 ? o.ids[R.src + (col - R.c0)] : o.pad;
          col++;
        }
      }
      *reinterpret_cast<uint4 *>(out + e0) = make_uint4((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
    }
    hint = __shfl(b, 63);  // (lane 63's last batch is the nearest to the next step; an idle lane hands the old hint on)
  }
}

unsigned int bat_orbit_positions() {
  const unsigned long long u = cfg()->batches_orbit.u & ~63ull;
  return (unsigned int)(u < 64 ? 64 : u > BAT_ORBIT ? BAT_ORBIT : u);
}
void launch_bat_keys(const BatIn &in, const BatRule &r, uint32_t *key, unsigned long long *info, hipStream_t st) {
  hipLaunchKernelGGL(k_bat_keys, dim3(blk_grid(in.n, BLOCK)), dim3(BLOCK), 0, st, in, r, key, info);
}
void launch_bat_sort_pass(const uint32_t *key_in, const uint32_t *idx_in, unsigned long long n, unsigned int shift, uint32_t *hist,
                          unsigned long long *hist_off, unsigned long long *scan_tmp, unsigned long long *scan_total, uint32_t *key_out,
                          uint32_t *idx_out, hipStream_t st) {
  const unsigned long long tiles = bat_tiles(n);
  hipLaunchKernelGGL(k_bat_hist, dim3((unsigned int)tiles), dim3(BLOCK), 0, st, key_in, n, shift, tiles, hist);
  launch_exclusive_scan(hist, 256 * tiles, hist_off, scan_tmp, scan_total, st);
  hipLaunchKernelGGL(k_bat_scatter, dim3((unsigned int)tiles), dim3(BLOCK), 0, st, key_in, idx_in, n, shift, tiles, hist_off, key_out, idx_out);
}
void launch_bat_cuts(const uint32_t *key, const uint32_t *order, unsigned long long n_kept, const BatRule &r, unsigned int orbit, uint32_t *skey,
                     uint32_t *nxt, unsigned long long *hop, uint32_t *entry, uint32_t *base, unsigned long long *batch_first,
                     unsigned long long *info, hipStream_t st) {
  const unsigned long long n_blocks = (n_kept + orbit - 1) / orbit;
  hipLaunchKernelGGL(k_bat_skey, dim3(blk_grid(n_kept, BLOCK)), dim3(BLOCK), 0, st, key, order, n_kept, skey);
  hipLaunchKernelGGL(k_bat_orbit, dim3((unsigned int)n_blocks), dim3(BAT_ORBIT_THREADS), 0, st, skey, n_kept, r, orbit, nxt, hop);
  hipLaunchKernelGGL(k_bat_chain, dim3(1), dim3(64), 0, st, hop, n_kept, orbit, entry, base, info);
  hipLaunchKernelGGL(k_bat_walk, dim3((unsigned int)n_blocks), dim3(BLOCK), 0, st, nxt, n_kept, orbit, entry, base, batch_first);
}
void launch_bat_measure(const BatPlan &p, const unsigned long long *off, uint32_t *widths, uint32_t *cnt, unsigned long long *total, hipStream_t st) {
  hipLaunchKernelGGL(k_bat_measure, dim3(blk_grid(p.n_batches, NWAVES)), dim3(BLOCK), 0, st, p, off, widths, cnt, total);
}
void launch_bat_write(const BatPlan &p, const int32_t *ids, const unsigned long long *off, const uint32_t *widths,
                      const unsigned long long *batch_off, unsigned long long n_elems, int32_t pad, bool left_pad, int32_t *out, hipStream_t st) {
  const BatOut o{p, ids, off, widths, batch_off, n_elems, pad, left_pad};
  const unsigned long long waves = (n_elems + BAT_CHUNK - 1) / BAT_CHUNK;
  hipLaunchKernelGGL(k_bat_write, dim3((unsigned int)((waves + NWAVES - 1) / NWAVES)), dim3(BLOCK), 0, st, o, out);
}

}  // namespace yttm
