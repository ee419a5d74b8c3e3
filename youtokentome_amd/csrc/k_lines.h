// k_lines.h -- the lines of a text in HBM (bytes -> uint64 offsets[n_lines + 1]), the way in of the batch encoder for a file or a byte buffer.
// Included at the end of k_encode.hip.
//
// replaces: std::getline over the input, as LineReader restates it (host_cli.cpp), for a whole text at once.  A line ends at the byte 0x0A; a last
// line without one counts; nothing follows a final newline; "\r" is an ordinary byte.  Line i is text[off[i] .. off[i + 1]) WITH its newline (a
// space to the encoder: cp_is_space(10)), off[0] = 0, off[n_lines] = n.
//
// So a line starts at 0 and behind every newline except one in the text's last byte: the kernels look for newlines in text[0 .. n - 1) only.
// Three steps on the lane's stream, each behind a launch boundary:
//   count   k_lines<false>: cnt[t] = newlines in tile t (a tile: LN_TILE bytes; one store per tile, no atomic)
//   scan    launch_exclusive_scan(cnt) -> rank[t]                                                                    (k_frontend.hip)
//   write   k_lines<true>: off[1 + rank[t] + k] = (position of the tile's k-th newline) + 1; off[0] and off[n_lines] by workgroup 0
// and the longest line from the written offsets (k_lines_longest: one 64-bit atomicMax per workgroup), which also covers lines that span tiles.
// Algorithmic bytes: N read by the count pass (the write pass reads them again, mostly from L2 misses: 2 N of traffic) + 8 (n_lines + 1) written.
//
// Mapping: tiles are cut in the ALIGNED coordinate q = p + (address of text & 15), so every 16-byte unit of a tile is aligned whatever the
// text's address; a lane loads LN_UNITS units per tile, unit j * BLOCK + thread (coalesced, all four loads issued before the first use: 16 KB
// in flight per workgroup).  Only the text's first and last unit can be partial; tiles that hold one read those units byte by byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yttm_device.h"
#include "yttm_kernels.h"

namespace yttm {

constexpr int LN_UNITS = 4;                      // 16-byte units per lane and tile
constexpr int LN_TILE = BLOCK * 16 * LN_UNITS;   // bytes per tile

// bit 7 of every byte of w that is 0x0A
__device__ inline uint32_t ln_nl_bits(uint32_t w) {
  const uint32_t y = w ^ 0x0a0a0a0au;
  return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
}
// ... as bits 0..3 in byte order
__device__ inline uint32_t ln_nl_nibble(uint32_t w) { return (((ln_nl_bits(w) >> 7) * 0x00204081u) >> 21) & 0xfu; }
__device__ inline uint32_t ln_unit_mask(const uint4 &v) {
  return ln_nl_nibble(v.x) | (ln_nl_nibble(v.y) << 4) | (ln_nl_nibble(v.z) << 8) | (ln_nl_nibble(v.w) << 12);
}
__device__ inline uint32_t ln_unit_count(const uint4 &v) {
  return (uint32_t)(__popc(ln_nl_bits(v.x)) + __popc(ln_nl_bits(v.y)) + __popc(ln_nl_bits(v.z)) + __popc(ln_nl_bits(v.w)));
}
// a unit at the text's edge: only the bytes with lo <= q < hi are read
__device__ inline uint32_t ln_edge_mask(const uint8_t *abase, unsigned long long q0, unsigned long long lo, unsigned long long hi) {
  uint32_t m = 0;
  for (uint32_t b = 0; b < 16; b++) {
    const unsigned long long q = q0 + b;
    if (q >= lo && q < hi && abase[q] == (uint8_t)0x0a) m |= 1u << b;
  }
  return m;
}

// abase: the text's address rounded down to 16 bytes; the bytes searched are abase[lo .. hi) (lo < 16).
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_lines(const uint8_t *__restrict__ abase, unsigned long long lo, unsigned long long hi,
                                                 unsigned long long n_tiles, uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ rank,
                                                 unsigned long long *__restrict__ off, unsigned long long n_lines, unsigned long long n_bytes) {
  __shared__ uint32_t s_w[LN_UNITS][NWAVES];
  const int w = (int)(threadIdx.x >> 6);
  const uint32_t lane = (uint32_t)lane_id();
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) {
    off[0] = 0;
    off[n_lines] = n_bytes;
  }
  for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const unsigned long long t0 = t * (unsigned long long)LN_TILE;
    const bool inner = t0 >= lo && t0 + (unsigned long long)LN_TILE <= hi;  // (uniform) no unit of the tile reaches outside the text
    uint32_t m[LN_UNITS];
    if (inner) {
      uint4 v[LN_UNITS];
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) v[j] = *reinterpret_cast<const uint4 *>(abase + t0 + 16ull * ((unsigned long long)j * BLOCK + threadIdx.x));
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) m[j] = WRITE ? ln_unit_mask(v[j]) : ln_unit_count(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) {
        const unsigned long long q0 = t0 + 16ull * ((unsigned long long)j * BLOCK + threadIdx.x);
        uint32_t mk = 0;
        if (q0 < hi && q0 + 16 > lo) {
          if (q0 >= lo && q0 + 16 <= hi) mk = ln_unit_mask(*reinterpret_cast<const uint4 *>(abase + q0));
          else mk = ln_edge_mask(abase, q0, lo, hi);
        }
        m[j] = WRITE ? mk : (uint32_t)__popc(mk);
      }
    }
    if (!WRITE) {
      uint32_t c = 0;
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) c += m[j];
      for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
      if (lane == 0) s_w[0][w] = c;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < NWAVES; k++) s += s_w[0][k];
        cnt[t] = s;
      }
      __syncthreads();
    } else {
      // ranks in position order: unit j * BLOCK + thread, so row j of wave k comes behind every row < j and behind the waves < k of row j
      uint32_t x[LN_UNITS];
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) {
        const uint32_t c = (uint32_t)__popc(m[j]);
        const uint32_t inc = wave_incl_scan(c);
        x[j] = inc - c;
        if (lane == 63) s_w[j][w] = inc;
      }
      __syncthreads();
      unsigned long long r = rank[t] + 1;  // (+ 1: off[0] is the first line's start)
#pragma unroll
      for (int j = 0; j < LN_UNITS; j++) {
        uint32_t before = x[j];
        for (int k = 0; k < NWAVES; k++) {
          const uint32_t s = s_w[j][k];
          if (k < w) before += s;
        }
        const unsigned long long q0 = t0 + 16ull * ((unsigned long long)j * BLOCK + threadIdx.x);
        unsigned long long at = r + before;
        for (uint32_t mk = m[j]; mk; mk &= mk - 1) off[at++] = q0 + (unsigned long long)(__ffs((int)mk) - 1) + 1 - lo;
        for (int k = 0; k < NWAVES; k++) r += s_w[j][k];
      }
      __syncthreads();
    }
  }
}

// longest line of off[0 .. n_lines]: one atomicMax per workgroup.  Reads 8 (n_lines + 1) bytes.
__global__ __launch_bounds__(BLOCK) void k_lines_longest(const unsigned long long *__restrict__ off, unsigned long long n_lines, unsigned long long *longest) {
  __shared__ unsigned long long s_m[NWAVES];
  unsigned long long m = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; s < n_lines; s += (unsigned long long)gridDim.x * BLOCK) {
    const unsigned long long l = off[s + 1] - off[s];
    m = l > m ? l : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_down(m, o);
    m = t > m ? t : m;
  }
  if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NWAVES; i++) m = s_m[i] > m ? s_m[i] : m;
    if (m) atomicMax(longest, m);
  }
}

static unsigned int lines_grid(unsigned long long n_tiles) {
  const unsigned long long cap = 256ull * 16;
  return (unsigned int)(n_tiles < 1 ? 1 : n_tiles > cap ? cap : n_tiles);
}
unsigned long long lines_tiles(const void *d_text, unsigned long long n_bytes) {
  if (n_bytes < 2) return 0;
  const unsigned long long lo = (unsigned long long)((uintptr_t)d_text & 15u);
  return (lo + n_bytes - 1 + LN_TILE - 1) / LN_TILE;
}
void launch_lines_count(const uint8_t *d_text, unsigned long long n_bytes, uint32_t *cnt, hipStream_t st) {
  const unsigned long long n_tiles = lines_tiles(d_text, n_bytes);
  if (!n_tiles) return;
  const unsigned long long lo = (unsigned long long)((uintptr_t)d_text & 15u);
  hipLaunchKernelGGL((k_lines<false>), dim3(lines_grid(n_tiles)), dim3(BLOCK), 0, st, d_text - lo, lo, lo + n_bytes - 1, n_tiles, cnt, nullptr, nullptr, 0ull, 0ull);
}
void launch_lines_write(const uint8_t *d_text, unsigned long long n_bytes, const unsigned long long *rank, unsigned long long *off, unsigned long long n_lines,
                        hipStream_t st) {
  if (!n_bytes) return;
  const unsigned long long n_tiles = lines_tiles(d_text, n_bytes);
  const unsigned long long lo = (unsigned long long)((uintptr_t)d_text & 15u);
  hipLaunchKernelGGL((k_lines<true>), dim3(lines_grid(n_tiles)), dim3(BLOCK), 0, st, d_text - lo, lo, lo + n_bytes - 1, n_tiles, nullptr, rank, off, n_lines, n_bytes);
}
void launch_lines_longest(const unsigned long long *off, unsigned long long n_lines, unsigned long long *longest, hipStream_t st) {
  if (!n_lines) return;
  unsigned long long b = (n_lines + BLOCK - 1) / BLOCK;
  if (b > 256 * 8) b = 256 * 8;
  hipLaunchKernelGGL(k_lines_longest, dim3((unsigned int)b), dim3(BLOCK), 0, st, off, n_lines, longest);
}

}  // namespace yttm
