// k_blocks.h -- training blocks on the device: sentences of ids -> rows of exactly L ids with segment numbers, positions and the list of
// fragments (the rule is in include/yttm_mi355x.h).  Included at the end of k_encode.hip like its siblings.
//
// The sequence a call packs is the encoder's open row followed by the call's sentences (BlkIn): sentence i starts at voff(i) of one virtual
// stream of `total` ids.  Every row r takes a contiguous piece of that stream, [rowsrc[r], rowsrc[r + 1]), to its first columns; what is left of
// the row is padding.  Stream mode: rowsrc[r] = r L.  Whole mode: rowsrc[r] = voff(rowsent[r]), rowsent the orbit of sentence 0 under
//   next(i) = the last j with voff(j) <= voff(i) + L        (the first sentence that does not fit a row starting at i; a binary search per i).
// Passes (all on one stream, no kernel waits for another workgroup):
//   k_blk_flags    1 per non-empty sentence -> launch_exclusive_scan -> ne[i] = the non-empty sentences in front of i
//   k_blk_orbit    (whole) next(i), and per workgroup of BLK_ORBIT sentences, by pointer doubling in LDS, every entry's exit from its block and the
//                  orbit points on the way (hops); a sentence longer than L is reported (the smallest index)
//   k_blk_chain    (whole) one lane hops from block to block: the entry of every block the orbit visits and the rows in front of it; a block that
//                  `next` jumps over (more than BLK_ORBIT empty sentences) keeps BLK_NONE.  Serial in n / BLK_ORBIT, one dependent load a hop.
//   k_blk_walk     (whole) a thread per visited block walks from its entry to its exit and writes rowsent[rows in front + k]
//   k_blk_measure  a thread per row: rowsrc[r] and the fragments of the row (from ne) -> launch_exclusive_scan -> row_frags
//   k_blk_write    the flat output [n_rows L] in chunks of BLK_CHUNK elements, a wavefront per chunk in steps of 256 (64 lanes x 4 elements, one
//                  16-byte store per lane and array): a merge of the row grid with the sentence offsets.  The chunk's first sentence comes from one
//                  binary search; from then on the sentence starts inside a step are read 64 at a time (as many rounds as it takes: a run of
//                  empty sentences puts hundreds of boundaries on one position) and marked in the wavefront's 264 bytes of LDS by stream position.
//                  An element starts a fragment where its column is 0 or its stream position is marked; seg and pos come from the ballots of those
//                  starts (counts below the lane) and two max-scans (the last start; the starts in front of the last row start), with a carry
//                  across the steps: the ordinal so far and the open fragment's start.  The last id of a fragment writes its (start, length).
//   k_blk_keep     (tail = keep) the incomplete row's ids and boundaries into the open row's other generation
// Algorithmic bytes: read 4 K + 8 (S + 1), written 12 n_rows L + 8 n_frags + 8 (n_rows + 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yttm_device.h"
#include "yttm_kernels.h"

namespace yttm {

constexpr unsigned int BLK_STEP = 256;                    // elements a wavefront writes per step
constexpr unsigned int BLK_STEPS = 8;                     // steps per wavefront
constexpr unsigned int BLK_CHUNK = BLK_STEP * BLK_STEPS;  // elements per wavefront
constexpr unsigned int BLK_FLAG_WORDS = BLK_STEP / 4 + 2;  // a byte per stream position of a step, one more for the position behind it

// the largest i of [0, n] with voff(i) <= x (voff(0) = 0 <= x).  For x < total it is the non-empty sentence that holds position x.
__device__ inline unsigned long long blk_last_le(const BlkIn &in, unsigned long long x) {
  unsigned long long lo = 0, hi = in.n() + 1;
  while (hi - lo > 1) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    if (in.voff(mid) <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(BLOCK) void k_blk_flags(BlkIn in, uint32_t *__restrict__ cnt) {
  const unsigned long long n = in.n();
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK)
    cnt[i] = in.voff(i + 1) > in.voff(i) ? 1u : 0u;
}

__global__ __launch_bounds__(BLK_ORBIT) void k_blk_orbit(BlkIn in, unsigned long long L, uint32_t *__restrict__ nxt, unsigned long long *__restrict__ hop,
                                                         unsigned long long *__restrict__ bad) {
  __shared__ uint32_t tgt[BLK_ORBIT], hops[BLK_ORBIT];
  const uint32_t t = threadIdx.x;
  const unsigned long long n = in.n(), b0 = (unsigned long long)blockIdx.x * BLK_ORBIT, i = b0 + t;
  unsigned long long to = n;
  uint32_t h = 0;
  if (i < n) {
    const unsigned long long a = in.voff(i);
    if (in.voff(i + 1) - a > L) {
      atomicMin(bad, i);
      to = i + 1;
    } else {
      to = blk_last_le(in, a + L);  // (>= i + 1: sentence i fits)
    }
    h = 1;
    nxt[i] = (uint32_t)to;
  }
  tgt[t] = (uint32_t)to;
  hops[t] = h;
  __syncthreads();
  for (unsigned int round = 0; round < 10; round++) {  // 2^10 = BLK_ORBIT hops at the most
    const bool inside = to < n && to < b0 + BLK_ORBIT;
    const uint32_t u = inside ? (uint32_t)(to - b0) : t;
    const uint32_t t2 = tgt[u], h2 = hops[u];
    __syncthreads();
    if (inside) {
      to = t2;
      h += h2;
    }
    tgt[t] = (uint32_t)to;
    hops[t] = h;
    __syncthreads();
  }
  if (i < n) hop[i] = to | ((unsigned long long)h << 32);
}

// entry[] holds BLK_NONE before the launch.  info[0] = the orbit's rows.
__global__ void k_blk_chain(const unsigned long long *__restrict__ hop, unsigned long long n, uint32_t *__restrict__ entry, uint32_t *__restrict__ rowbase,
                            unsigned long long *__restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned long long cur = 0, rows = 0;
  while (cur < n) {
    const unsigned long long blk = cur / BLK_ORBIT;  // (a block `next` jumped over is never entered)
    entry[blk] = (uint32_t)cur;
    rowbase[blk] = (uint32_t)rows;
    const unsigned long long h = hop[cur];
    rows += h >> 32;
    cur = h & 0xffffffffull;
  }
  info[0] = rows;
}

// rowsent[rows + 1]: the first sentence of every row of the orbit, then n.  info[1] = the ids of the orbit's last row.
__global__ __launch_bounds__(64) void k_blk_walk(BlkIn in, const uint32_t *__restrict__ nxt, const uint32_t *__restrict__ entry,
                                                 const uint32_t *__restrict__ rowbase, unsigned long long n_blocks, uint32_t *__restrict__ rowsent,
                                                 unsigned long long *__restrict__ info) {
  const unsigned long long b = (unsigned long long)blockIdx.x * 64 + threadIdx.x, n = in.n();
  if (b >= n_blocks || entry[b] == BLK_NONE) return;
  unsigned long long cur = entry[b], r = rowbase[b], last = cur;
  const unsigned long long end = (b + 1) * BLK_ORBIT < n ? (b + 1) * BLK_ORBIT : n;
  while (cur < end) {
    rowsent[r++] = (uint32_t)cur;
    last = cur;
    cur = nxt[cur];
  }
  if (cur >= n) {
    rowsent[r] = (uint32_t)n;
    info[1] = in.total - in.voff(last);
  }
}

// a thread per row r of [0, n_rows]: rowsrc[r]; for r < n_rows the fragments of the row.  Stream mode: rowsent == nullptr.
__global__ __launch_bounds__(BLOCK) void k_blk_measure(BlkIn in, const unsigned long long *__restrict__ ne, unsigned long long L, unsigned long long n_rows,
                                                       const uint32_t *__restrict__ rowsent, uint32_t *__restrict__ cnt,
                                                       unsigned long long *__restrict__ rowsrc) {
  for (unsigned long long r = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; r <= n_rows; r += (unsigned long long)gridDim.x * BLOCK) {
    if (rowsent) {
      const unsigned long long a = rowsent[r];
      rowsrc[r] = in.voff(a);
      if (r < n_rows) cnt[r] = (uint32_t)(ne[rowsent[r + 1]] - ne[a]);
    } else {
      const unsigned long long src = r * L < in.total ? r * L : in.total;
      rowsrc[r] = src;
      if (r < n_rows) {
        const unsigned long long end = src + L < in.total ? src + L : in.total;  // (src < total: the row holds an id)
        cnt[r] = (uint32_t)(1 + ne[blk_last_le(in, end - 1)] - ne[blk_last_le(in, src)]);
      }
    }
  }
}

struct __attribute__((packed, aligned(4))) BlkQuad {  // four ids at an address that is only 4-byte aligned
  int32_t v[4];
};

struct BlkRows {  // where the rows take their ids from
  const unsigned long long *rowsrc;
  unsigned long long L, n_rows, n_out;
  // the stream position element e takes its id from, or, on padding and behind the output, that of the next element that takes one
  __device__ unsigned long long srcpos(unsigned long long e) const {
    if (e >= n_out) return rowsrc[n_rows];
    const unsigned long long r = e / L, c = e - r * L, s0 = rowsrc[r], s1 = rowsrc[r + 1];
    return c < s1 - s0 ? s0 + c : s1;
  }
};

__device__ inline uint32_t blk_incl_max(uint32_t v) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane_id() >= o && t > v) v = t;
  }
  return v;
}

__global__ __launch_bounds__(BLOCK) void k_blk_write(BlkIn in, const unsigned long long *__restrict__ ne, BlkRows R, const unsigned long long *__restrict__ row_frags,
                                                     int32_t pad, int32_t *__restrict__ rows, int32_t *__restrict__ seg, int32_t *__restrict__ pos,
                                                     int32_t *__restrict__ frags) {
  __shared__ uint32_t flag_words[NWAVES][BLK_FLAG_WORDS];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t *fw = flag_words[w];
  const uint8_t *flag = reinterpret_cast<const uint8_t *>(fw);
  const unsigned long long c0 = ((unsigned long long)blockIdx.x * NWAVES + (unsigned long long)w) * BLK_CHUNK;
  if (c0 >= R.n_out) return;
  const unsigned long long c1 = c0 + BLK_CHUNK < R.n_out ? c0 + BLK_CHUNK : R.n_out;
  const uint32_t L32 = (uint32_t)R.L;  // (n_rows L < 2^31: rows, columns and flat indices fit 32 bits)
  // ---- what the chunk's first element inherits: the starts of its row in front of it, and the last of them
  uint32_t carry_ord = 0, carry_start = (uint32_t)c0;
  unsigned long long p_first = R.srcpos(c0);
  {
    const unsigned long long r = c0 / R.L, c = c0 - r * R.L, s0 = R.rowsrc[r], len = R.rowsrc[r + 1] - s0;
    if (c != 0 && c < len) {
      const unsigned long long sp = blk_last_le(in, s0 + c - 1), at = in.voff(sp) > s0 ? in.voff(sp) : s0;
      carry_ord = (uint32_t)(1 + ne[sp] - ne[blk_last_le(in, s0)]);
      carry_start = (uint32_t)(c0 - (s0 + c - at));
    }
  }
  unsigned long long j = p_first ? blk_last_le(in, p_first - 1) + 1 : 0;  // the first sentence that starts at or behind p_first
  const unsigned long long n = in.n();
  for (unsigned long long b = c0; b < c1; b += BLK_STEP) {
    const unsigned long long p_end = R.srcpos(b + BLK_STEP);
    // ---- the sentence starts of [p_first, p_end], by stream position
    wave_sync();
    fw[lane] = 0;
    if (lane < BLK_FLAG_WORDS - 64) fw[64 + lane] = 0;
    wave_sync();
    for (;;) {
      const unsigned long long idx = j + lane;
      const unsigned long long x = idx < n ? in.voff(idx) : ~0ull;
      if (x <= p_end && x < in.total) reinterpret_cast<uint8_t *>(fw)[x - p_first] = 1;
      const uint32_t before = (uint32_t)__popcll(ballot_b(x < p_end));
      j += before;
      if (before < 64) break;
    }
    wave_sync();
    // ---- this lane's four elements
    const uint32_t e0 = (uint32_t)b + 4 * lane;
    uint32_t r = e0 / L32, c = e0 - r * L32;
    unsigned long long s0 = 0, len = 0;
    const bool inside0 = e0 < R.n_out;
    if (inside0) {
      s0 = R.rowsrc[r];
      len = R.rowsrc[r + 1] - s0;
    }
    bool valid[4], start[4], rowstart[4], last[4];
    unsigned long long p[4];
    uint32_t row_of[4];
    for (int k = 0; k < 4; k++) {
      const bool inside = e0 + k < R.n_out;
      valid[k] = inside && c < len;
      p[k] = s0 + c;
      row_of[k] = r;
      rowstart[k] = valid[k] && c == 0;
      const uint32_t at = valid[k] ? (uint32_t)(p[k] - p_first) : 0u;
      start[k] = valid[k] && (c == 0 || flag[at]);
      last[k] = valid[k] && (c + 1 == len || flag[at + 1]);
      if (++c == L32 && k < 3) {  // the next element opens the next row
        c = 0;
        r++;
        if (e0 + k + 1 < R.n_out) {
          s0 = R.rowsrc[r];
          len = R.rowsrc[r + 1] - s0;
        } else {
          len = 0;
        }
      }
    }
    // ---- the ids
    int32_t v[4];
    if (valid[0] && valid[3] && row_of[0] == row_of[3] && p[0] >= in.f) {
      const BlkQuad q = *reinterpret_cast<const BlkQuad *>(in.ids + (p[0] - in.f));
      for (int k = 0; k < 4; k++) v[k] = q.v[k];
    } else {
      for (int k = 0; k < 4; k++) v[k] = valid[k] ? in.id(p[k]) : pad;
    }
    // ---- starts below the lane, the last of them, the starts in front of the last row start (both + 1; 0: none in this step)
    const unsigned long long M0 = ballot_b(start[0]), M1 = ballot_b(start[1]), M2 = ballot_b(start[2]), M3 = ballot_b(start[3]);
    const uint32_t below = lanes_below(M0) + lanes_below(M1) + lanes_below(M2) + lanes_below(M3);
    uint32_t own_last = 0, own_cb = 0, cnt = below;
    for (int k = 0; k < 4; k++) {
      if (rowstart[k]) own_cb = cnt + 1;
      if (start[k]) {
        cnt++;
        own_last = 4 * lane + k + 1;
      }
    }
    const uint32_t inc_last = blk_incl_max(own_last);
    const bool any_row = ballot_b(own_cb != 0) != 0;
    const uint32_t inc_cb = any_row ? blk_incl_max(own_cb) : 0u;
    uint32_t last_s = __shfl_up(inc_last, 1), cb = __shfl_up(inc_cb, 1);
    if (lane == 0) last_s = cb = 0;
    // ---- seg, pos, and the fragments that end here
    int32_t sg[4], ps[4];
    cnt = below;
    for (int k = 0; k < 4; k++) {
      const uint32_t q = 4 * lane + k;
      if (rowstart[k]) cb = cnt + 1;
      if (start[k]) {
        cnt++;
        last_s = q + 1;
      }
      const uint32_t ord = cb ? cnt - (cb - 1) : carry_ord + cnt;
      const uint32_t at = last_s ? q - (last_s - 1) : (uint32_t)b + q - carry_start;
      sg[k] = valid[k] ? (int32_t)ord : 0;
      ps[k] = valid[k] ? (int32_t)at : 0;
      if (last[k]) {
        const unsigned long long g = row_frags[row_of[k]] + ord - 1;
        const uint32_t e = (uint32_t)b + q;
        *reinterpret_cast<unsigned long long *>(frags + 2 * g) = (unsigned long long)(e - at) | ((unsigned long long)(at + 1) << 32);
      }
    }
    if (inside0) {  // (the arrays end on a multiple of 4 elements: the last group is stored whole)
      *reinterpret_cast<uint4 *>(rows + e0) = make_uint4((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]);
      *reinterpret_cast<uint4 *>(seg + e0) = make_uint4((uint32_t)sg[0], (uint32_t)sg[1], (uint32_t)sg[2], (uint32_t)sg[3]);
      *reinterpret_cast<uint4 *>(pos + e0) = make_uint4((uint32_t)ps[0], (uint32_t)ps[1], (uint32_t)ps[2], (uint32_t)ps[3]);
    }
    // ---- the carry into the next step
    const uint32_t total_starts = (uint32_t)(__popcll(M0) + __popcll(M1) + __popcll(M2) + __popcll(M3));
    const uint32_t fin_last = uni(__shfl(inc_last, 63)), fin_cb = uni(__shfl(inc_cb, 63));
    carry_ord = fin_cb ? total_starts - (fin_cb - 1) : carry_ord + total_starts;
    if (fin_last) carry_start = (uint32_t)b + fin_last - 1;
    p_first = p_end;
  }
}

// The incomplete row behind the last emitted one, [p0, total), as the next open row: its ids and the starts of its fragments, new_off[m' + 1].
// info[2] = m'.
__global__ __launch_bounds__(BLOCK) void k_blk_keep(BlkIn in, const unsigned long long *__restrict__ ne, unsigned long long p0, int32_t *__restrict__ new_ids,
                                                    unsigned long long *__restrict__ new_off, unsigned long long *__restrict__ info) {
  const unsigned long long n = in.n(), f = in.total - p0, sf = blk_last_le(in, p0), m_new = ne[n] - ne[sf];
  const unsigned long long tid = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long i = tid; i < f; i += step) new_ids[i] = in.id(p0 + i);
  for (unsigned long long s = sf + 1 + tid; s < n; s += step)
    if (in.voff(s + 1) > in.voff(s)) new_off[ne[s] - ne[sf]] = in.voff(s) - p0;
  if (tid == 0) {
    new_off[0] = 0;
    new_off[m_new] = f;
    info[2] = m_new;
  }
}

static unsigned int blk_grid(unsigned long long items, unsigned long long per_block) {
  const unsigned long long b = (items + per_block - 1) / per_block;
  return (unsigned int)(b < 1 ? 1 : b > 256 * 16 ? 256 * 16 : b);
}

void launch_blk_flags(const BlkIn &in, uint32_t *cnt, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_flags, dim3(blk_grid(in.n(), BLOCK)), dim3(BLOCK), 0, st, in, cnt);
}
void launch_blk_orbit(const BlkIn &in, unsigned long long L, uint32_t *nxt, unsigned long long *hop, uint32_t *entry, uint32_t *rowbase, uint32_t *rowsent,
                      unsigned long long *bad, unsigned long long *info, hipStream_t st) {
  const unsigned long long n = in.n(), n_blocks = (n + BLK_ORBIT - 1) / BLK_ORBIT;
  hipLaunchKernelGGL(k_blk_orbit, dim3((unsigned int)n_blocks), dim3(BLK_ORBIT), 0, st, in, L, nxt, hop, bad);
  hipLaunchKernelGGL(k_blk_chain, dim3(1), dim3(64), 0, st, hop, n, entry, rowbase, info);
  hipLaunchKernelGGL(k_blk_walk, dim3((unsigned int)((n_blocks + 63) / 64)), dim3(64), 0, st, in, nxt, entry, rowbase, n_blocks, rowsent, info);
}
void launch_blk_measure(const BlkIn &in, const unsigned long long *ne, unsigned long long L, unsigned long long n_rows, const uint32_t *rowsent, uint32_t *cnt,
                        unsigned long long *rowsrc, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_measure, dim3(blk_grid(n_rows + 1, BLOCK)), dim3(BLOCK), 0, st, in, ne, L, n_rows, rowsent, cnt, rowsrc);
}
void launch_blk_write(const BlkIn &in, const unsigned long long *ne, unsigned long long L, unsigned long long n_rows, const unsigned long long *rowsrc,
                      const unsigned long long *row_frags, int32_t pad, int32_t *rows, int32_t *seg, int32_t *pos, int32_t *frags, hipStream_t st) {
  const BlkRows R{rowsrc, L, n_rows, n_rows * L};
  const unsigned long long waves = (R.n_out + BLK_CHUNK - 1) / BLK_CHUNK;
  hipLaunchKernelGGL(k_blk_write, dim3((unsigned int)((waves + NWAVES - 1) / NWAVES)), dim3(BLOCK), 0, st, in, ne, R, row_frags, pad, rows, seg, pos, frags);
}
void launch_blk_keep(const BlkIn &in, const unsigned long long *ne, unsigned long long p0, int32_t *new_ids, unsigned long long *new_off,
                     unsigned long long *info, hipStream_t st) {
  hipLaunchKernelGGL(k_blk_keep, dim3(blk_grid(in.total - p0 + 1, BLOCK)), dim3(BLOCK), 0, st, in, ne, p0, new_ids, new_off, info);
}

}  // namespace yttm
