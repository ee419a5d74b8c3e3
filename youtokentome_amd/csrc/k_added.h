// k_added.h -- the added tokens on the device (the rule is in include/yttm_mi355x.h "Added tokens"): literal byte strings that are matched in
// the batch's text, never split, and stand in the ids as one id each.  Included at the end of k_encode.hip like its siblings.  Two families:
//
// The split: text + offsets[n_sent + 1] -> the refined batch, in which every sentence is cut into its segments and matches
//   g_0, m_1, g_1, ..., m_j, g_j (2 j + 1 sub-sentences, a segment may be empty): sub_first[n_sent + 1], sub_off[n_sub + 1], tok[n_sub]
//   (the token's index for a match, -1 for a segment).
//   measure  k_added_split<false>: cnt[s] = 2 * (matches of sentence s) + 1
//   scan     launch_exclusive_scan(cnt) -> sub_first[n_sent + 1]                                                      (k_frontend.hip)
//   write    k_added_split<true>: the same walk again; an accepted match r of sentence s stores sub_off / tok [sub_first[s] + 2 r + 1, + 2]
//   Finding the candidates does not depend on order: the lane of byte p asks, cheapest first, the 256-bit set of first bytes (four 64-bit
//   kernel arguments, scalar registers), then the directory's bucket of the two leading bytes (the tokens of a bucket longest first, so the
//   first that compares equal is the longest at p; an entry holds the token's place in the blob, its length and its index in one 64-bit
//   word; a one-byte token is looked up by its byte where no longer one matched), then compares bytes, eight at a time.  Only the greedy
//   selection is sequential: `covered` (the first byte behind the last accepted match) is carried across the 64-byte rows, a lane below it is
//   no candidate, and a row's candidate ballot is resolved in a scalar loop that runs once per ACCEPTED match (the candidates an accepted
//   match covers are cleared with one shift).  A match never reads or crosses its sentence's end.
//   Mapping (k_subword.h's): a wavefront takes a group of at most 63 consecutive sentences, a lane per boundary, and walks one sentence after the
//   other, 64 bytes a row, a lane per byte; the bytes of ADD_ROWS rows are loaded together before the first row is looked at, so a sentence of
//   up to 256 bytes is one round trip to memory.  No LDS, no global atomic, nothing depends on the order of the workgroups; the inputs are only read.
//   Algorithmic bytes (N bytes of text, S sentences): read N + 8 (S + 1), written 8 (n_sub + 1) + 4 n_sub + 8 (S + 1).  (Not counted: the write
//   pass reads the text and the offsets a second time; cnt, 4 S, written, read and scanned in between; the token tables, which stay in L2.)
//
// The join: the ids of the refined batch (encoded with bos = eos = reverse = false) + tok + sub_first -> the sentences' ids:
//   [bos]? ++ ids(g_0) ++ [first + k(m_1)] ++ ids(g_1) ++ ... ++ ids(g_j) ++ [eos]?, back to front as a whole where `reverse` is set.
//   measure  k_added_join_measure: out_len[s], a thread per sentence
//   scan     launch_exclusive_scan(out_len) -> out_off[n_sent + 1]
//   write    k_added_join: a wavefront takes a group of sentences, whose output is contiguous, and appends sub-sentence after sub-sentence
//            through k_textout.h's TileWriter with 4-byte elements (k_restrict.h), 64 ids a step; the output leaves as 16-byte stores.
//   Algorithmic bytes (K_in refined ids, K_out ids): read 4 K_in + 8 (n_sub + 1) + 4 n_sub + 8 (S + 1), written 4 K_out + 8 (S + 1).
// Limits: a single sentence is walked by one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "added_plan.h"
#include "k_textout.h"
#include "yttm_kernels.h"

namespace yttm {

static_assert(SUB_FLUSH + 4u * 64u <= (uint32_t)DEC_TILE, "a step of 64 ids fits behind SUB_FLUSH - 1 staged bytes");

constexpr int ADD_ROWS = 4;  // 64-byte rows of a step: a lane loads a byte of each before the first is looked at (four loads in flight)

// len bytes of a and b, eight at a time: the loads of a chunk do not wait for one another
__device__ inline bool added_equal(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t len) {
  for (uint32_t i = 0; i < len; i += 8) {
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
      if (i + j < len) diff |= (uint32_t)a[i + j] ^ (uint32_t)b[i + j];
    if (diff) return false;
  }
  return true;
}

// the longest token at text[p ..) that ends at or in front of `end`: its length (0: none) and its index.  c0, c1: text[p], text[p + 1]
// (c1 only where p + 1 < end).  A candidate costs three dependent loads: the bucket's bounds, a list entry, the bytes.
__device__ inline uint32_t added_match_at(const AddedTable &tb, const uint8_t *__restrict__ text, unsigned long long p, unsigned long long end, uint32_t c0,
                                          uint32_t c1, uint32_t *tok) {
  if (p + 1 < end) {
    const uint32_t b = added_bucket(c0, c1);
    for (uint32_t q = tb.dir_off[b], q1 = tb.dir_off[b + 1]; q < q1; q++) {  // longest first
      const unsigned long long e = tb.list[q];
      const uint32_t len = added_entry_len(e);
      if (p + len > end) continue;
      if (added_equal(text + p, tb.blob + added_entry_off(e), len)) {
        *tok = added_entry_tok(e);
        return len;
      }
    }
  }
  const uint32_t k = tb.one[c0];
  if (k == ADDED_NO_TOKEN) return 0;
  *tok = k;
  return 1;
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_added_split(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ off, unsigned long long n_sent,
                                                       AddedTable tb, unsigned int group, uint32_t *__restrict__ cnt,
                                                       const unsigned long long *__restrict__ sub_first, unsigned long long *__restrict__ sub_off,
                                                       int32_t *__restrict__ tok) {
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt();
  if (WRITE && blockIdx.x == 0 && threadIdx.x == 0) sub_off[sub_first[n_sent]] = off[n_sent];
  for (WaveGroups wg(n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds sb(off, g0, g1, lane), fb(WRITE ? sub_first : off, g0, g1, lane);
    uint32_t my_cnt = 0;  // (measure) lane j: the sub-sentences of sentence g0 + j
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long b0 = sb.at(j), b1 = sb.at(j + 1);
      const unsigned long long sf = fb.at(j);  // (write) the sentence's first sub-sentence
      if (WRITE && lane == 0) {
        sub_off[sf] = b0;
        tok[sf] = -1;
      }
      unsigned long long covered = b0;  // the first byte behind the last accepted match: carried across the rows and the steps
      uint32_t n_match = 0;
      for (unsigned long long step = b0; step < b1; step += 64ull * ADD_ROWS) {
        uint32_t c[ADD_ROWS];
#pragma unroll
        for (int r = 0; r < ADD_ROWS; r++) {
          const unsigned long long q = step + 64ull * r + lane;
          c[r] = q < b1 ? text[q] : 0u;
        }
#pragma unroll
        for (int r = 0; r < ADD_ROWS; r++) {
          const unsigned long long base = step + 64ull * r;
          if (base >= b1) break;  // (uniform)
          const unsigned long long p = base + lane;
          const bool inside = p < b1;
          const uint32_t c0 = c[r];
          // the next byte: the neighbouring lane's, for lane 63 lane 0's of the next row (behind the last row: a load)
          uint32_t c1 = __shfl_down(c0, 1);
          const uint32_t wrap = r + 1 < ADD_ROWS ? (uint32_t)__shfl(c[r + 1 < ADD_ROWS ? r + 1 : r], 0) : 0u;
          if (lane == 63u) c1 = r + 1 < ADD_ROWS ? wrap : (p + 1 < b1 ? text[p + 1] : 0u);
          const unsigned long long fw = c0 < 128u ? (c0 < 64u ? tb.first[0] : tb.first[1]) : (c0 < 192u ? tb.first[2] : tb.first[3]);
          uint32_t mlen = 0, mtok = 0;
          if (inside && p >= covered && ((fw >> (c0 & 63u)) & 1ull)) mlen = added_match_at(tb, text, p, b1, c0, c1, &mtok);
          // ---- the greedy selection among the row's candidates: leftmost first, and nothing that an accepted match covers
          unsigned long long cand = ballot_b(mlen != 0), acc = 0;
          while (cand) {
            const int l = __ffsll((long long)cand) - 1;
            const uint32_t len = uni(__shfl(mlen, l));
            acc |= 1ull << l;
            covered = base + (unsigned long long)l + len;
            const unsigned long long rel = covered - base;
            cand = rel >= 64 ? 0ull : cand & (~0ull << rel);
          }
          if (WRITE && ((acc >> lane) & 1ull)) {
            const unsigned long long at = sf + 2ull * (n_match + (uint32_t)__popcll(acc & lt)) + 1ull;
            sub_off[at] = p;
            tok[at] = (int32_t)mtok;
            sub_off[at + 1] = p + mlen;  // (the segment behind the match; it may be empty)
            tok[at + 1] = -1;
          }
          n_match += (uint32_t)__popcll(acc);
        }
      }
      if (!WRITE && lane == (uint32_t)j) my_cnt = 2u * n_match + 1u;
    }
    if (!WRITE && g0 + lane < g1) cnt[g0 + lane] = my_cnt;
  }
}

// out_len[s] of the join: the ids of the sentence's segments, one id per match, bos and eos
__global__ __launch_bounds__(BLOCK) void k_added_join_measure(AddedJoin in, uint32_t *__restrict__ out_len) {
  for (unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; s < in.n_sent; s += (unsigned long long)gridDim.x * BLOCK) {
    const unsigned long long f0 = in.sub_first[s], f1 = in.sub_first[s + 1];
    unsigned long long len = (in.bos ? 1u : 0u) + (in.eos ? 1u : 0u);
    for (unsigned long long i = f0; i < f1; i++) len += in.tok[i] < 0 ? in.roff[i + 1] - in.roff[i] : 1ull;
    out_len[s] = (uint32_t)len;
  }
}

__global__ __launch_bounds__(BLOCK) void k_added_join(AddedJoin in, unsigned int group, const unsigned long long *__restrict__ out_off, int32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[NWAVES][DEC_TILE];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  for (WaveGroups wg(in.n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds fb(in.sub_first, g0, g1, lane);
    TileWriter stg(s_tile[w], lane);
    stg.open(reinterpret_cast<uint8_t *>(out), 4ull * uni64(out_off[g0]));
    const auto put = [&](int32_t id) {  // one id; fewer than SUB_FLUSH bytes are staged before and behind it
      if (lane == 0) *reinterpret_cast<int32_t *>(stg.at(0)) = id;
      stg.commit(4u);
      stg.flush_if_due();
    };
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long f0 = fb.at(j), f1 = fb.at(j + 1);
      if (in.reverse ? in.eos : in.bos) put(in.reverse ? in.eos_id : in.bos_id);
      for (unsigned long long q = 0; q < f1 - f0; q++) {
        const unsigned long long i = in.reverse ? f1 - 1 - q : f0 + q;  // (every slot is visited: an empty segment appends nothing)
        const int32_t t = uni(in.tok[i]);
        if (t >= 0) {
          put(in.first + t);
          continue;
        }
        const unsigned long long r0 = uni64(in.roff[i]), r1 = uni64(in.roff[i + 1]);
        for (unsigned long long c = r0; c < r1; c += 64) {
          const uint32_t n = r1 - c < 64 ? (uint32_t)(r1 - c) : 64u;
          if (lane < n) reinterpret_cast<int32_t *>(stg.at(0))[lane] = in.reverse ? in.rids[r1 - 1 - (c - r0) - lane] : in.rids[c + lane];
          stg.commit(4u * n);
          stg.flush_if_due();
        }
      }
      if (in.reverse ? in.bos : in.eos) put(in.reverse ? in.bos_id : in.eos_id);
    }
    stg.close();
  }
}

// each pass is given what it uses.  write: sub_first[n_sent + 1] is the exclusive scan of cnt; sub_off holds sub_first[n_sent] + 1 entries, tok
// sub_first[n_sent]
void launch_added_split(bool write, const uint8_t *text, const unsigned long long *off, unsigned long long n_sent, unsigned long long n_bytes,
                        const AddedTable &tb, uint32_t *cnt, const unsigned long long *sub_first, unsigned long long *sub_off, int32_t *tok, hipStream_t st) {
  if (!n_sent) return;
  const unsigned int group = group_size(n_sent, n_bytes, 4096, LANE_GROUP_MAX);
  const dim3 grid = grid_for_groups(n_sent, group), block(BLOCK);
  if (write) hipLaunchKernelGGL((k_added_split<true>), grid, block, 0, st, text, off, n_sent, tb, group, (uint32_t *)nullptr, sub_first, sub_off, tok);
  else hipLaunchKernelGGL((k_added_split<false>), grid, block, 0, st, text, off, n_sent, tb, group, cnt, (const unsigned long long *)nullptr,
                          (unsigned long long *)nullptr, (int32_t *)nullptr);
}

// out: 16-byte aligned, out_off: the exclusive scan of out_len, in ids.  n_ids (the refined batch's) sizes the groups.
void launch_added_join(bool write, const AddedJoin &in, unsigned long long n_ids, uint32_t *out_len, const unsigned long long *out_off, int32_t *out,
                       hipStream_t st) {
  if (!in.n_sent) return;
  if (!write) {
    hipLaunchKernelGGL(k_added_join_measure, grid_for(in.n_sent, BLOCK), dim3(BLOCK), 0, st, in, out_len);
    return;
  }
  const unsigned int group = group_size(in.n_sent, n_ids, 256, LANE_GROUP_MAX);
  hipLaunchKernelGGL(k_added_join, grid_for_groups(in.n_sent, group), dim3(BLOCK), 0, st, in, group, out_off, out);
}

}  // namespace yttm
