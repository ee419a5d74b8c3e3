// k_subword.h -- SUBWORD output on the device: the ids K5 left + the sentences' text -> the text `yttm encode --output_type subword` prints.
// Included at the end of k_encode.hip (behind k_decode.h; the output goes through k_textout.h's TileWriter, the classification of a byte is enc_classify).
//
// replaces: BaseEncoder::encode_as_subwords bpe.h:41-46, bpe.cpp:1757 (pieces by id_to_subword(id, false) bpe.cpp:1774-1807, unknown runs
// bpe.cpp:1597-1613) + the formatting of encode_cli bpe.cpp:1942-2014 (utils.h:92-103: every piece followed by one space, then '\n'), for a batch.
//
// The text of every id lives in HBM as one blob + piece_off[V + 1], filled from the host's id_to_subword(id, replace_space = false)
// (host_decode.cpp): one definition of a piece's text.  The id unk_id never reads it: the k-th unk_id of a sentence in FORWARD order is the k-th
// maximal run of valid, non-space code points outside the alphabet, its text the UTF-8 of those code points -- invalid bytes inside
// a run are dropped and do not end it.  With `reverse` K5 stored the ids back to front, so the k-th unk_id in stored order of a sentence with n of
// them is run n - 1 - k (the host loop formats forward and reverses the pieces).  A run the sentence does not have gives "".
// Three steps on the lane's stream, none waits for another's progress, no global atomic:
//   measure  k_subword<false>: out_len[s] = sum over the sentence's ids of (piece bytes + 1) + 1
//   scan     launch_exclusive_scan(out_len) -> line_off[S + 1]                                                       (k_frontend.hip)
//   write    k_subword<true>: pieces, runs, spaces and newlines -> the tile writer -> the output blob
// Algorithmic bytes (K ids, S sentences, B_out output bytes): read 4 K + 8 (S + 1) + the text of the sentences that hold an unk_id, written
// B_out + 8 (S + 1).  (Not counted: the sentences' byte offsets, another 8 (S + 1); the write pass reads ids, offsets and that text a second
// time; the table, which stays in L2.)
//
// Mapping: a wavefront takes a GROUP of consecutive sentences (their output is contiguous: line_off is a scan in sentence order) and walks one
// sentence after the other, its ids 64 at a time, a lane per id.  A sentence without an unk_id never touches its text.  One with an unk_id is
// classified 64 bytes a step (sub_walk_runs: the carry of "the last valid char was unknown" crosses the steps); the write pass keeps the runs
// it needs -- first byte, end, valid bytes -- in an LDS directory of SUB_DIR runs and walks the text again when a step's runs lie outside it (a
// sentence of thousands of runs: once per SUB_DIR of them).
// Limits: a sentence (text and output) below 4 GB; a single sentence is walked by one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_decode.h"

namespace yttm {

constexpr int SUB_DIR = 128;        // runs of a sentence the write pass holds at a time
constexpr uint32_t SUB_LANE_RUN = 64;  // a run of more valid bytes than this is copied by the whole wave, not by its lane

// Is byte i of the sentence kept by the reference's decode (utf8.cpp:111-128)?  A byte inside a valid char, which is every byte except the start
// of an invalid one.  (Between the first and the last byte of an unknown run every valid char belongs to the run.)
__device__ inline bool sub_keep(const uint8_t *__restrict__ s, unsigned long long i, unsigned long long nbytes) {
  if (!u8_is_start(s, i, nbytes)) return true;
  uint32_t len;
  return u8_decode_at(s, i, nbytes, &len) != INVALID_CP;
}

// The unknown runs of a sentence, 64 bytes a step: f(c, i, r) in the lane of every valid unknown char (c: its class, i: its first byte, r: the
// number of its run).  Returns the number of runs.  All lanes call.
template <class F>
__device__ inline uint32_t sub_walk_runs(const EncModel &m, const uint8_t *__restrict__ s, unsigned long long nbytes, F &&f) {
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt();
  bool carry_unk = false;  // the last valid char before this step was an unknown one
  uint32_t runs = 0;
  for (unsigned long long b0 = 0; b0 < nbytes; b0 += 64) {
    const unsigned long long i = b0 + lane;
    EncChar c;
    enc_classify(m, s, i, nbytes, c);
    const unsigned long long V = ballot_b(c.valid), U = ballot_b(c.unk);
    bool prev_unk = carry_unk;
    const unsigned long long pv = V & lt;
    if (pv) prev_unk = (U >> (63 - __clzll((long long)pv))) & 1ull;
    const unsigned long long ST = ballot_b(c.unk && !prev_unk);  // a space or a known char in front, or the sentence's start
    if (c.unk) f(c, i, runs + (uint32_t)__popcll(ST & (lt | (1ull << lane))) - 1u);
    runs += (uint32_t)__popcll(ST);
    if (V) carry_unk = (U >> (63 - __clzll((long long)V))) & 1ull;
  }
  return runs;
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_subword(EncModel m, SubInput in, DecTable tb, unsigned int group, uint32_t *__restrict__ out_len,
                                                   const unsigned long long *__restrict__ out_off, uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[WRITE ? NWAVES : 1][WRITE ? DEC_TILE : 16];
  __shared__ uint32_t s_beg[WRITE ? NWAVES : 1][SUB_DIR], s_end[WRITE ? NWAVES : 1][SUB_DIR], s_vlen[WRITE ? NWAVES : 1][SUB_DIR];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt();
  uint32_t *const beg = s_beg[WRITE ? w : 0], *const end = s_end[WRITE ? w : 0], *const vlen = s_vlen[WRITE ? w : 0];
  for (WaveGroups wg(in.n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds ib(in.ioff, g0, g1, lane), sb(in.soff, g0, g1, lane);
    uint32_t my_len = 0;  // (measure) lane j: the output bytes of sentence g0 + j
    TileWriter stg(s_tile[WRITE ? w : 0], lane);
    if (WRITE) stg.open(out, uni64(out_off[g0]));
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long i0 = ib.at(j), i1 = ib.at(j + 1);
      const unsigned long long b0 = sb.at(j), nbytes = sb.at(j + 1) - b0;
      const uint8_t *s = in.text + b0;
      if (!WRITE) {
        uint32_t acc = 0, n_unk = 0;
        for (unsigned long long base = i0; base < i1; base += 64) {
          const unsigned long long k = base + lane;
          const bool inside = k < i1;
          const int32_t id = inside ? in.ids[k] : 0;
          const bool is_unk = inside && id == in.unk_id;
          if (inside && !is_unk && (uint32_t)id < tb.vocab) acc += tb.piece_off[id + 1] - tb.piece_off[id];
          if (inside) acc++;  // the space behind every piece
          n_unk += (uint32_t)__popcll(ballot_b(is_unk));
        }
        if (n_unk) sub_walk_runs(m, s, nbytes, [&](const EncChar &c, unsigned long long, uint32_t r) { if (r < n_unk) acc += c.len; });
        const uint32_t total = uni(__shfl(wave_incl_scan(acc), 63)) + 1u;  // + the newline
        if (lane == (uint32_t)j) my_len = total;
        continue;
      }
      // ---- write
      uint32_t n_unk = 0;  // (reverse) the sentence's unk_ids: the k-th in stored order is run n_unk - 1 - k
      if (in.reverse) {
        for (unsigned long long base = i0; base < i1; base += 64) {
          const unsigned long long k = base + lane;
          n_unk += (uint32_t)__popcll(ballot_b(k < i1 && in.ids[k] == in.unk_id));
        }
      }
      uint32_t unk_seen = 0, w0 = 0;  // unk_ids in front of this step; the directory holds runs [w0, w0 + SUB_DIR)
      bool dir_valid = false;
      for (unsigned long long base = i0; base < i1; base += 64) {
        const unsigned long long k = base + lane;
        const bool inside = k < i1;
        const int32_t id = inside ? in.ids[k] : 0;
        const bool is_unk = inside && id == in.unk_id;
        const unsigned long long UK = ballot_b(is_unk);
        uint32_t src = 0, len = 0, rb = 0, re = 0;
        if (inside && !is_unk && (uint32_t)id < tb.vocab) {
          src = tb.piece_off[id];
          len = tb.piece_off[id + 1] - src;
        }
        if (UK) {
          const uint32_t cnt = (uint32_t)__popcll(UK);
          const uint32_t ord = unk_seen + (uint32_t)__popcll(UK & lt);
          const uint32_t f = in.reverse ? n_unk - 1u - ord : ord;  // the run of this lane's unk_id, in forward order
          const uint32_t fmin = in.reverse ? n_unk - unk_seen - cnt : unk_seen, fmax = fmin + cnt - 1u;
          if (!dir_valid || fmin < w0 || fmax >= w0 + (uint32_t)SUB_DIR) {
            w0 = in.reverse ? (fmax + 1u > (uint32_t)SUB_DIR ? fmax + 1u - (uint32_t)SUB_DIR : 0u) : fmin;
            wave_sync();
            for (uint32_t q = lane; q < (uint32_t)SUB_DIR; q += 64) {
              beg[q] = 0xffffffffu;
              end[q] = 0;
              vlen[q] = 0;
            }
            wave_sync();
            sub_walk_runs(m, s, nbytes, [&](const EncChar &c, unsigned long long i, uint32_t r) {
              if (r >= w0 && r - w0 < (uint32_t)SUB_DIR) {
                atomicMin(&beg[r - w0], (uint32_t)i);
                atomicMax(&end[r - w0], (uint32_t)i + c.len);
                atomicAdd(&vlen[r - w0], c.len);
              }
            });
            wave_sync();
            dir_valid = true;
          }
          if (is_unk) {  // (a run the sentence does not have: no bytes)
            len = vlen[f - w0];
            rb = beg[f - w0];
            re = end[f - w0];
            if (!len) rb = re = 0;
          }
          unk_seen += cnt;
        }
        const uint32_t olen = inside ? len + 1u : 0u;
        const uint32_t inc = wave_incl_scan(olen);
        const uint32_t x = inc - olen, total = uni(__shfl(inc, 63));
        const bool wide = total > (uint32_t)DEC_SEG || ballot_b(is_unk && len > SUB_LANE_RUN) != 0ull;
        if (wide || !stg.fits(total)) stg.flush_units();
        if (!wide) {
          if (inside) {
            uint8_t *const p = stg.at(x);
            if (is_unk) {
              uint32_t n = 0;
              for (uint32_t i = rb; i < re; i++)
                if (sub_keep(s, i, nbytes)) p[n++] = s[i];
            } else {
              for (uint32_t b = 0; b < len; b++) p[b] = tb.blob[src + b];
            }
            p[len] = (uint8_t)' ';
          }
          stg.commit(total);
        } else {  // pieces that do not fit the tile together, or a long run: one by one, the wave copies a piece
          unsigned long long pm = ballot_b(inside);
          while (pm) {
            const int l = __ffsll((long long)pm) - 1;
            pm &= pm - 1;
            const uint32_t plen = uni(__shfl(len, l)), psrc = uni(__shfl(src, l)), prb = uni(__shfl(rb, l)), pre = uni(__shfl(re, l));
            if ((UK >> l) & 1ull) {  // a run streams through the tile 64 bytes of text a step, its invalid bytes filtered out
              for (uint32_t c0 = prb; c0 < pre; c0 += 64) {
                const uint32_t i = c0 + lane;
                stg.append_kept(i < pre && sub_keep(s, i, nbytes), [&]() { return s[i]; });
              }
            } else {
              stg.copy_piece(tb.blob + psrc, plen);
            }
            stg.append_byte((uint8_t)' ');
          }
          stg.flush_units();
        }
      }
      stg.append_byte((uint8_t)'\n');
    }
    if (WRITE) {
      stg.close();
    } else if (g0 + lane < g1) {
      out_len[g0 + lane] = my_len;
    }
  }
}

// sentences per group of the kernels that hold a group's boundaries a lane each (k_subword, k_idprint, k_spans): about 256 ids
static unsigned int lane_group(unsigned long long n_sent, unsigned long long n_ids) { return group_size(n_sent, n_ids, 256, LANE_GROUP_MAX); }

// each pass is given what it uses
void launch_subword(bool write, const EncModel &m, const SubInput &in, const DecTable &tb, unsigned long long n_ids, uint32_t *out_len,
                    const unsigned long long *out_off, uint8_t *out, hipStream_t st) {
  if (!in.n_sent) return;
  const unsigned int group = lane_group(in.n_sent, n_ids);
  const dim3 grid = grid_for_groups(in.n_sent, group), block(BLOCK);
  if (write) hipLaunchKernelGGL((k_subword<true>), grid, block, 0, st, m, in, tb, group, (uint32_t *)nullptr, out_off, out);
  else hipLaunchKernelGGL((k_subword<false>), grid, block, 0, st, m, in, tb, group, out_len, (const unsigned long long *)nullptr, (uint8_t *)nullptr);
}

}  // namespace yttm
