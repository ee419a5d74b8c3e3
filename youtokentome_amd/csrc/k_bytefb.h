// k_bytefb.h -- the byte fallback on the device: ids + offsets + the sentences' text -> every unk_id that stands for an unknown run replaced by
// the ids V + b of the run's UTF-8 bytes (the rule is in include/yttm_mi355x.h "Byte fallback").  Included at the end of k_encode.hip like its
// siblings; the runs are found by k_subword.h's sub_walk_runs over enc_classify, the output goes through k_textout.h's TileWriter with 4-byte
// elements as in k_restrict.h.
//
// The k-th unk_id of a sentence in FORWARD order is the sentence's k-th unknown run (k_subword.h); with `reverse` the ids are stored back to
// front, the k-th stored unk_id of a sentence with n of them is run n - 1 - k, and the run's bytes are stored back to front too.  An unk_id
// whose sentence has no such run stays; runs beyond the sentence's unk_ids are ignored.  Every other id stays.
// Three steps on the lane's stream, none waits for another's progress, no global atomic:
//   measure  k_bytefb<false>: out_len[s] = n_ids(s) - (unk_ids that have a run) + the valid bytes of those runs; *saw = 1 where a wavefront met
//            an unk_id at all (a plain store, the same value from every wavefront)
//   scan     launch_exclusive_scan(out_len) -> out_off[S + 1], in ids                                                 (k_frontend.hip)
//   write    k_bytefb<true>: ids and byte ids -> LDS staging tile -> the output in aligned 16-byte stores
// The host skips the write pass only when *saw stayed 0: a run of one ASCII char leaves the total as it was and still changes the id.
// Algorithmic bytes (K_in ids, K_out ids, S sentences): read 4 K_in + 8 (S + 1) + the text of the sentences that hold an unk_id, written
// 4 K_out + 8 (S + 1).  (Not counted: the sentences' byte offsets, another 8 (S + 1); the write pass reads ids, offsets and that text again.)
//
// Mapping (k_subword.h's): a wavefront takes a GROUP of consecutive sentences and walks one after the other, its ids 64 at a time, a lane per
// id.  A sentence without an unk_id never touches its text; the measure pass asks the whole group first, 64 ids a step across the sentences,
// and a group without an unk_id is done with its offsets alone.  The write pass keeps the runs it needs -- first byte, end, valid bytes -- in
// an LDS directory of SUB_DIR runs and walks the text again when a step's runs lie outside it.  A step whose expansions do not fit the tile
// together is staged in runs of lanes that do; a run of more than SUB_LANE_RUN valid bytes is copied by the whole wavefront, 64 bytes of text a
// step (bytefb_copy_long).
// Limits: a sentence (text and output) below 4 GB; a single sentence is walked by one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_restrict.h"
#include "k_subword.h"

namespace yttm {

static_assert(SUB_FLUSH + 4u * 64u <= (uint32_t)DEC_TILE, "a 64-byte step of a long run, as ids, fits behind SUB_FLUSH - 1 staged bytes");
static_assert(SUB_LANE_RUN <= RST_SEG, "a run that its lane copies fits a segment alone: the runs of lanes always advance");

// One run of any length, text[rb, re) with its invalid bytes filtered out, as ids first + byte: the whole wavefront, 64 bytes of text a step
// (back to front where the sentence is stored so).  Fewer than SUB_FLUSH bytes are staged before and behind it.
__device__ inline void bytefb_copy_long(TileWriter &stg, const uint8_t *__restrict__ s, unsigned long long nbytes, uint32_t rb, uint32_t re, int32_t first,
                                        bool reverse, uint32_t lane) {
  const unsigned long long lt = lanemask_lt();
  for (uint32_t c0 = 0; c0 < re - rb; c0 += 64) {
    const uint32_t c = c0 + lane;
    const bool in_run = c < re - rb;
    const uint32_t i = reverse ? re - 1u - c : rb + c;
    const bool keep = in_run && sub_keep(s, i, nbytes);
    const unsigned long long K = ballot_b(keep);
    int32_t *const p = reinterpret_cast<int32_t *>(stg.at(0));
    if (keep) p[__popcll(K & lt)] = first + (int32_t)s[i];
    stg.commit(4u * (uint32_t)__popcll(K));
    stg.flush_if_due();
  }
}

struct ByteFbInput {  // SubInput and the first byte id
  SubInput sub;
  int32_t first;  // V: byte b is the id first + b
};

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_bytefb(EncModel m, ByteFbInput bin, unsigned int group, uint32_t *__restrict__ out_len, uint32_t *__restrict__ saw,
                                                  const unsigned long long *__restrict__ out_off, int32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[WRITE ? NWAVES : 1][WRITE ? DEC_TILE : 16];
  __shared__ uint32_t s_beg[WRITE ? NWAVES : 1][WRITE ? SUB_DIR : 1], s_end[WRITE ? NWAVES : 1][WRITE ? SUB_DIR : 1], s_vlen[WRITE ? NWAVES : 1][WRITE ? SUB_DIR : 1];
  const SubInput &in = bin.sub;
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt();
  uint32_t *const beg = s_beg[WRITE ? w : 0], *const end = s_end[WRITE ? w : 0], *const vlen = s_vlen[WRITE ? w : 0];
  bool saw_any = false;  // (measure) this wavefront met an unk_id
  for (WaveGroups wg(in.n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds ib(in.ioff, g0, g1, lane), sb(in.soff, g0, g1, lane);
    if (!WRITE) {
      // ---- the whole group first, across its sentences: without an unk_id every length is a difference of offsets
      const unsigned long long k0 = ib.at(0), k1 = ib.at((int)(g1 - g0));
      bool any = false;
      for (unsigned long long base = k0; base < k1; base += 64) {
        const unsigned long long k = base + lane;
        any = any || ballot_b(k < k1 && in.ids[k] == in.unk_id) != 0ull;
      }
      if (!any) {
        const unsigned long long nxt = __shfl_down(ib.mine, 1);
        if (g0 + lane < g1) out_len[g0 + lane] = (uint32_t)(nxt - ib.mine);
        continue;
      }
      saw_any = true;
    }
    uint32_t my_len = 0;  // (measure) lane j: the output ids of sentence g0 + j
    TileWriter stg(s_tile[WRITE ? w : 0], lane);
    if (WRITE) stg.open(reinterpret_cast<uint8_t *>(out), 4ull * uni64(out_off[g0]));
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long i0 = ib.at(j), i1 = ib.at(j + 1);
      const unsigned long long b0 = sb.at(j), nbytes = sb.at(j + 1) - b0;
      const uint8_t *s = in.text + b0;
      if (!WRITE) {
        uint32_t n_unk = 0;
        for (unsigned long long base = i0; base < i1; base += 64) {
          const unsigned long long k = base + lane;
          n_unk += (uint32_t)__popcll(ballot_b(k < i1 && in.ids[k] == in.unk_id));
        }
        uint32_t total = (uint32_t)(i1 - i0);
        if (n_unk) {
          uint32_t acc = 0;
          const uint32_t runs = sub_walk_runs(m, s, nbytes, [&](const EncChar &c, unsigned long long, uint32_t r) { if (r < n_unk) acc += c.len; });
          total += uni(__shfl(wave_incl_scan(acc), 63)) - (runs < n_unk ? runs : n_unk);  // (an unk_id without a run stays)
        }
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
        uint32_t len = inside ? 1u : 0u, rb = 0, re = 0;
        bool run = false;  // this lane's unk_id has a run: len valid bytes within text[rb, re)
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
          if (is_unk && vlen[f - w0]) {  // (a run the sentence does not have: the unk_id stays)
            run = true;
            len = vlen[f - w0];
            rb = beg[f - w0];
            re = end[f - w0];
          }
          unk_seen += cnt;
        }
        const uint32_t inc = wave_incl_scan(len);
        const uint32_t x = inc - len, total = uni(__shfl(inc, 63));
        const bool big = run && len > SUB_LANE_RUN;
        const unsigned long long BIG = ballot_b(big);
        const auto stage = [&](uint32_t at) {  // this lane's id or its run's byte ids, `at` ids behind the staged ones
          int32_t *const p = reinterpret_cast<int32_t *>(stg.at(4u * at));
          if (run) {
            uint32_t n = 0;
            for (uint32_t i = rb; i < re; i++)
              if (sub_keep(s, i, nbytes)) p[in.reverse ? len - 1u - n++ : n++] = bin.first + (int32_t)s[i];
          } else if (inside) {
            p[0] = id;
          }
        };
        if (!BIG && total <= RST_SEG) {
          if (!stg.fits(4u * total)) stg.flush_units();  // (behind it fewer than 16 bytes are staged: a segment fits)
          stage(x);
          stg.commit(4u * total);
          continue;
        }
        // ---- the step's ids do not fit the tile together, or a run is a long one: runs of lanes that fit and hold no long run, each flushed;
        // a long run goes to the whole wavefront
        stg.flush_units();
        uint32_t done = 0, first = 0;  // ids of the step staged so far; the first lane not staged yet
        while (first < 64u) {
          const unsigned long long behind = BIG & (~0ull << first);
          const uint32_t fb = behind ? (uint32_t)__ffsll((long long)behind) - 1u : 64u;  // the first long run at or behind `first`
          const bool mine = lane >= first && lane < fb && inc - done <= RST_SEG;  // (inc grows with the lane: the lanes that fit are first .. first + cnt - 1)
          const uint32_t cnt = (uint32_t)__popcll(ballot_b(mine));
          if (cnt == 0) {  // (lane `first` holds a long run: whatever is shorter fits a segment alone)
            const uint32_t plen = uni(__shfl(len, (int)first)), prb = uni(__shfl(rb, (int)first)), pre = uni(__shfl(re, (int)first));
            bytefb_copy_long(stg, s, nbytes, prb, pre, bin.first, in.reverse != 0, lane);
            stg.flush_units();
            done += plen;
            first += 1;
            continue;
          }
          const uint32_t n = uni(__shfl(inc, (int)(first + cnt - 1))) - done;
          if (mine) stage(x - done);
          stg.commit(4u * n);
          stg.flush_units();
          done += n;
          first += cnt;
        }
      }
    }
    if (WRITE) {
      stg.close();
    } else if (g0 + lane < g1) {
      out_len[g0 + lane] = my_len;
    }
  }
  if (!WRITE && saw_any && lane == 0) *saw = 1u;
}

// each pass is given what it uses; out: 16-byte aligned, out_off: the exclusive scan of out_len, in ids; *saw holds 0 before the measure pass
void launch_bytefb(bool write, const EncModel &m, const SubInput &in, int32_t first, unsigned long long n_ids, uint32_t *out_len, uint32_t *saw,
                   const unsigned long long *out_off, int32_t *out, hipStream_t st) {
  if (!in.n_sent) return;
  const unsigned int group = lane_group(in.n_sent, n_ids);
  const dim3 grid = grid_for_groups(in.n_sent, group), block(BLOCK);
  const ByteFbInput bin{in, first};
  if (write) hipLaunchKernelGGL((k_bytefb<true>), grid, block, 0, st, m, bin, group, (uint32_t *)nullptr, (uint32_t *)nullptr, out_off, out);
  else hipLaunchKernelGGL((k_bytefb<false>), grid, block, 0, st, m, bin, group, out_len, saw, (const unsigned long long *)nullptr, (int32_t *)nullptr);
}

}  // namespace yttm
