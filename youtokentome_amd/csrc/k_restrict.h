// k_restrict.h -- the vocabulary restriction on the device: ids + offsets -> every id replaced by its expansion E(id) (the rule is in
// include/yttm_mi355x.h "Encode under a restricted vocabulary").  Included at the end of k_encode.hip like its siblings.
//
// The expansion of every id of [0, V) lives in HBM as exp_ids[] + exp_off[V + 1] (host_encoder.cpp builds both, and a second exp_ids with every
// expansion back to front for sentences that are stored back to front); an id that stays has the expansion [id], an id outside [0, V) is not
// looked up and passes through.  At vocab 32 000 the tables are a few hundred KB and stay in L2 like the decode's piece table.  Three steps on
// the lane's stream, the shape of k_decode.h:
//   measure  k_restrict<false>: out_len[s] = the sum of the expansion lengths of sentence s
//   scan     launch_exclusive_scan(out_len) -> out_off[S + 1], in ids                                                 (k_frontend.hip)
//   write    k_restrict<true>: the expansions -> LDS staging tile -> the output in aligned 16-byte stores
// No global atomics.  Where the scan's total equals the number of ids nothing splits (every expansion has at least one id, and one of length
// one is the id itself): the host skips the write pass.
// Algorithmic bytes (K_in ids, K_out ids, S sentences): read 4 K_in + 8 (S + 1), written 4 K_out + 8 (S + 1) (+ 4 S of out_len written, read
// and scanned in between), plus the table traffic, which stays in L2.
//
// Mapping (as k_decode.h): a wavefront takes a GROUP of consecutive sentences and walks the group's ids 64 at a time ACROSS sentence
// boundaries, a lane per id.  The output of a group is contiguous, so the write pass needs no boundary at all; the measure pass closes every
// sentence whose boundary lies in the step from the prefix sums of the step's lengths.
// The tile: the TileWriter of k_textout.h with 4-byte elements -- every position it is asked for is a multiple of 4 (the cursor is 4 * an id
// offset, every commit 4 * a number of ids), so at() is word aligned and the lanes stage whole words; its byte stores are the up to 12 bytes
// of a 16-byte unit that two groups share.  A step whose expansions do not fit the tile together is staged in runs of lanes that do; an
// expansion longer than the tile is copied by the whole wavefront in segments (restrict_copy_long), as copy_piece does for long pieces.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_textout.h"
#include "yttm_kernels.h"

namespace yttm {

constexpr uint32_t RST_SEG = (uint32_t)DEC_SEG / 4u;  // most ids staged at once (508): fits behind an unfinished 16-byte unit
static_assert(RST_SEG * 4u <= (uint32_t)DEC_SEG && RST_SEG >= 64u, "a step of 64 ids that stay fits the tile at once");

// One expansion of any length, copied by the whole wavefront in segments of RST_SEG ids, each flushed: fewer than 16 bytes stay staged.
__device__ inline void restrict_copy_long(TileWriter &stg, const int32_t *__restrict__ src, uint32_t n_ids, uint32_t lane) {
  for (uint32_t done = 0; done < n_ids;) {
    const uint32_t n = n_ids - done < RST_SEG ? n_ids - done : RST_SEG;
    if (!stg.fits(4u * n)) stg.flush_units();
    int32_t *const p = reinterpret_cast<int32_t *>(stg.at(0));
    for (uint32_t b = lane; b < n; b += 64) p[b] = src[done + b];
    stg.commit(4u * n);
    stg.flush_units();
    done += n;
  }
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_restrict(const int32_t *__restrict__ ids, const unsigned long long *__restrict__ off, unsigned long long n_sent,
                                                    RestrictTable tb, unsigned int group, uint32_t *__restrict__ out_len,
                                                    const unsigned long long *__restrict__ out_off, int32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[WRITE ? NWAVES : 1][WRITE ? DEC_TILE : 16];
  __shared__ uint32_t s_xs[WRITE ? 1 : NWAVES][WRITE ? 1 : 65];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  for (WaveGroups wg(n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const unsigned long long k0 = uni64(off[g0]), k1 = uni64(off[g1]);
    unsigned long long sc = g0;    // (measure) the first boundary (start of sentence sc) that lies at or behind `base`
    uint32_t run = 0, open_p = 0;  // (measure) output ids of the group before this step; ... before the start of the sentence still open
    TileWriter stg(s_tile[WRITE ? w : 0], lane);
    if (WRITE) stg.open(reinterpret_cast<uint8_t *>(out), 4ull * uni64(out_off[g0]));
    for (unsigned long long base = k0;; base += 64) {
      const bool last = base + 64 >= k1;
      // ---- this lane's id and its expansion: exp_ids[src .. src + len), or the id itself where it is outside [0, vocab)
      const unsigned long long k = base + lane;
      const bool inside = k < k1;
      const int32_t id = inside ? ids[k] : 0;
      const bool oor = (uint32_t)id >= tb.vocab;  // (unsigned: a negative id is outside)
      uint32_t src = 0, len = 0;
      if (inside) {
        len = 1;
        if (!oor) {
          src = tb.exp_off[id];
          len = tb.exp_off[id + 1] - src;
        }
      }
      const uint32_t inc = wave_incl_scan(len);
      const uint32_t x = inc - len, total = uni(__shfl(inc, 63));
      const auto stage = [&](uint32_t at) {  // this lane's expansion, `at` ids behind the staged ones
        int32_t *const p = reinterpret_cast<int32_t *>(stg.at(4u * at));
        if (oor) {
          if (inside) p[0] = id;
        } else {
          for (uint32_t b = 0; b < len; b++) p[b] = tb.exp_ids[src + b];
        }
      };
      if (!WRITE) {
        // ---- every boundary in [base, base + 64) (the last step: every one left) closes a sentence: its length is a difference of prefixes
        s_xs[w][lane] = x;
        if (lane == 0) s_xs[w][64] = total;
        wave_sync();
        for (;;) {
          const unsigned long long s = sc + lane;
          const bool have = s <= g1;
          const unsigned long long v = have ? off[s] : ~0ull;
          const bool res = have && (v < base + 64 || last);
          const uint32_t cnt = (uint32_t)__popcll(ballot_b(res));  // (boundaries are sorted: the resolved ones are lanes 0 .. cnt-1)
          if (cnt == 0) break;
          const uint32_t pfx = res ? run + s_xs[w][(uint32_t)(v - base)] : 0u;
          const uint32_t next = __shfl_down(pfx, 1);
          if (res && lane + 1 < cnt) out_len[s] = next - pfx;
          if (lane == 0 && sc > g0) out_len[sc - 1] = pfx - open_p;
          open_p = uni(__shfl(pfx, (int)cnt - 1));
          sc += cnt;
          if (cnt < 64) break;
        }
        wave_sync();
        run += total;
      } else if (total <= RST_SEG) {  // (every step ends with flush_units: DEC_SEG more bytes fit)
        stage(x);
        stg.commit(4u * total);
        stg.flush_units();
      } else {
        // ---- the step's expansions do not fit the tile together: runs of lanes whose expansions do, each flushed; a lane whose expansion
        // alone is longer than a segment hands it to the whole wavefront
        uint32_t done = 0, first = 0;  // ids of the step staged so far; the first lane not staged yet
        while (done < total) {
          const bool mine = lane >= first && inc - done <= RST_SEG;  // (inc grows with the lane: the lanes that fit are first .. first + cnt - 1)
          const uint32_t cnt = (uint32_t)__popcll(ballot_b(mine));
          if (cnt == 0) {
            const uint32_t plen = uni(__shfl(len, (int)first)), psrc = uni(__shfl(src, (int)first));
            restrict_copy_long(stg, tb.exp_ids + psrc, plen, lane);
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
      if (last) break;
    }
    if (WRITE) stg.close();
  }
}

// each pass is given what it uses; out: 16-byte aligned, out_off: the exclusive scan of out_len, in ids
void launch_restrict(bool write, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent, unsigned long long n_ids,
                     const RestrictTable &tb, uint32_t *out_len, const unsigned long long *out_off, int32_t *out, hipStream_t st) {
  if (!n_sent) return;
  const unsigned int group = group_size(n_sent, n_ids, 256, 64);  // (a group may hold any number of sentences: the boundaries are read 64 at a time)
  const dim3 grid = grid_for_groups(n_sent, group), block(BLOCK);
  if (!write) hipLaunchKernelGGL((k_restrict<false>), grid, block, 0, st, ids, off, n_sent, tb, group, out_len, nullptr, nullptr);
  else hipLaunchKernelGGL((k_restrict<true>), grid, block, 0, st, ids, off, n_sent, tb, group, nullptr, out_off, out);
}

}  // namespace yttm
