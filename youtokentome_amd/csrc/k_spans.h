// k_spans.h -- byte spans on the device: the ids K5 left + the sentences' text -> for every id the bytes of the sentence it stands for.
// Included at the end of k_encode.hip (behind k_subword.h: the groups of sentences are its lane_group's, the classification of a byte is enc_classify).
//
// The rule.  Read through enc_classify, a sentence is a sequence of UNITS: a valid non-space char of the alphabet is one, and so is a maximal run
// of valid chars outside the alphabet that no space and no alphabet char interrupts (invalid bytes do not end a run: SURVEY.md A.7).  A unit
// starts at the first byte of its first char and ends one past the last byte of its last valid char.  Token t covers u(t) units -- piece_units[t],
// filled by the host (host_decode.cpp): 1 for unk_id, else the code points of id_to_subword(t, false) other than U+2581 -- so with a_k the
// exclusive prefix sum of u over the sentence's ids in FORWARD order, token k has the span [start(unit a_k), end(unit a_k + u - 1)), and a token
// without units ("▁" alone, <PAD>, <BOS>, <EOS>) the empty span (p, p), p = start(unit a_k), or the end of the last unit where there is no
// such unit (0 in a sentence without units).  With `reverse` K5 stored the ids back to front: stored id k is forward token n - 1 - k, and span k
// belongs to stored id k.  The sum of u equals the number of units; a sentence where it does not raises *bad (an internal error of the host call).
//
// One pass, no global atomic: the output is 8 bytes per id at the id's own index.
// Algorithmic bytes (N text bytes, K ids, S sentences): read N + 4 K + 16 (S + 1), written 8 K.  (Not counted: piece_units, which stays in L2.)
//
// Mapping: a wavefront takes a GROUP of consecutive sentences (lane_group) and walks one after the other as a merge of two monotone sequences:
//   the id tiles    64 ids at a time, a lane per id: u, then A = a_k (wave scan + the tiles before) and E = A + u - 1;
//   the text steps  64 bytes at a time, a lane per byte: ST = the lanes where a unit starts, LAST = the lanes of the last char in the step of
//                   each unit that has a char in it -- bit j of ST is unit ub + j, bit j of LAST unit ub - cont + j (cont: the step opens inside
//                   the unknown run the steps before left open).
// A token takes its start from the step that holds unit A (the lane of the (A - ub)-th bit of ST) and its end from every step that holds a char
// of unit E (the lane of that bit of LAST + the char's length, handed over by a shuffle; a later step of the same run overwrites it).  The tile
// is stored once every token of it is final -- its last unit is behind it, closed by a space or a known char, or the text is at its end --,
// else the next step is read; the step's masks stay in scalar registers while the tiles advance, so text and ids are each read once and no LDS
// is needed.  Carried across the steps: whether the last valid char was unknown (the open run), the units so far, the end of the last unit.
// Limits: a sentence below 4 GB; a single sentence is walked by one wavefront.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_subword.h"

namespace yttm {

// the lane of the n-th set bit of mask (n < popcount(mask); anything else gives a lane below 64)
__device__ inline uint32_t spn_select(unsigned long long mask, uint32_t n) {
  uint32_t pos = 0;
  uint32_t c = (uint32_t)__popc((uint32_t)mask);
  uint32_t w = (uint32_t)mask;
  if (n >= c) {
    n -= c;
    pos = 32;
    w = (uint32_t)(mask >> 32);
  }
  for (uint32_t half = 16; half; half >>= 1) {
    c = (uint32_t)__popc(w & ((1u << half) - 1u));
    if (n >= c) {
      n -= c;
      pos += half;
      w >>= half;
    }
  }
  return pos & 63u;
}

__global__ __launch_bounds__(BLOCK) void k_spans(EncModel m, SubInput in, const uint32_t *__restrict__ piece_units, uint32_t vocab, unsigned int group,
                                                 unsigned long long *__restrict__ spans, uint32_t *__restrict__ bad) {
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt();
  for (WaveGroups wg(in.n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds ib(in.ioff, g0, g1, lane), sb(in.soff, g0, g1, lane);
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long i0 = ib.at(j), i1 = ib.at(j + 1);
      const unsigned long long t0 = sb.at(j), nbytes = sb.at(j + 1) - t0;
      const uint8_t *s = in.text + t0;
      // ---- the text side: the step at hand and what the steps so far carry
      unsigned long long next_b0 = 0;      // first byte of the step to read next
      unsigned long long ST = 0, LAST = 0;  // the step at hand (none yet: no unit)
      uint32_t sb0 = 0, ub = 0, cont = 0;   // its first byte; units in front of it; 1: its first LAST bit is the run left open before it
      uint32_t clen = 0;                    // this lane's char of the step: its bytes
      uint32_t units = 0, last_end = 0;     // units so far (ub + those of the step); the end of the last of them so far
      bool open = false;                    // the last valid char so far was an unknown one: the last unit may go on
      auto next_step = [&]() {
        const unsigned long long i = next_b0 + lane;
        EncChar c;
        enc_classify(m, s, i, nbytes, c);
        const unsigned long long V = ballot_b(c.valid), U = ballot_b(c.unk);
        bool prev_unk = open;
        const unsigned long long pv = V & lt;
        if (pv) prev_unk = (U >> (63 - __clzll((long long)pv))) & 1ull;
        const unsigned long long nv = V & ~lt & ~(1ull << lane);  // the valid chars behind this one
        const bool next_unk = nv && ((U >> (__ffsll((long long)nv) - 1)) & 1ull);
        const bool body = c.valid && !c.space;
        ST = ballot_b(body && !(c.unk && prev_unk));
        LAST = ballot_b(body && !(c.unk && next_unk));
        clen = c.len;
        sb0 = (uint32_t)next_b0;
        ub = units;
        // the first char of the step that is no space goes on with the open run iff it is a unit's char and starts none
        const unsigned long long B = ballot_b(body);
        cont = (B && !((ST >> (__ffsll((long long)B) - 1)) & 1ull)) ? 1u : 0u;
        units += (uint32_t)__popcll(ST);
        const uint32_t hl = LAST ? (uint32_t)(63 - __clzll((long long)LAST)) : 0u;
        const uint32_t hlen = uni(__shfl(clen, (int)hl));
        if (LAST) last_end = sb0 + hl + hlen;
        if (V) open = (U >> (63 - __clzll((long long)V))) & 1ull;
        next_b0 += 64;
      };
      // ---- the id side
      const unsigned long long n_tok = i1 - i0;
      uint32_t a_base = 0;  // units of the tokens in front of the tile
      for (unsigned long long base = 0; base < n_tok; base += 64) {
        const unsigned long long f = base + lane;  // forward index of this lane's token
        const bool inside = f < n_tok;
        const unsigned long long k = in.reverse ? i1 - 1 - f : i0 + f;
        const int32_t id = inside ? in.ids[k] : 0;
        const uint32_t u = inside && (uint32_t)id < vocab ? piece_units[id] : 0u;
        const uint32_t inc = wave_incl_scan(u);
        const uint32_t A = a_base + inc - u, E = A + u - 1u;  // (E only where u > 0)
        a_base += uni(__shfl(inc, 63));
        uint32_t start = 0, end = 0;
        bool have_start = false, have_end = false;
        for (;;) {
          // what the step at hand holds for this tile
          const uint32_t cnt = (uint32_t)__popcll(ST);
          const uint32_t ra = A - ub, re = E - (ub - cont);
          const bool want_s = inside && !have_start && A >= ub && ra < cnt;
          const bool want_e = inside && u > 0 && E + cont >= ub && re < cnt + cont;
          const uint32_t ps = spn_select(ST, want_s ? ra : 0u), pe = spn_select(LAST, want_e ? re : 0u);
          const uint32_t le = __shfl(clen, (int)pe);
          if (want_s) {
            start = sb0 + ps;
            have_start = true;
          }
          if (want_e) {
            end = sb0 + pe + le;
            have_end = true;
          }
          const bool text_done = next_b0 >= nbytes;
          const bool settled = !inside || text_done || (u > 0 ? have_end && (E + 1u < units || !open) : have_start);
          if (!ballot_b(!settled)) break;
          next_step();
        }
        // the text is at its end and something is missing: a token without units behind the last unit, or ids that do not fit the text
        if (inside) {
          if (u == 0) {
            if (!have_start) {
              start = last_end;
              if (A != units) *bad = 1u;
            }
            end = start;
          } else if (!have_start || !have_end) {
            start = end = 0;
            *bad = 1u;
          }
          spans[k] = (unsigned long long)start | ((unsigned long long)end << 32);  // one 8-byte store per id: (start, end)
        }
      }
      while (next_b0 < nbytes) next_step();  // (white space and invalid bytes behind the last token's unit, or units no id stands for)
      if (units != a_base && lane == 0) *bad = 1u;
    }
  }
}

// spans + ioff -> row-major [n_sent, width][2] (tail of a row = (0, 0)), an 8-byte store per element.  Rows must fit (the host checks first).
__global__ __launch_bounds__(BLOCK) void k_spans_pad(const unsigned long long *__restrict__ spans, const unsigned long long *__restrict__ ioff,
                                                     unsigned long long n_sent, unsigned long long width, unsigned long long *__restrict__ matrix) {
  const unsigned long long total = n_sent * width;
  for (unsigned long long e = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * BLOCK) {
    const unsigned long long row = e / width, col = e - row * width, o = ioff[row];
    matrix[e] = col < ioff[row + 1] - o ? spans[o + col] : 0ull;
  }
}

void launch_spans(const EncModel &m, const SubInput &in, const uint32_t *piece_units, uint32_t vocab, unsigned long long n_ids, uint32_t *spans, uint32_t *bad,
                  hipStream_t st) {
  if (!in.n_sent) return;
  const unsigned int group = lane_group(in.n_sent, n_ids);
  hipLaunchKernelGGL(k_spans, grid_for_groups(in.n_sent, group), dim3(BLOCK), 0, st, m, in, piece_units, vocab, group, (unsigned long long *)spans, bad);
}
void launch_spans_pad(const uint32_t *spans, const unsigned long long *ioff, unsigned long long n_sent, unsigned long long width, uint32_t *matrix,
                      hipStream_t st) {
  if (!n_sent || !width) return;
  unsigned long long b = (n_sent * width + BLOCK - 1) / BLOCK;
  if (b > 256 * 16) b = 256 * 16;
  hipLaunchKernelGGL(k_spans_pad, dim3((unsigned int)b), dim3(BLOCK), 0, st, (const unsigned long long *)spans, ioff, n_sent, width,
                     (unsigned long long *)matrix);
}

}  // namespace yttm
