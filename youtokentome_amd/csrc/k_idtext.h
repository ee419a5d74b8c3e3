// k_idtext.h -- decimal id text on the device, both ways: the lines of a text -> the ids `while (ss >> x)` reads from each (k_idparse), and the
// pending encode result -> the text `yttm encode --output_type id` prints (k_idprint).  Included at the end of k_encode.hip (behind k_subword.h:
// the groups of the printer are its lane_group's).
//
// replaces: the parse of BaseEncoder::decode(const vector<string>&, ...) bpe.cpp:1863-1873 (`while (ss >> x) ids.push_back(x)` per line, restated
// in decode_cli, host_cli.cpp) and the id formatting of encode_cli bpe.cpp:1942-2014 (utils.h:92-103: every id followed by one space, then
// '\n'), for a whole text / batch at once.
//
// ---- the parser.  WS = 0x20, 0x09 .. 0x0D; a digit '0' .. '9'; a sign '+' '-'; every other byte (NUL and bytes >= 0x80 too) is "other".  A
// NUMBER is a maximal run of digits, its value the run read as decimal, negated iff the byte just before the run is '-'.  A FAIL POINT is an
// "other" byte, a sign whose next byte in the line is not a digit, or the first digit of a number whose signed value lies outside int32.  The
// ids of a line are the numbers that start before the line's first fail point; nothing carries over to the next line.
// A number and a fail point never overlap, so "starts before the first fail point" is decided where the number ENDS (its last digit), where
// its value is complete: kept iff no fail point lies in the line at or before that byte, its own overflow included.
// Three steps on the lane's stream, no atomic:
//   measure  k_idparse<false>: count[line] = kept numbers of the line
//   scan     launch_exclusive_scan(count) -> out_off[n_lines + 1]                                                   (k_frontend.hip)
//   write    k_idparse<true>: the kept numbers of a group, in byte order, at ids[out_off[first line of the group] ..)
// Algorithmic bytes (N text bytes, n lines, K ids): read N + 8 (n + 1), written 4 K + 8 (n + 1) (the write pass reads the text again).
//
// Mapping: a wavefront takes a GROUP of consecutive lines -- their bytes are contiguous, text[off[g0] .. off[g1]), and so are their ids -- and
// walks those bytes 64 a step, a lane per byte, ACROSS the lines: a newline is the one byte that ends a line, so the line of a byte is the
// number of newlines in front of it and a group may hold any number of lines.  The classes are ballots; the length of the digit run that ends
// in a lane comes from the digit mask, its value from one shuffle per digit of the step's longest run.  What crosses a step: whether the step
// ended inside a run, that run's value so far -- saturating at 2^31 + 1, it never wraps --, its sign (or, outside a run, whether the last
// byte was '-'), whether the open line has failed, and the open line's count.  One byte ahead of the step is read to know whether a run or a
// sign in lane 63 goes on.
// Limits: a line below 4 G numbers; a single line is walked by one wavefront.
//
// ---- the printer.  Per sentence every id in decimal ('-' for a negative one, -2147483648 included) followed by one space, then '\n'.
// measure -> scan -> write as k_subword.h, a lane per id of one sentence at a time; the digits go through the tile writer
// (k_textout.h).  Algorithmic bytes: read 4 K + 8 (S + 1), written B_out + 8 (S + 1).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_subword.h"

namespace yttm {

constexpr unsigned long long IDP_SAT = 0x80000001ull;  // every magnitude above 2^31, the largest one an int32 has

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_idparse(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ loff, unsigned long long n_lines,
                                                   unsigned int group, uint32_t *__restrict__ count, const unsigned long long *__restrict__ out_off,
                                                   int32_t *__restrict__ ids) {
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  const unsigned long long lt = lanemask_lt(), le = lt | (1ull << lane);
  for (WaveGroups wg(n_lines, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const unsigned long long k0 = uni64(loff[g0]), k1 = uni64(loff[g1]);
    // what crosses a step; a group starts behind a newline (or at the text's start): all clear
    bool c_digit = false, c_neg = false, c_fail = false;
    unsigned long long c_val = 0;
    uint32_t c_cnt = 0;
    unsigned long long line = g0;  // the line that is open at the step's first byte
    unsigned long long opos = WRITE ? uni64(out_off[g0]) : 0ull;
    for (unsigned long long b0 = k0; b0 < k1; b0 += 64) {
      const unsigned long long i = b0 + lane;
      const bool inside = i < k1;
      const uint32_t b = inside ? (uint32_t)text[i] : 0x20u;
      const bool ahead_digit = b0 + 64 < k1 && (uint32_t)text[b0 + 64] - (uint32_t)'0' < 10u;  // (uniform: one byte, every lane the same)
      const uint32_t dg = b - (uint32_t)'0';
      const bool is_d = dg < 10u, is_s = b == (uint32_t)'+' || b == (uint32_t)'-', is_ws = b == 0x20u || (b >= 9u && b <= 13u);
      const unsigned long long D = ballot_b(is_d), NL = ballot_b(b == 0x0au), M = ballot_b(b == (uint32_t)'-');
      const bool next_d = (((D >> 1) | (ahead_digit ? 1ull << 63 : 0ull)) >> lane) & 1ull;
      // the digits of the run up to this lane, inside the step
      const unsigned long long nd_below = ~D & lt;
      const uint32_t len = !is_d ? 0u : nd_below ? lane - (uint32_t)(63 - __clzll((long long)nd_below)) : lane + 1u;
      unsigned long long val = 0, p10 = 1;
      bool big = false;
      for (uint32_t k = 0; ballot_b(len > k) != 0ull; k++) {  // (as many turns as the step's longest run has digits)
        const uint32_t dk = __shfl(dg, (int)((lane - k) & 63u));
        if (len > k) {
          if (k < 10u) val += (unsigned long long)dk * p10;
          else big = big || dk != 0u;
        }
        if (k < 10u) p10 *= 10ull;
      }
      if (big || val > IDP_SAT) val = IDP_SAT;
      // the run that began in a step before goes on in lane 0: its value so far in front of this step's len0 digits
      if (c_digit && (D & 1ull)) {
        const uint32_t len0 = ~D ? (uint32_t)__ffsll((long long)~D) - 1u : 64u;
        unsigned long long p = 1;
        for (uint32_t j = 0; j < len0 && j < 10u; j++) p *= 10ull;
        if (is_d && len == lane + 1u && c_val != 0ull) {
          const unsigned long long v = c_val * p + val;  // (c_val <= 2^31 + 1 and p <= 10^9: no wrap)
          val = len0 > 9u || v > IDP_SAT ? IDP_SAT : v;
        }
      }
      const uint32_t start = lane + 1u - len;  // (of a digit lane's run; 0: it began at or in front of the step's first byte)
      const bool neg = is_d && (start > 0u ? ((M >> (start - 1u)) & 1ull) != 0ull : c_neg);
      const bool end = is_d && !next_d;
      const bool overflow = end && (neg ? val > 0x80000000ull : val > 0x7fffffffull);
      const unsigned long long F = ballot_b((inside && !is_d && !is_s && !is_ws) || (is_s && !next_d) || overflow);
      // this lane's line inside the step: behind the last newline below the lane
      const unsigned long long nl_below = NL & lt;
      const unsigned long long mine = nl_below ? ~((2ull << (63 - __clzll((long long)nl_below))) - 1ull) : ~0ull;
      const bool failed = (F & le & mine) != 0ull || (!nl_below && c_fail);
      const bool kept = end && !failed;
      const unsigned long long K = ballot_b(kept);
      if (!WRITE) {
        if (b == 0x0au) count[line + (unsigned long long)__popcll(nl_below)] = (uint32_t)__popcll(K & lt & mine) + (nl_below ? 0u : c_cnt);
      } else if (kept) {
        ids[opos + (unsigned long long)__popcll(K & lt)] = (int32_t)(neg ? 0u - (uint32_t)val : (uint32_t)val);
      }
      // ---- carries
      if (NL) {
        const unsigned long long above = ~((2ull << (63 - __clzll((long long)NL))) - 1ull);  // behind the step's last newline (none for lane 63)
        c_cnt = (uint32_t)__popcll(K & above);
        c_fail = (F & above) != 0ull;
        line += (unsigned long long)__popcll(NL);
      } else {
        c_cnt += (uint32_t)__popcll(K);
        c_fail = c_fail || F != 0ull;
      }
      opos += (unsigned long long)__popcll(K);
      c_digit = (D >> 63) != 0ull;
      const unsigned long long v63 = ((unsigned long long)__shfl((uint32_t)(val >> 32), 63) << 32) | (unsigned long long)__shfl((uint32_t)val, 63);
      const bool n63 = __shfl((int)neg, 63) != 0;
      c_val = c_digit ? v63 : 0ull;
      c_neg = c_digit ? n63 : (M >> 63) != 0ull;
    }
    if (!WRITE && line < g1 && lane == 0) count[line] = c_cnt;  // the text's last line has no newline
  }
}

// each pass is given what it uses
void launch_idparse(bool write, const uint8_t *text, const unsigned long long *loff, unsigned long long n_lines, unsigned long long n_bytes, uint32_t *count,
                    const unsigned long long *out_off, int32_t *ids, hipStream_t st) {
  if (!n_lines) return;
  const unsigned int group = group_size(n_lines, n_bytes, 4096, 1u << 20);  // lines per group: about 4 KB of text
  const dim3 grid = grid_for_groups(n_lines, group), block(BLOCK);
  if (write) hipLaunchKernelGGL((k_idparse<true>), grid, block, 0, st, text, loff, n_lines, group, (uint32_t *)nullptr, out_off, ids);
  else hipLaunchKernelGGL((k_idparse<false>), grid, block, 0, st, text, loff, n_lines, group, count, (const unsigned long long *)nullptr, (int32_t *)nullptr);
}

// ---- the printer -------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t IDT_MAX = 12;  // bytes of one id at most: '-', ten digits, the space
static_assert(SUB_FLUSH + 64 * IDT_MAX <= (uint32_t)DEC_TILE, "a step's 64 ids fit behind SUB_FLUSH - 1 staged bytes");

__device__ inline uint32_t idt_digits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_idprint(const int32_t *__restrict__ ids, const unsigned long long *__restrict__ ioff, unsigned long long n_sent,
                                                   unsigned int group, uint32_t *__restrict__ out_len, const unsigned long long *__restrict__ out_off,
                                                   uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[WRITE ? NWAVES : 1][WRITE ? DEC_TILE : 16];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  for (WaveGroups wg(n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const LaneBounds ib(ioff, g0, g1, lane);
    uint32_t my_len = 0;  // (measure) lane j: the output bytes of sentence g0 + j
    TileWriter stg(s_tile[WRITE ? w : 0], lane);
    if (WRITE) stg.open(out, uni64(out_off[g0]));
    for (unsigned long long sidx = g0; sidx < g1; sidx++) {
      const int j = (int)(sidx - g0);
      const unsigned long long i0 = ib.at(j), i1 = ib.at(j + 1);
      uint32_t acc = 0;
      for (unsigned long long base = i0; base < i1; base += 64) {
        const unsigned long long k = base + lane;
        const bool inside = k < i1;
        const int32_t id = inside ? ids[k] : 0;
        const bool neg = id < 0;
        uint32_t v = neg ? 0u - (uint32_t)id : (uint32_t)id;
        const uint32_t nd = idt_digits(v);
        const uint32_t olen = inside ? nd + (neg ? 1u : 0u) + 1u : 0u;  // (+ the space behind every id)
        if (!WRITE) {
          acc += olen;
          continue;
        }
        const uint32_t inc = wave_incl_scan(olen);
        const uint32_t x = inc - olen, total = uni(__shfl(inc, 63));
        if (!stg.fits(total)) stg.flush_units();
        if (inside) {
          uint8_t *p = stg.at(x);
          if (neg) *p++ = (uint8_t)'-';
          uint8_t *q = p + nd;
          *q = (uint8_t)' ';
          do {
            *--q = (uint8_t)('0' + v % 10u);
            v /= 10u;
          } while (q > p);
        }
        stg.commit(total);
        stg.flush_if_due();
      }
      if (!WRITE) {
        const uint32_t total = uni(__shfl(wave_incl_scan(acc), 63)) + 1u;  // + the newline
        if (lane == (uint32_t)j) my_len = total;
        continue;
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

// each pass is given what it uses
void launch_idprint(bool write, const int32_t *ids, const unsigned long long *ioff, unsigned long long n_sent, unsigned long long n_ids, uint32_t *out_len,
                    const unsigned long long *out_off, uint8_t *out, hipStream_t st) {
  if (!n_sent) return;
  const unsigned int group = lane_group(n_sent, n_ids);
  const dim3 grid = grid_for_groups(n_sent, group), block(BLOCK);
  if (write) hipLaunchKernelGGL((k_idprint<true>), grid, block, 0, st, ids, ioff, n_sent, group, (uint32_t *)nullptr, out_off, out);
  else hipLaunchKernelGGL((k_idprint<false>), grid, block, 0, st, ids, ioff, n_sent, group, out_len, (const unsigned long long *)nullptr, (uint8_t *)nullptr);
}

}  // namespace yttm
