// k_decode.h -- device decode (ids -> text) and the padded form of the encoder's result.  Included at the end of k_encode.hip.
//
// replaces: BaseEncoder::decode(const vector<int>&, ...) bpe.cpp:1843-1861 on top of id_to_subword(id, &s, true) bpe.cpp:1774-1807, for a whole batch.
//
// The text of every id lives in HBM as one blob + piece_off[V + 1] (host_decode.h fills it from the host's id_to_subword, so there is one definition
// of a piece's text); at vocab 32 000 that is a few hundred KB and stays in L2.  Three steps on the lane's stream, none waits for another's progress:
//   measure  k_decode<PADDED, false>: out_len[s] = sum of the kept pieces' lengths - the strip byte; the smallest flat index of an id that is
//            neither ignored nor valid goes to *bad_min (one 64-bit atomicMin per workgroup that saw one; the host reads it after the stream's sync)
//   scan     launch_exclusive_scan(out_len) -> out_off[S + 1]                                                      (k_frontend.hip)
//   write    k_decode<PADDED, true>: the pieces' bytes -> LDS staging tile -> the output blob in aligned 16-byte stores
// Algorithmic bytes (K ids, S sentences, B_out output bytes): read 4 K + 8 (S + 1), written B_out + 8 (S + 1) (+ 4 S of out_len written, read and
// scanned in between), plus the table traffic, which stays in L2.
//
// Mapping (as K5): a wavefront takes a GROUP of consecutive sentences -- one long sentence, or several short ones -- and walks the group's ids
// 64 at a time ACROSS sentence boundaries: a lane holds one id, whatever sentence it belongs to.  The output of a group is contiguous (out_off is
// a scan in sentence order), so the write pass needs the sentence boundaries for one thing only: which id is the first KEPT one of its sentence
// (the strip rule).  Boundaries are read 64 at a time by the lanes (offsets[s], or s * row_stride for a padded matrix) and turned into a lane mask.
// Limit: a single sentence is walked by one wavefront, 64 ids a step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_textout.h"
#include "yttm_kernels.h"

namespace yttm {

__device__ inline unsigned long long dec_bpos(const DecInput &in, unsigned long long s) { return in.offsets ? in.offsets[s] : s * in.stride; }

// NL (ragged input only): a '\n' behind every sentence, as decode_cli writes its lines -- out_len[s] counts it, the write pass puts the newlines of
// the sentences that END at a position (every boundary but the group's first one; empty sentences: several) in front of that position's piece,
// and those of a boundary that no step reaches (the group ends exactly on a step's end) behind the last step.
template <bool PADDED, bool WRITE, bool NL = false>
__global__ __launch_bounds__(BLOCK) void k_decode(DecInput in, DecTable tb, DecIgnore ig, unsigned int group, uint32_t *__restrict__ out_len,
                                                  unsigned long long *__restrict__ bad_min, const unsigned long long *__restrict__ out_off,
                                                  uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[WRITE ? NWAVES : 1][WRITE ? DEC_TILE : 16];
  __shared__ uint32_t s_xs[NWAVES][65];
  __shared__ uint32_t s_flag[NWAVES][64];
  __shared__ uint32_t s_nl[NL && WRITE ? NWAVES : 1][NL && WRITE ? 64 : 1];
  __shared__ unsigned long long s_bad[NWAVES];
  const int w = uni((int)(threadIdx.x >> 6));
  const uint32_t lane = (uint32_t)lane_id();
  unsigned long long bad = ~0ull;
  for (WaveGroups wg(in.n_sent, group, w); wg.more(); wg.next()) {
    const unsigned long long g0 = wg.g0(), g1 = wg.g1();
    const unsigned long long k0 = uni64(dec_bpos(in, g0)), k1 = uni64(dec_bpos(in, g1));
    unsigned long long sc = g0;              // the first boundary (start of sentence sc) that lies at or behind `base`
    unsigned long long rowb = g0, colb = 0;  // (PADDED) row and column of `base`
    uint32_t run = 0, open_p = 0;            // (measure) output bytes of the group before this step; ... before the start of the sentence still open
    bool carry = false;                      // the sentence that is open at `base` has a kept id already
    uint32_t nl_left = NL ? (uint32_t)(g1 - g0) : 0u;  // (NL, write) newlines of the group not yet staged
    TileWriter stg(s_tile[WRITE ? w : 0], lane);
    if (WRITE) stg.open(out, uni64(out_off[g0]));
    for (unsigned long long base = k0;; base += 64) {
      const bool last = base + 64 >= k1;
      // ---- this lane's id
      const unsigned long long k = base + lane;
      bool inside = k < k1;
      if (PADDED) {
        const unsigned long long rel = colb + lane;
        const unsigned long long q = in.stride >= 64 ? (rel >= in.stride ? 1ull : 0ull) : (unsigned long long)((uint32_t)rel / (uint32_t)in.stride);
        const unsigned long long row = rowb + q, col = rel - q * in.stride;
        unsigned long long row_len = in.width;
        if (inside && in.lengths) {  // (values outside [0, width] are clamped: a row never reaches into the next one)
          const int32_t l = in.lengths[row];
          row_len = l < 0 ? 0ull : ((unsigned long long)l < in.width ? (unsigned long long)l : in.width);
        }
        inside = inside && col < row_len;
      }
      const int32_t id = inside ? in.ids[k] : 0;
      const bool oor = (uint32_t)id >= tb.vocab;
      bool kept = inside;
      if (inside && ig.any) {  // the ignore set is asked before the range check (bpe.cpp:1850)
        bool ign = false;
        if (!oor) ign = (ig.bitmap[(uint32_t)id >> 5] >> ((uint32_t)id & 31u)) & 1u;
        else for (uint32_t j = 0; j < ig.n_extra; j++) ign = ign || ig.extra[j] == id;
        kept = !ign;
      }
      uint32_t src = 0, len = 0;
      if (kept) {
        bool invalid = oor;
        if (!oor) {
          src = tb.piece_off[id];
          const uint32_t end = tb.piece_off[id + 1] & ~DEC_INVALID;
          if (src & DEC_INVALID) invalid = true;
          else len = end - src;
        }
        if (invalid) {
          src = 0;
          if (k < bad) bad = k;
        }
      }
      // ---- sentence starts in [base, base + 64) as a lane mask
      s_flag[w][lane] = 0;
      if (NL && WRITE) s_nl[w][lane] = 0;
      wave_sync();
      unsigned long long hits = 0;
      for (unsigned long long s2 = sc;; s2 += 64) {
        const unsigned long long s = s2 + lane;
        const bool have = s <= g1;
        const unsigned long long v = have ? dec_bpos(in, s) : ~0ull;
        const bool hit = have && v < base + 64;
        if (hit && s < g1) s_flag[w][(uint32_t)(v - base)] = 1;
        if (NL && WRITE && hit && s > g0) atomicAdd(&s_nl[w][(uint32_t)(v - base)], 1u);
        const uint32_t cnt = (uint32_t)__popcll(ballot_b(hit));
        hits += cnt;
        if (cnt < 64) break;
      }
      wave_sync();
      const unsigned long long startmask = ballot_b(s_flag[w][lane] != 0), keptmask = ballot_b(kept);
      // ---- the strip rule: the first kept id of a sentence loses a leading space
      const unsigned long long lt = lanemask_lt();
      const unsigned long long at_or_before = startmask & (lt | (1ull << lane));
      const int p = at_or_before ? 63 - __clzll((long long)at_or_before) : -1;
      const unsigned long long kept_before = keptmask & lt & (p >= 0 ? ~((1ull << p) - 1ull) : ~0ull);
      const bool first = kept && kept_before == 0 && (p >= 0 || !carry);
      if (startmask) carry = (keptmask >> (63 - __clzll((long long)startmask))) != 0;
      else carry = carry || keptmask != 0;
      if (first && len > 0 && tb.blob[src] == (uint8_t)' ') {
        src++;
        len--;
      }
      const uint32_t nlb = NL && WRITE ? s_nl[w][lane] : 0u;  // newlines in front of this lane's piece
      const uint32_t inc = wave_incl_scan(len + nlb);
      const uint32_t x = inc - len, total = uni(__shfl(inc, 63));  // (x: where the piece goes, behind its newlines)
      if (!WRITE) {
        // ---- every boundary in [base, base + 64) (the last step: every one left) closes a sentence: its length is a difference of prefixes
        s_xs[w][lane] = x;
        if (lane == 0) s_xs[w][64] = total;
        wave_sync();
        for (;;) {
          const unsigned long long s = sc + lane;
          const bool have = s <= g1;
          const unsigned long long v = have ? dec_bpos(in, s) : ~0ull;
          const bool res = have && (v < base + 64 || last);
          const uint32_t cnt = (uint32_t)__popcll(ballot_b(res));  // (boundaries are sorted: the resolved ones are lanes 0 .. cnt-1)
          if (cnt == 0) break;
          const uint32_t pfx = res ? run + s_xs[w][(uint32_t)(v - base)] : 0u;
          const uint32_t next = __shfl_down(pfx, 1);
          if (res && lane + 1 < cnt) out_len[s] = next - pfx + (NL ? 1u : 0u);
          if (lane == 0 && sc > g0) out_len[sc - 1] = pfx - open_p + (NL ? 1u : 0u);
          open_p = uni(__shfl(pfx, (int)cnt - 1));
          sc += cnt;
          if (cnt < 64) break;
        }
        wave_sync();
        run += total;
      } else {
        sc += hits;
        if (total <= (uint32_t)DEC_SEG) {
          uint8_t *const nlp = stg.at(x - nlb), *const p = nlp + nlb;  // (every step ends with flush_units: DEC_SEG more bytes fit)
          if (NL) for (uint32_t b = 0; b < nlb; b++) nlp[b] = (uint8_t)'\n';
          for (uint32_t b = 0; b < len; b++) p[b] = tb.blob[src + b];
          stg.commit(total);
          stg.flush_units();
        } else {  // pieces that do not fit the tile together (a word of thousands of chars can be one piece): one by one, the wave copies a piece
          unsigned long long pm = ballot_b(len + nlb > 0);
          while (pm) {
            const int l = __ffsll((long long)pm) - 1;
            pm &= pm - 1;
            const uint32_t plen = uni(__shfl(len, l)), psrc = uni(__shfl(src, l));
            if (NL) stg.append_run((uint8_t)'\n', uni(__shfl(nlb, l)));  // (at most 64 newlines a step)
            stg.copy_piece(tb.blob + psrc, plen);
          }
        }
      }
      if (NL && WRITE) nl_left -= uni(__shfl(wave_incl_scan(nlb), 63));
      if (last) break;
      if (PADDED) {
        colb += 64;
        if (colb >= in.stride) {
          if (in.stride >= 64) {
            colb -= in.stride;
            rowb++;
          } else {
            rowb += (uint32_t)colb / (uint32_t)in.stride;
            colb = (uint32_t)colb % (uint32_t)in.stride;
          }
        }
      }
    }
    if (NL && WRITE && nl_left) stg.append_run((uint8_t)'\n', nl_left);
    if (WRITE) stg.close();
  }
  if (!WRITE) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long t = __shfl_down(bad, o);
      if (t < bad) bad = t;
    }
    if (lane == 0) s_bad[w] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long m = s_bad[0];
      for (int i = 1; i < NWAVES; i++) m = s_bad[i] < m ? s_bad[i] : m;
      if (m != ~0ull) atomicMin(bad_min, m);
    }
  }
}

// *bad_min must hold ~0 before the measure pass; each pass is given what it uses
void launch_decode(bool write, bool newline, const DecInput &in, const DecTable &tb, const DecIgnore &ig, unsigned long long n_flat, uint32_t *out_len,
                   unsigned long long *bad_min, const unsigned long long *out_off, uint8_t *out, hipStream_t st) {
  if (!in.n_sent) return;
  const unsigned int group = group_size(in.n_sent, n_flat, 256, 64);  // (a group may hold any number of sentences: the boundaries are read 64 at a time)
  const dim3 grid = grid_for_groups(in.n_sent, group), block(BLOCK);
  const bool padded = in.offsets == nullptr;
  if (write) out_len = nullptr, bad_min = nullptr;
  else out_off = nullptr, out = nullptr;
  if (newline) {  // (ragged only: the callers' inputs are the parser's)
    if (!write) hipLaunchKernelGGL((k_decode<false, false, true>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
    else hipLaunchKernelGGL((k_decode<false, true, true>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
    return;
  }
  if (!write && !padded) hipLaunchKernelGGL((k_decode<false, false>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
  if (!write && padded) hipLaunchKernelGGL((k_decode<true, false>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
  if (write && !padded) hipLaunchKernelGGL((k_decode<false, true>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
  if (write && padded) hipLaunchKernelGGL((k_decode<true, true>), grid, block, 0, st, in, tb, ig, group, out_len, bad_min, out_off, out);
}

// ---- the encoder's result as a padded matrix -----------------------------------------------------------------------------------------
// longest row of out_off[0 .. n_sent]: one atomicMax per workgroup.  Reads 8 (S + 1) bytes.
__global__ __launch_bounds__(BLOCK) void k_enc_longest(const unsigned long long *__restrict__ out_off, unsigned long long n_sent, unsigned int *longest) {
  __shared__ uint32_t s_m[NWAVES];
  uint32_t m = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; s < n_sent; s += (unsigned long long)gridDim.x * BLOCK) {
    const unsigned long long l = out_off[s + 1] - out_off[s];
    const uint32_t l32 = l > 0xffffffffull ? 0xffffffffu : (uint32_t)l;
    m = l32 > m ? l32 : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = __shfl_down(m, o);
    m = t > m ? t : m;
  }
  if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NWAVES; i++) m = s_m[i] > m ? s_m[i] : m;
    if (m) atomicMax(longest, m);
  }
}

__device__ inline int32_t enc_pad_value(const int32_t *__restrict__ ids, const unsigned long long *__restrict__ out_off, unsigned long long row,
                                        unsigned long long col, int32_t pad_value) {
  const unsigned long long o = out_off[row];
  return col < out_off[row + 1] - o ? ids[o + col] : pad_value;
}
// k_enc_pad: ids + out_off -> row-major int32 [n_sent, width] (tail of a row = pad_value) and int32 lengths[n_sent].  The matrix is walked as one
// flat array in 16-byte units from its first 16-byte boundary: a wavefront stores 1 KB at a time, a part of a long row or several short rows; the
// up to 3 elements in front of the first unit and behind the last one are stored one by one.  Rows must fit (the host checks k_enc_longest first).
// Bytes: read 4 K + 8 (S + 1), written 4 S width + 4 S.
__global__ __launch_bounds__(BLOCK) void k_enc_pad(const int32_t *__restrict__ ids, const unsigned long long *__restrict__ out_off, unsigned long long n_sent,
                                                   unsigned long long width, int32_t pad_value, int32_t *__restrict__ matrix, int32_t *__restrict__ lengths,
                                                   unsigned long long head, unsigned long long n_quads) {
  const unsigned long long t0 = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, nt = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long s = t0; s < n_sent; s += nt) lengths[s] = (int32_t)(out_off[s + 1] - out_off[s]);
  const unsigned long long total = n_sent * width;
  for (unsigned long long q = t0; q < n_quads; q += nt) {
    const unsigned long long e = head + 4 * q;
    unsigned long long row = e / width, col = e - row * width;
    uint32_t v[4];
    for (int i = 0; i < 4; i++) {
      v[i] = (uint32_t)enc_pad_value(ids, out_off, row, col, pad_value);
      if (++col == width) {
        col = 0;
        row++;
      }
    }
    *reinterpret_cast<uint4 *>(matrix + e) = make_uint4(v[0], v[1], v[2], v[3]);
  }
  if (t0 < 8) {  // the elements outside the aligned units
    const unsigned long long tail0 = head + 4 * n_quads;
    const unsigned long long e = t0 < 4 ? t0 : tail0 + (t0 - 4);
    if ((t0 < 4 && e < head) || (t0 >= 4 && e < total)) matrix[e] = enc_pad_value(ids, out_off, e / width, e % width, pad_value);
  }
}

void launch_enc_longest(const unsigned long long *out_off, unsigned long long n_sent, unsigned int *longest, hipStream_t st) {
  if (!n_sent) return;
  hipLaunchKernelGGL(k_enc_longest, grid_for(n_sent, BLOCK), dim3(BLOCK), 0, st, out_off, n_sent, longest);
}
// matrix: 4-byte aligned (the caller checks)
void launch_enc_pad(const int32_t *ids, const unsigned long long *out_off, unsigned long long n_sent, unsigned long long width, int32_t pad_value,
                    int32_t *matrix, int32_t *lengths, hipStream_t st) {
  if (!n_sent) return;
  const unsigned long long total = n_sent * width;
  unsigned long long head = ((16u - ((uintptr_t)matrix & 15u)) & 15u) / 4;
  if (head > total) head = total;
  const unsigned long long n_quads = (total - head) / 4;
  unsigned long long items = n_quads > n_sent ? n_quads : n_sent, b = (items + BLOCK - 1) / BLOCK;
  if (b > 256 * 16) b = 256 * 16;
  hipLaunchKernelGGL(k_enc_pad, dim3((unsigned int)(b ? b : 1)), dim3(BLOCK), 0, st, ids, out_off, n_sent, width, pad_value, matrix, lengths, head, n_quads);
}

}  // namespace yttm
