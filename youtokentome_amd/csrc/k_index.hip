// k_index.hip -- the pair index (pair -> the words / tiles that hold it; the reference's pair2pos, bpe.cpp:438/:626/:694): seeded from the hot
// list, built by two streaming passes over the token slots (count, fill).  (Until round 4 part of k_merge.hip.)
#include "k_tile_core.h"
#include "k_index_core.h"

namespace yttm {

// every hot-list slot that is still at or above hot_tau becomes a key of the index
__global__ __launch_bounds__(BLOCK) void k_idx_seed(PairTable pt, PairIndex ix) {
  const unsigned int hn_raw = *pt.hot_n;
  const unsigned int hn = hn_raw < pt.hot_cap ? hn_raw : pt.hot_cap;
  for (unsigned int i = blockIdx.x * BLOCK + threadIdx.x; i < hn; i += gridDim.x * BLOCK) {
    const uint32_t sl = pt.hot_slots[i];
    const unsigned long long c = *pt.cnt_p(sl) & PT_CNT;
    if (c < pt.hot_tau || c == 0) continue;
    const unsigned long long key = *pt.key_p(sl);
    const uint32_t h = enc_hash((uint32_t)(key >> 32), (uint32_t)key);
    uint32_t s = h & ix.mask;
    for (;;) {
      const unsigned long long k = atomicCAS(&ix.key[s], PT_EMPTY, key);
      if (k == PT_EMPTY || k == key) break;
      s = (s + 1) & ix.mask;
    }
    atomicOr(&ix.bloom[enc_bloom_word(h)], enc_bloom_bits(h));
  }
}
// One wavefront per tile, tokens in registers: every adjacency whose pair is a key of the index is counted (FILL = false) or has
// its tile / its word appended to the key's postings (FILL = true; one posting per adjacency: duplicates are harmless, the gather
// claims a tile / a word once).  At the word-mode switch nearly every adjacency is a posting (1 GB corpus: 78 M of 94 M tokens, 10 000
// keys): one global atomic per posting was 6 ms per pass.  So a workgroup sums its postings per key in an LDS table first -- count pass:
// one global add per key and workgroup; fill pass: count, reserve the workgroup's run of each key with ONE add, then go over the tiles
// again and hand the run out from LDS cursors.  Keys that find no room in the table take the global atomic per posting as before.
constexpr int IDXA_NT = 512, IDXA_SLOTS = 2048, IDXA_BITS = 11, IDXA_PROBES = 8;
struct IdxAgg {                          // the workgroup's table: pair -> its slot of the index and this workgroup's postings of it.  The
  unsigned long long key[IDXA_SLOTS];    // frequent pairs get in first (PT_EMPTY = free) and are then resolved without leaving the CU:
  uint32_t slot[IDXA_SLOTS];             // no Bloom test, no probe of the index in L2
  uint32_t cnt[IDXA_SLOTS];              // postings of this workgroup; fill pass, second sweep: the cursor
  uint32_t base[IDXA_SLOTS];             // fill pass: start of this workgroup's run of the key's postings
};
// entry of `key` in its probe window, or -1
__device__ inline int idxa_lookup(const IdxAgg &T, unsigned long long key) {
  uint32_t h = pair_hash32(key) >> (32 - IDXA_BITS);
  static_assert(IDXA_SLOTS == 1 << IDXA_BITS, "hash bits");
  for (int p = 0; p < IDXA_PROBES; p++) {
    const unsigned long long k = __hip_atomic_load(&T.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == key) return (int)h;
    if (k == PT_EMPTY) return -1;
    h = (h + 1) & (IDXA_SLOTS - 1);
  }
  return -1;
}
// SWEEP 0: count into the table (count pass: + global adds for what finds no room); SWEEP 1 (fill pass): write the postings
template <int SLOT, bool FILL, bool WORDS, int SWEEP>
__device__ inline void idx_sweep(const TileSet &ts, const PairIndex &ix, const uint32_t *bloom, IdxAgg &T, uint32_t shard) {
  const int lane = lane_id();
  const uint32_t stride = gridDim.x * (IDXA_NT / 64);
  for (uint32_t t = uni(blockIdx.x * (IDXA_NT / 64) + (uint32_t)(threadIdx.x >> 6)); t < ts.n_tiles; t += stride) {  // (uni: a wave's tile is the same in its lanes)
    const int n = (int)ts.tile_len[t];
    uint4 r[SLOT / 256];
    tile_fetch<SLOT>(r, ts, t, n);
    // WORDS: a posting is the WORD that holds the adjacency (word mode: the tile may hold TOK_HOLEs -- word-start bit set, so never the
    // second token of an adjacency; never counted as a word start).
    uint32_t wrow = WORDS ? ts.tile_word0[t] : 0u;
    (void)wrow;
#define IDX_PAIR(T0, T1, WIDX)                                                        \
  if (!((T1)&TOK_WS)) {                                                                \
    const uint32_t a_ = (T0)&TOK_MASK, b_ = (T1)&TOK_MASK;                             \
    const unsigned long long key_ = pair_key(a_, b_);                                  \
    const uint32_t h_ = enc_hash(a_, b_);                                              \
    const uint32_t bits_ = enc_bloom_bits(h_);                                         \
    const bool maybe_ = (bloom[enc_bloom_word(h_)] & bits_) == bits_;  /* (late builds: few adjacencies are keys of the index) */ \
    int e_ = maybe_ ? idxa_lookup(T, key_) : -1;                                       \
    uint32_t s_ = 0xffffffffu;                                                         \
    if (maybe_ && e_ < 0) {  /* not in the table: is it a key of the index at all? */   \
      s_ = idx_find(ix, key_, h_);                                                     \
      if (SWEEP == 0 && s_ != 0xffffffffu) {  /* a place in the table, if its probe window has one */ \
        uint32_t w_ = pair_hash32(key_) >> (32 - IDXA_BITS);                           \
        for (int p_ = 0; p_ < IDXA_PROBES; p_++) {                                     \
          unsigned long long k_ = __hip_atomic_load(&T.key[w_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
          if (k_ == PT_EMPTY) {                                                        \
            k_ = atomicCAS(&T.key[w_], PT_EMPTY, key_);                                \
            if (k_ == PT_EMPTY) k_ = key_;                                             \
          }                                                                            \
          if (k_ == key_) {                                                            \
            T.slot[w_] = s_;                                                           \
            e_ = (int)w_;                                                              \
            break;                                                                     \
          }                                                                            \
          w_ = (w_ + 1) & (IDXA_SLOTS - 1);                                            \
        }                                                                              \
      }                                                                                \
    }                                                                                  \
    if (SWEEP == 0) {                                                                  \
      if (e_ >= 0) atomicAdd(&T.cnt[e_], 1u);                                          \
      else if (!FILL && s_ != 0xffffffffu) atomicAdd(&ix.cnt[(size_t)s_ * IDX_SHARDS + shard], 1u); \
    } else if (e_ >= 0 || s_ != 0xffffffffu) {                                         \
      unsigned long long at_;                                                          \
      if (e_ >= 0) {                                                                   \
        at_ = (unsigned long long)T.base[e_] + atomicAdd(&T.cnt[e_], 1u);              \
      } else {                                                                         \
        const size_t cs_ = (size_t)s_ * IDX_SHARDS + shard;                            \
        at_ = ix.off[cs_] + atomicAdd(&ix.cnt[cs_], 1u);                               \
      }                                                                                \
      ix.post[at_] = WORDS ? (WIDX) : t;                                               \
    }                                                                                  \
  }
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) {
      if (256 * j < n) {
        uint32_t nx = from_lane_right(r[j].x);
        uint32_t nx0 = TOK_WS;
        if (j + 1 < SLOT / 256) nx0 = from_lane0(r[j + 1 < SLOT / 256 ? j + 1 : j].x);
        if (lane == 63) nx = nx0;
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;  // word of my token i
        if (WORDS && SWEEP == 1) {
          const bool s0 = tok_is_ws(r[j].x), s1 = tok_is_ws(r[j].y), s2 = tok_is_ws(r[j].z), s3 = tok_is_ws(r[j].w);
          const unsigned long long m0 = __ballot(s0), m1 = __ballot(s1), m2 = __ballot(s2), m3 = __ballot(s3);
          const unsigned long long lt = lanemask_lt();
          const uint32_t wb = wrow + (uint32_t)(__popcll(m0 & lt) + __popcll(m1 & lt) + __popcll(m2 & lt) + __popcll(m3 & lt));
          w0 = wb + (s0 ? 1u : 0u) - 1u;
          w1 = w0 + (s1 ? 1u : 0u);
          w2 = w1 + (s2 ? 1u : 0u);
          w3 = w2 + (s3 ? 1u : 0u);
          wrow += (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
        }
        // (slots behind the live prefix hold zeros: id 0 is a special token, never part of a pair of the index)
        IDX_PAIR(r[j].x, r[j].y, w0)
        IDX_PAIR(r[j].y, r[j].z, w1)
        IDX_PAIR(r[j].z, r[j].w, w2)
        IDX_PAIR(r[j].w, nx, w3)
      }
    }
#undef IDX_PAIR
  }
}
// `save` [gridDim.x]: the count pass leaves every workgroup's table there, and the fill pass of a build with many postings (agg) starts from
// it instead of counting again (same grid, same tiles per workgroup: the table is exactly what that sweep would rebuild -- a third of the
// build's work).
template <int SLOT, bool FILL, bool WORDS>
__global__ __launch_bounds__(IDXA_NT) void k_idx_stream(TileSet ts, PairIndex ix, int agg /* fill pass: 0 = few postings, one sweep with an atomic each */,
                                                        IdxAgg *__restrict__ save) {
  __shared__ IdxAgg T;
  __shared__ uint32_t bloom[ENC_BLOOM_WORDS];
  for (int i = (int)threadIdx.x; i < ENC_BLOOM_WORDS; i += IDXA_NT) bloom[i] = ix.bloom[i];
  const bool reload = FILL && agg && save;
  for (int i = (int)threadIdx.x; i < IDXA_SLOTS; i += IDXA_NT) {
    T.key[i] = reload ? save[blockIdx.x].key[i] : PT_EMPTY;
    T.cnt[i] = reload ? save[blockIdx.x].cnt[i] : 0u;
    if (reload) T.slot[i] = save[blockIdx.x].slot[i];
  }
  __syncthreads();
  const uint32_t shard = blockIdx.x % IDX_SHARDS;
  if (!FILL || (agg && !reload)) idx_sweep<SLOT, FILL, WORDS, 0>(ts, ix, bloom, T, shard);
  __syncthreads();
  for (int i = (int)threadIdx.x; i < IDXA_SLOTS; i += IDXA_NT) {
    const uint32_t c = T.cnt[i];
    if (!FILL && save) {
      save[blockIdx.x].key[i] = T.key[i];
      save[blockIdx.x].slot[i] = T.slot[i];
      save[blockIdx.x].cnt[i] = c;
    }
    if (T.key[i] == PT_EMPTY || !c) continue;
    const size_t cs = (size_t)T.slot[i] * IDX_SHARDS + shard;
    const uint32_t b0 = atomicAdd(&ix.cnt[cs], c);
    if (FILL) {
      T.base[i] = (uint32_t)ix.off[cs] + b0;  // (the postings number fewer than 2^32: build_index checks)
      T.cnt[i] = 0;
    }
  }
  if (!FILL) return;
  __syncthreads();
  idx_sweep<SLOT, FILL, WORDS, 1>(ts, ix, bloom, T, shard);
}
// ---------------------------------------------------------------------------------------------- the build by radix partition
// The streaming build above pays one LDS atomic on a table slot shared by many lanes, or -- the key found no room in the table: every build
// of tens of thousands of keys -- one global atomic per posting, in both passes, and ends in 4-byte stores all over `post`.  Here a posting
// becomes an 8-byte RECORD {slot of the index, word row} and the records are partitioned like k_pairradix.hip's:
//
//   k_idx_rsweep    tiles -> per adjacency the slot of its pair in the index (Bloom test in LDS, probe of ix.key in L2), left in `slots`
//                   (one word per token slot, bit 31 = the token starts a word, so that the second sweep reads no token and resolves nothing);
//                   records per level-1 group (slot >> s1, <= 256 groups) in an LDS histogram -> wgcnt[group][workgroup], gtot[group], total
//   k_idx_rwgoff    every workgroup's OWN run of every group (goff[group] = where the group starts; goff[nb1] = all records)
//   k_idx_rscatter  `slots` -> rec, grouped by slot >> s1: a record's place comes from a cursor in LDS, no global atomic
//   k_idx_rslots    per group, in chunks of IDXR_NT * PER records (a hot key's records spread over as many workgroups as they fill chunks): counts
//                   per slot in a DENSE LDS array over the group's 2^s1 slots; <false>: one global add per distinct slot and chunk -> ix.cnt
//                   (shard 0 takes all of a key's postings); the exclusive scan gives ix.off; <true>: one RETURNING add per distinct slot and
//                   chunk reserves the chunk's piece of the slot's run, the word rows go there from LDS cursors
//
// Bytes moved (T token slots swept, P postings): 4T read + 4T written, 4T read + 8P written, 8P read, 8P read + 4P written.
constexpr int IDXR_NT = 256;                                   // k_idx_rwgoff, k_idx_rslots
constexpr int IDXR_SW_NT = 512, IDXR_WAVES = IDXR_SW_NT / 64;  // the two sweeps: 33 KB of LDS, four workgroups per CU -- eight waves per SIMD
constexpr uint32_t IDXR_NONE = 0x3fffffffu;     // "this adjacency is no key of the index" in `slots` (the index has at most 2^20 slots)
constexpr int IDXR_PER = 32, IDXR_PER_SMALL = 1;  // records per thread and work item of k_idx_rslots (in registers): 8192 a chunk, and 256 for
constexpr unsigned long long IDXR_SMALL = 1u << 16;  // builds of fewer postings than this -- else a few dozen workgroups would do all the work
constexpr uint32_t IDXR_MAX_SPAN = 4096;        // slots of a level-1 group at most (the dense LDS arrays)
constexpr unsigned int IDXR_GRID_MAX = 1024;    // workgroups of the two sweeps at most (wgcnt / wgoff hold 256 groups x this many)
// scratch (uint32): total (2 words, a uint64) | gtot[256] | goff[257] (+1 pad) | wgcnt[256][IDXR_GRID_MAX] | wgoff[256][IDXR_GRID_MAX]
constexpr size_t IDXR_GTOT = 2, IDXR_GOFF = 258, IDXR_WGCNT = 516, IDXR_WGOFF = IDXR_WGCNT + (size_t)256 * IDXR_GRID_MAX;
__host__ __device__ inline uint32_t idxr_shift1(uint32_t mask) {  // level 1: at most 256 groups of 2^s1 consecutive slots
  uint32_t s = 0;
  while ((mask >> s) + 1u > 256u) s++;
  return s;
}
__device__ inline uint32_t idxr_resolve(const PairIndex &ix, const uint32_t *bloom, uint32_t t0, uint32_t t1) {
  if (t1 & TOK_WS) return IDXR_NONE;
  const uint32_t a = t0 & TOK_MASK, b = t1 & TOK_MASK;
  const uint32_t h = enc_hash(a, b);
  const uint32_t bits = enc_bloom_bits(h);
  if ((bloom[enc_bloom_word(h)] & bits) != bits) return IDXR_NONE;
  const uint32_t s = idx_find(ix, pair_key(a, b), h);
  return s == 0xffffffffu ? IDXR_NONE : s;
}
template <int SLOT>
__global__ __launch_bounds__(IDXR_SW_NT) void k_idx_rsweep(TileSet ts, PairIndex ix, uint32_t s1, uint32_t nb1, uint32_t *__restrict__ slots /* [n_tiles * SLOT] */,
                                                        uint32_t *__restrict__ scratch) {
  __shared__ uint32_t bloom[ENC_BLOOM_WORDS];
  __shared__ uint32_t h[256];
  __shared__ unsigned long long wg_total;
  for (int i = (int)threadIdx.x; i < ENC_BLOOM_WORDS; i += IDXR_SW_NT) bloom[i] = ix.bloom[i];
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  if (threadIdx.x == 0) wg_total = 0;
  __syncthreads();
  const int lane = lane_id();
  const uint32_t stride = gridDim.x * IDXR_WAVES;
  // (a tile's tokens are fetched one tile ahead of their use, its length two tiles ahead)
  uint32_t t = uni(blockIdx.x * IDXR_WAVES + (uint32_t)(threadIdx.x >> 6));
  int n = t < ts.n_tiles ? (int)ts.tile_len[t] : 0, n1 = t + stride < ts.n_tiles ? (int)ts.tile_len[t + stride] : 0;
  uint4 r[SLOT / 256];
  if (t < ts.n_tiles) tile_fetch<SLOT>(r, ts, t, n);
  for (; t < ts.n_tiles; t += stride) {
    uint4 rn[SLOT / 256];
    if (t + stride < ts.n_tiles) tile_fetch<SLOT>(rn, ts, t + stride, n1);
    const int n2 = t + 2 * stride < ts.n_tiles ? (int)ts.tile_len[t + 2 * stride] : 0;
    uint4 *dst = reinterpret_cast<uint4 *>(slots + (size_t)t * SLOT);
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) {
      if (256 * j < n) {
        uint32_t nx = from_lane_right(r[j].x);
        uint32_t nx0 = TOK_WS;
        if (j + 1 < SLOT / 256) nx0 = from_lane0(r[j + 1 < SLOT / 256 ? j + 1 : j].x);
        if (lane == 63) nx = nx0;
        const int i = lane + 64 * j;
        if (4 * i < n) {  // (slots behind the live prefix hold zeros: id 0 is a special token, never part of a pair of the index)
          uint4 o;
          o.x = idxr_resolve(ix, bloom, r[j].x, r[j].y);
          o.y = idxr_resolve(ix, bloom, r[j].y, r[j].z);
          o.z = idxr_resolve(ix, bloom, r[j].z, r[j].w);
          o.w = idxr_resolve(ix, bloom, r[j].w, nx);
          if (o.x != IDXR_NONE) atomicAdd(&h[o.x >> s1], 1u);
          if (o.y != IDXR_NONE) atomicAdd(&h[o.y >> s1], 1u);
          if (o.z != IDXR_NONE) atomicAdd(&h[o.z >> s1], 1u);
          if (o.w != IDXR_NONE) atomicAdd(&h[o.w >> s1], 1u);
          o.x |= tok_is_ws(r[j].x) ? TOK_WS : 0u;
          o.y |= tok_is_ws(r[j].y) ? TOK_WS : 0u;
          o.z |= tok_is_ws(r[j].z) ? TOK_WS : 0u;
          o.w |= tok_is_ws(r[j].w) ? TOK_WS : 0u;
          dst[i] = o;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) r[j] = rn[j];
    n = n1;
    n1 = n2;
  }
  __syncthreads();
  if (threadIdx.x < nb1) {
    const uint32_t c = h[threadIdx.x];
    scratch[IDXR_WGCNT + (size_t)threadIdx.x * gridDim.x + blockIdx.x] = c;
    if (c) {
      atomicAdd(&scratch[IDXR_GTOT + threadIdx.x], c);
      atomicAdd(&wg_total, (unsigned long long)c);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_total) atomicAdd(reinterpret_cast<unsigned long long *>(scratch), wg_total);
}
// workgroup g of this launch: level-1 group g -- where it starts, and where each workgroup of the sweeps puts its records of it
__global__ __launch_bounds__(IDXR_NT) void k_idx_rwgoff(uint32_t *__restrict__ scratch, uint32_t n_wg, uint32_t nb1) {
  __shared__ uint32_t part[IDXR_NT];
  const uint32_t *gtot = scratch + IDXR_GTOT;
  const uint32_t *c = scratch + IDXR_WGCNT + (size_t)blockIdx.x * n_wg;
  uint32_t *o = scratch + IDXR_WGOFF + (size_t)blockIdx.x * n_wg;
  const uint32_t per = (n_wg + IDXR_NT - 1) / IDXR_NT, lo = threadIdx.x * per, hi = lo + per < n_wg ? lo + per : n_wg;
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += c[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t g = 0; g < blockIdx.x; g++) before += gtot[g];
  if (threadIdx.x == 0) {
    scratch[IDXR_GOFF + blockIdx.x] = before;
    if (blockIdx.x + 1 == nb1) scratch[IDXR_GOFF + nb1] = before + gtot[blockIdx.x];
  }
  for (uint32_t j = 0; j < threadIdx.x; j++) before += part[j];
  for (uint32_t i = lo; i < hi; i++) {
    o[i] = before;
    before += c[i];
  }
}
template <int SLOT>
__global__ __launch_bounds__(IDXR_SW_NT) void k_idx_rscatter(TileSet ts, uint32_t s1, uint32_t nb1, const uint32_t *__restrict__ slots, const uint32_t *__restrict__ scratch,
                                                          unsigned long long *__restrict__ rec) {
  __shared__ uint32_t cur[256];  // next place of this workgroup's records of each group (its runs were laid out by k_idx_rwgoff)
  if (threadIdx.x < nb1) cur[threadIdx.x] = scratch[IDXR_WGOFF + (size_t)threadIdx.x * gridDim.x + blockIdx.x];
  __syncthreads();
  const uint32_t stride = gridDim.x * IDXR_WAVES;
  // (the same tiles as this workgroup of k_idx_rsweep took: same grid, same loop)
  const uint4 none = make_uint4(IDXR_NONE, IDXR_NONE, IDXR_NONE, IDXR_NONE);
  auto fetch = [&](uint4(&v)[SLOT / 256], uint32_t tile, int len) {
    const uint4 *src = reinterpret_cast<const uint4 *>(slots + (size_t)tile * SLOT);
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) {
      const int i = lane_id() + 64 * j;
      v[j] = (4 * i < len) ? src[i] : none;
    }
  };
  uint32_t t = uni(blockIdx.x * IDXR_WAVES + (uint32_t)(threadIdx.x >> 6));
  int n = t < ts.n_tiles ? (int)ts.tile_len[t] : 0, n1 = t + stride < ts.n_tiles ? (int)ts.tile_len[t + stride] : 0;
  uint32_t wrow = t < ts.n_tiles ? ts.tile_word0[t] : 0u;
  uint4 q[SLOT / 256];
  if (t < ts.n_tiles) fetch(q, t, n);
  for (; t < ts.n_tiles; t += stride) {
    uint4 qn[SLOT / 256];
    if (t + stride < ts.n_tiles) fetch(qn, t + stride, n1);
    const uint32_t wrow1 = t + stride < ts.n_tiles ? ts.tile_word0[t + stride] : 0u;
    const int n2 = t + 2 * stride < ts.n_tiles ? (int)ts.tile_len[t + 2 * stride] : 0;
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) {
      if (256 * j < n) {
        const uint4 v = q[j];
        // word of my token: k_idx_stream's arithmetic on the ballots of the word-start bits
        const bool b0 = (v.x & TOK_WS) != 0, b1 = (v.y & TOK_WS) != 0, b2 = (v.z & TOK_WS) != 0, b3 = (v.w & TOK_WS) != 0;
        const unsigned long long m0 = __ballot(b0), m1 = __ballot(b1), m2 = __ballot(b2), m3 = __ballot(b3);
        const unsigned long long lt = lanemask_lt();
        const uint32_t wb = wrow + (uint32_t)(__popcll(m0 & lt) + __popcll(m1 & lt) + __popcll(m2 & lt) + __popcll(m3 & lt));
        const uint32_t w0 = wb + (b0 ? 1u : 0u) - 1u, w1 = w0 + (b1 ? 1u : 0u), w2 = w1 + (b2 ? 1u : 0u), w3 = w2 + (b3 ? 1u : 0u);
        wrow += (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
        const uint32_t s0 = v.x & TOK_MASK, s1_ = v.y & TOK_MASK, s2 = v.z & TOK_MASK, s3 = v.w & TOK_MASK;
        if (s0 != IDXR_NONE) rec[atomicAdd(&cur[s0 >> s1], 1u)] = ((unsigned long long)s0 << 32) | w0;
        if (s1_ != IDXR_NONE) rec[atomicAdd(&cur[s1_ >> s1], 1u)] = ((unsigned long long)s1_ << 32) | w1;
        if (s2 != IDXR_NONE) rec[atomicAdd(&cur[s2 >> s1], 1u)] = ((unsigned long long)s2 << 32) | w2;
        if (s3 != IDXR_NONE) rec[atomicAdd(&cur[s3 >> s1], 1u)] = ((unsigned long long)s3 << 32) | w3;
      }
    }
#pragma unroll
    for (int j = 0; j < SLOT / 256; j++) q[j] = qn[j];
    n = n1;
    n1 = n2;
    wrow = wrow1;
  }
}
// rec (grouped by slot >> s1) -> FILL = false: ix.cnt; FILL = true: ix.post.  A work item is a chunk of ONE group's records.
template <bool FILL, int PER>
__global__ __launch_bounds__(IDXR_NT) void k_idx_rslots(const unsigned long long *__restrict__ rec, const uint32_t *__restrict__ scratch, uint32_t s1, uint32_t nb1,
                                                        PairIndex ix) {
  constexpr uint32_t IDXR_CHUNK = (uint32_t)PER * IDXR_NT;
  __shared__ uint32_t dense[IDXR_MAX_SPAN], place[FILL ? IDXR_MAX_SPAN : 1];
  __shared__ uint32_t item0[257];  // work items before each group
  const uint32_t *goff = scratch + IDXR_GOFF;
  const uint32_t span = 1u << s1;
  for (uint32_t i = threadIdx.x; i < span; i += IDXR_NT) dense[i] = 0;
  if (threadIdx.x == 0) {
    uint32_t it = 0;
    for (uint32_t g = 0; g < nb1; g++) {
      item0[g] = it;
      it += (goff[g + 1] - goff[g] + IDXR_CHUNK - 1) / IDXR_CHUNK;
    }
    item0[nb1] = it;
  }
  __syncthreads();
  const uint32_t n_items = item0[nb1];
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    uint32_t g = 0;  // the last group with item0[g] <= it (groups without records share their successor's value: the last of them wins)
    for (uint32_t step = 128; step; step >>= 1)
      if (g + step < nb1 && item0[g + step] <= it) g += step;
    const uint32_t lo = goff[g] + (it - item0[g]) * IDXR_CHUNK, end = goff[g + 1], hi = lo + IDXR_CHUNK < end ? lo + IDXR_CHUNK : end;
    const uint32_t slot0 = g << s1;
    unsigned long long r[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
      const uint32_t i = lo + (uint32_t)j * IDXR_NT + threadIdx.x;
      r[j] = i < hi ? rec[i] : ~0ull;
      if (r[j] != ~0ull) atomicAdd(&dense[(uint32_t)(r[j] >> 32) - slot0], 1u);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < span; s += IDXR_NT) {
      const uint32_t c = dense[s];
      if (!c) continue;
      dense[s] = 0;
      const size_t cs = (size_t)(slot0 + s) * IDX_SHARDS;
      const uint32_t b0 = atomicAdd(&ix.cnt[cs], c);
      if (FILL) place[s] = (uint32_t)ix.off[cs] + b0;  // (the postings number fewer than 2^32: build_index checks)
    }
    __syncthreads();
    if (FILL) {
#pragma unroll
      for (int j = 0; j < PER; j++)
        if (r[j] != ~0ull) ix.post[atomicAdd(&place[(uint32_t)(r[j] >> 32) - slot0], 1u)] = (uint32_t)r[j];
      __syncthreads();  // (place is rewritten by the next item)
    }
  }
}

void launch_idx_seed(const PairTable &pt, const PairIndexArgs &a, unsigned int listed_hint, hipStream_t st) {
  const PairIndex ix{a.key, a.cnt, a.off, a.bloom, a.post, a.mask};
  unsigned int g = (listed_hint + BLOCK - 1) / BLOCK;
  if (g < 1) g = 1;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(k_idx_seed, dim3(g), dim3(BLOCK), 0, st, pt, ix);
}
size_t idx_save_bytes() { return (size_t)512 * sizeof(IdxAgg); }
void launch_idx_stream(bool fill, const TileSet &ts, const PairIndexArgs &a, hipStream_t st, bool agg, void *save_) {
  IdxAgg *save = reinterpret_cast<IdxAgg *>(save_);
  if (!ts.n_tiles) return;
  const PairIndex ix{a.key, a.cnt, a.off, a.bloom, a.post, a.mask};
  unsigned int g = (ts.n_tiles + IDXA_NT / 64 - 1) / (IDXA_NT / 64);
  if (g > 512) g = 512;  // (two workgroups per CU: 72 KB of LDS each; count and fill pass MUST use the same grid -- a workgroup's shard and tiles)
  if (fill) hipLaunchKernelGGL((k_idx_stream<TILE_SLOT_A, true, true>), dim3(g), dim3(IDXA_NT), 0, st, ts, ix, agg ? 1 : 0, save);
  else hipLaunchKernelGGL((k_idx_stream<TILE_SLOT_A, false, true>), dim3(g), dim3(IDXA_NT), 0, st, ts, ix, agg ? 1 : 0, save);
}
// ---- the radix build's launchers.  sweep -> (host: total) -> scatter -> (host: exclusive scan of ix.cnt, cursors cleared) -> place
size_t idx_radix_scratch_u32() { return IDXR_WGOFF + (size_t)256 * IDXR_GRID_MAX; }
size_t idx_radix_scratch_head_bytes() { return IDXR_GOFF * 4; }  // what must arrive zeroed: the total and the groups' totals
static unsigned int idxr_grid(unsigned int n_tiles) { return tile_grid(n_tiles, IDXR_WAVES, 4); }
bool idx_radix_takes(unsigned int mask, unsigned int n_tiles) {
  return n_tiles && mask < (1u << 20) && (1u << idxr_shift1(mask)) <= IDXR_MAX_SPAN && idxr_grid(n_tiles) <= IDXR_GRID_MAX;
}
void launch_idx_radix_sweep(const TileSet &ts, const PairIndexArgs &a, uint32_t *scratch, uint32_t *slots, hipStream_t st) {
  const PairIndex ix{a.key, a.cnt, a.off, a.bloom, a.post, a.mask};
  const uint32_t s1 = idxr_shift1(a.mask), nb1 = (a.mask >> s1) + 1u;
  const unsigned int g = idxr_grid(ts.n_tiles);
  hipLaunchKernelGGL((k_idx_rsweep<TILE_SLOT_A>), dim3(g), dim3(IDXR_SW_NT), 0, st, ts, ix, s1, nb1, slots, scratch);
  hipLaunchKernelGGL(k_idx_rwgoff, dim3(nb1), dim3(IDXR_NT), 0, st, scratch, g, nb1);
}
static unsigned int idxr_items_grid(unsigned long long total, uint32_t nb1) {  // (a group's last chunk may be short: at most nb1 items more)
  return (unsigned int)std::min<unsigned long long>(2048, total / ((total < IDXR_SMALL ? IDXR_PER_SMALL : IDXR_PER) * IDXR_NT) + nb1);
}
template <bool FILL>
static void idxr_launch_slots(const unsigned long long *rec, const uint32_t *scratch, const PairIndex &ix, unsigned long long total, hipStream_t st) {
  const uint32_t s1 = idxr_shift1(ix.mask), nb1 = (ix.mask >> s1) + 1u;
  const unsigned int g = idxr_items_grid(total, nb1);
  if (total < IDXR_SMALL) hipLaunchKernelGGL((k_idx_rslots<FILL, IDXR_PER_SMALL>), dim3(g), dim3(IDXR_NT), 0, st, rec, scratch, s1, nb1, ix);
  else hipLaunchKernelGGL((k_idx_rslots<FILL, IDXR_PER>), dim3(g), dim3(IDXR_NT), 0, st, rec, scratch, s1, nb1, ix);
}
void launch_idx_radix_scatter(const TileSet &ts, const PairIndexArgs &a, const uint32_t *scratch, const uint32_t *slots, unsigned long long *rec,
                              unsigned long long total, hipStream_t st) {
  const PairIndex ix{a.key, a.cnt, a.off, a.bloom, a.post, a.mask};
  const uint32_t s1 = idxr_shift1(a.mask), nb1 = (a.mask >> s1) + 1u;
  hipLaunchKernelGGL((k_idx_rscatter<TILE_SLOT_A>), dim3(idxr_grid(ts.n_tiles)), dim3(IDXR_SW_NT), 0, st, ts, s1, nb1, slots, scratch, rec);
  idxr_launch_slots<false>(rec, scratch, ix, total, st);
}
void launch_idx_radix_place(const PairIndexArgs &a, const uint32_t *scratch, const unsigned long long *rec, unsigned long long total, hipStream_t st) {
  const PairIndex ix{a.key, a.cnt, a.off, a.bloom, a.post, a.mask};
  idxr_launch_slots<true>(rec, scratch, ix, total, st);
}
}  // namespace yttm
