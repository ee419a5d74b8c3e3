// gpu_ctx_internal.h -- what the translation units of GpuCtx share (round 5: gpu_ctx.cpp, 2 600 lines, was cut along its concerns: gpu_pool.cpp the
// device-memory pool, gpu_upload.cpp corpus -> HBM incl. the overlapped and the chunked front end, gpu_frontend.cpp K1 / K2 / tiles,
// gpu_pairs.cpp pair table + candidate lists, gpu_exchange.cpp the multi-GPU delta exchange, gpu_words.cpp word mode + pair index,
// gpu_ctx.cpp what is left: construction, timers, the merge round).  Code motion only.
// Also here: PoolBuf, the one owner of a block of the device-memory pool, and GpuCtx::Mem, every block a context owns (the structs that
// travel to kernels by value -- PairTable, TileSet, TokLists, PairIndexArgs, DeltaBuf -- are views filled from it and never free); and the
// layouts of the blocks the host addresses and the kernels fill -- the pinned block (PinBlock: mailbox, read-back area, batch staging), the
// device's round block, the counter block of the front end (CounterBlock), list lengths with their tickets (the mailbox itself,
// RoundMailbox, is in yttm_kernels.h).
#pragma once
#include "gpu_ctx.h"

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <future>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>

namespace yttm {

inline unsigned long long pow2_at_least(unsigned long long v) {
  unsigned long long c = 1;
  while (c < v) c <<= 1;
  return c;
}

// ---- gpu_pool.cpp: device memory pool, cached streams / pinned staging of finished contexts
extern thread_local hipStream_t tl_stream;  // the stream / device of the context this thread works for (a freed block may be reused on its own stream at once)
extern thread_local int tl_device;
bool pool_enabled();
void *pool_alloc(size_t bytes);
void pool_free(void *p);
void pool_quiesce(hipStream_t st);
std::mutex &pool_mutex();                 // also guards the event pool of the kernel-family timers (gpu_ctx.cpp)
unsigned long long pool_cached_bytes();   // bytes the pool holds for reuse
unsigned long long pool_peak_bytes();     // high-water mark of the bytes handed out ...
void pool_reset_peak();                   // ... since this call
void pool_arm(unsigned long long fail_at);  // a context is being made: pool_alloc's calls are counted from here, and call number fail_at throws (YTTM_TEST_ALLOC_FAIL; 0: none)
hipStream_t pool_take_stream(int device);           // a stream a finished context left behind (nullptr: none)
bool pool_give_stream(int device, hipStream_t st);  // false: not kept (the caller destroys it)
void *pool_take_pin();                               // the pinned staging buffer of a finished context (nullptr: none)
bool pool_give_pin(void *p);
void release_io_stage();  // gpu_upload.cpp: the upload workers' pinned chunks, streams and events

template <class T>
static T *dmalloc(size_t n) {
  return (T *)pool_alloc((n ? n : 1) * sizeof(T));
}
// One block of the pool and its owner: back in the pool when the owner goes, by return or by a throw (the encoder's DevBuf, enc_lanes.h, is the
// same shape over hipMalloc / hipFree: its buffers bypass the pool on purpose).  A local that a std::thread or a std::future still writes to must
// be declared BEFORE what joins it (destruction is in reverse order).
template <class T>
struct PoolBuf {
  T *p = nullptr;
  PoolBuf() = default;
  explicit PoolBuf(size_t n) { alloc(n); }
  PoolBuf(PoolBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
  PoolBuf &operator=(PoolBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~PoolBuf() { reset(); }
  operator T *() const { return p; }
  T *operator->() const { return p; }
  void reset() {
    if (p) pool_free(p);
    p = nullptr;
  }
  void alloc(size_t n) {  // n elements (at least one), whatever was there before: released first, never two generations at once
    reset();
    p = dmalloc<T>(n);
  }
};


constexpr unsigned int HOT_CAP = 1u << 18;  // hot-list slots (entries appended between rebuilds included)
// a rebuild picks the threshold that lists about HOT_TARGET pairs; fewer live entries than HOT_MIN: lower the threshold.
// YTTM_HOT_TARGET / YTTM_HOT_MIN / YTTM_HOT_CAP override them (the test-suite shrinks them to exercise rebuilds on tiny corpora).
constexpr unsigned int TOP_CAP = 1u << 15;  // top-list slots
constexpr unsigned int RULES_CAP = 1u << 14;  // hash slots for the per-round rule table (batch <= RULES_CAP/2)

// gpu_ctx.cpp: the open-addressing hash (x, y) -> z of a batch's x != y rules in tab[cap]; rules: k entries of `stride` words each, (x, y, z)
// triples or (x, y) pairs (z = 0)
void build_rule_hash(RuleSlot *tab, unsigned int cap, const uint32_t *rules, unsigned int stride, uint32_t k);

// ---- the small blocks that the host addresses and the kernels fill (gpu_ctx.h holds pointers to them)
// The device's round block: where a scan leaves its result before it is in the mailbox -- k_cand_scan's stays here (scan_full copies the block's
// head to the host, ONE copy per round), k_hot_scan's last workgroup forwards it (publish_round) and leaves the counters zeroed.
struct RoundBlock {
  unsigned int n_out[4];  // candidates that passed, keys in the table; k_hot_scan: the list's length, its live entries
  unsigned char pad0_[64 - 16];
  unsigned long long hist[CAND_BINS];
  unsigned char pad1_[8192 - 64 - 8 * CAND_BINS];
  CandRec cand[CAND_CAP];
};
static_assert(offsetof(RoundBlock, hist) == 64 && offsetof(RoundBlock, cand) == 8192, "the round block's layout");
static_assert(offsetof(RoundBlock, cand) == offsetof(RoundMailbox, cand) && sizeof(RoundBlock) == sizeof(RoundMailbox), "scan_full's copy lies over the mailbox, candidates on candidates");
// The front end's counters and the totals of its scans: one 512-byte block, every user a field of its own.  launch_char_hist adds to
// hist_totals[0..1] through the block's address and the chunked front end zeroes the block up to `status` while `status` and `lexicon_cur`
// are live: those keep their place; everything else is addressed field by field.
struct CounterBlock {
  alignas(64) unsigned long long hist_totals[2];    // K1: decode steps, segments
  alignas(64) unsigned int hist_bins;               // char_hist: non-zero bins of the histogram (launch_hist_compact)
  alignas(64) unsigned long long chunk_scan_total;  // K2a: segments of the text, or of the part / chunk at hand
  alignas(64) unsigned int status[8];               // K2b, K2c: the word table's report (k_frontend.hip)
  alignas(64) unsigned int cursor[4];               // K2c: words placed per class, heavy words
  alignas(64) unsigned long long words_scan_total;  // build_class: tokens of the class
  unsigned long long allreduce_scratch;             // allreduce_scalar
  alignas(64) unsigned long long tiles_scan_total;  // maybe_repack: live tokens of the class
  alignas(64) unsigned long long index_scan_total;  // build_index: postings
  unsigned long long lexicon_cur[2];                // chunked front end: the lexicon's end, bytes a relocation will need
};
static_assert(sizeof(CounterBlock) == 64 * 8 && offsetof(CounterBlock, hist_totals) == 0 && offsetof(CounterBlock, status) == 24 * 8 &&
                  offsetof(CounterBlock, lexicon_cur) > offsetof(CounterBlock, status),
              "the counter block's layout");
struct ListCtl {       // a list's length (PairTable::hot_n, top_n, maybe_n) and, beside it, the ticket of finished workgroups of the kernel that
  unsigned int n;      // consumes the list: k_hot_scan and every fused tail (hot list), k_dt_clean (the notes)
  unsigned int ticket;
  unsigned int pad_[2];
};
struct GatherCtl {
  unsigned int matched[WGATHER_MAXK];  // records matched per rule (left at zero)
  unsigned int ticket;                 // k_wgather's finished workgroups
  unsigned int pad_[3];
};
// The pinned block: the mailbox with the candidates' read-back area (scan_full reads its copy of the device's round block there instead), the
// staging of a batch that does not travel in the kernel arguments (k_round_begin and a copy read it over the link), and the one word word
// mode's kernels raise with system-scope stores.  The gaps are what earlier layouts left; every region keeps the offset it has always had.
struct PinBlock {
  union {
    RoundMailbox mailbox;
    RoundBlock round;
  };
  unsigned char pad0_[(1u << 16) - 8192];
  RuleSlot rules[RULES_CAP];                // the batch's rule hash
  unsigned char pad1_[8 * RULES_CAP * sizeof(uint32_t)];
  uint32_t bloom[PM_BLOOM_WORDS_H];         // its pair filter (pm_bloom_host)
  unsigned char pad2_[16384 - PM_BLOOM_WORDS_H * sizeof(uint32_t)];
  uint32_t xyz[3 * (RULES_CAP / 2)];        // word mode: its (x, y, z) triples
  unsigned char pad3_[(1u << 20) - (1u << 16) - 8 * RULES_CAP * sizeof(uint32_t) - 16384 - 3 * (RULES_CAP / 2) * sizeof(uint32_t) - 64];
  unsigned int broken;                      // TokLists::broken: the last line of the block
  unsigned char pad4_[64 - sizeof(unsigned int)];
};
constexpr size_t PIN_BYTES = sizeof(PinBlock);
static_assert(PIN_BYTES == (size_t)CAND_CAP * sizeof(CandRec) + (size_t)RULES_CAP * sizeof(RuleSlot) + (1u << 20), "the pinned block keeps its size");
static_assert(offsetof(PinBlock, rules) == (1u << 16) + (size_t)CAND_CAP * sizeof(CandRec) && offsetof(PinBlock, broken) == PIN_BYTES - 64, "the pinned block keeps its offsets");
static_assert(offsetof(PinBlock, bloom) == offsetof(PinBlock, rules) + sizeof(RuleSlot) * RULES_CAP + 8 * RULES_CAP * sizeof(uint32_t) && offsetof(PinBlock, xyz) == offsetof(PinBlock, bloom) + 16384,
              "the pinned block keeps its offsets");

// ---- every block of device memory a context owns.  Views (pt_, idx_, tl_, db_, WordClass::ts) are filled from these and never free.
struct GpuCtx::PairTableMem {
  PoolBuf<unsigned long long> slots;
  PoolBuf<unsigned int> n_keys;
};
// token tiles: class 0 = short words (slot 1024), class 1 = long words (slot 4096)
struct GpuCtx::WordClass {
  TileSet ts{};
  PoolBuf<uint32_t> d_tok, d_tile_len, d_tile_word0, d_wcnt;
  PoolBuf<uint32_t> d_scratch;  // class C only (k_giant.hip)
  PoolBuf<unsigned int> d_work_n;
  unsigned long long n_unique = 0, n_tokens0 = 0;
  unsigned int n_tiles = 0, nom = 0, slot = 0;
};
// What upload_corpus_fd has done of the front end while the file was still crossing the link (single GPU: K1, K2a and K2b on the parts that
// had arrived; see there): char_hist() / build_word_table() take it from here instead of launching the kernels.
struct GpuCtx::FrontSpec {
  bool hist_done = false;             // d_hist, ctr->hist_totals, d_chunk_segs hold K1's results for the whole text
  bool words_done = false;            // ht holds every segment's word, deduplicated under the code-point-as-id map (valid iff the alphabet keeps every char seen)
  unsigned long long n_segs = 0;
  PoolBuf<unsigned long long> ht;
  unsigned long long ht_cap = 0;
  unsigned int h_status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool long_segments = false;
};
struct GpuCtx::Mem {
  // corpus, K1
  PoolBuf<uint8_t> d_text_owned;
  PoolBuf<unsigned long long> d_hist;  // [N_CODEPOINTS]
  PoolBuf<uint32_t> d_chunk_segs;      // [fe_chunks(n_text_)] segment starts per 4 KB chunk (K1 counts them, K2a places them)
  FrontSpec spec;
  PoolBuf<CounterBlock> ctr;
  // K2
  PoolBuf<uint32_t> d_cpmap;  // [N_CODEPOINTS]
  WordClass cls[3];           // A: words <= TILE_NOM_A tokens, B: <= TILE_NOM_B, C: longer (one workgroup per tile, k_giant.hip)
  // pair table, candidate lists
  PairTableMem pt;
  PoolBuf<uint32_t> d_hot_slots, d_top_slots;
  PoolBuf<ListCtl> d_hot_ctl, d_top_ctl;  // (the hot list's ticket: k_hot_scan's and every fused tail's finished workgroups)
  PoolBuf<RoundBlock> d_round;
  // per-round staging
  PoolBuf<RuleSlot> d_rules;
  PoolBuf<uint32_t> d_bloom;  // pair filter of a batch that does not travel in the kernel arguments
  PoolBuf<unsigned long long> d_stats;
  // pair index of word mode (idx_ is its view)
  struct {
    PoolBuf<unsigned long long> key, off;
    PoolBuf<uint32_t> cnt, bloom, post;
  } idx;
  PoolBuf<unsigned long long> idx_scan_tmp;
  PoolBuf<unsigned char> idx_save;  // the index count pass's per-workgroup tables (k_idx_stream)
  PoolBuf<uint32_t> d_stamp;        // [class-A words] round that claimed the word for its worklist last
  // word mode (tl_ is the view of tl)
  PoolBuf<unsigned long long> d_wmeta;
  PoolBuf<GatherCtl> d_gather;
  PoolBuf<uint32_t> d_xyz;        // a batch too large for BatchArgs, as (x, y, z) triples
  PoolBuf<uint32_t> d_wworklist;  // [n_unique + 64] the round's words
  PoolBuf<DeltaRec> d_drec;       // [WORDS_MAX_GRID * drec_cap_] the round's count updates, a region per workgroup of k_words
  PoolBuf<unsigned int> d_drec_n;
  PoolBuf<uint4> d_irec;          // [WORDS_MAX_GRID * drec_cap_] the round's new-instance records before they go to the tokens' lists
  struct {
    PoolBuf<unsigned long long> base, cursor;
    PoolBuf<uint32_t> cap, fill, rec_word, rec_l, rec_r;
  } tl;
  // multi-GPU delta exchange (db_ is the view of delta)
  struct {
    PoolBuf<DtSlot> keys;
    PoolBuf<uint32_t> touched;
    PoolBuf<DeltaRec> send[2];  // the two send blocks (rounds alternate: yttm_device.h DeltaBuf)
  } delta;
  PoolBuf<DeltaRec> d_recv;
  PoolBuf<unsigned long long> d_xstat;  // [XSTAT_WORDS] the fold's report on a round's exchange (yttm_kernels.h)
  PoolBuf<uint32_t> d_maybe;            // slots whose count an add of this round saw at or above a list threshold (PairTable::maybe)
  PoolBuf<ListCtl> d_maybe_ctl;         // (its ticket: k_dt_clean's)
};

}  // namespace yttm
