// gpu_ctx_internal.h -- what the translation units of GpuCtx share (round 5: gpu_ctx.cpp, 2 600 lines, was cut along its concerns: gpu_pool.cpp the
// device-memory pool, gpu_upload.cpp corpus -> HBM incl. the overlapped and the chunked front end, gpu_frontend.cpp K1 / K2 / tiles,
// gpu_pairs.cpp pair table + candidate lists, gpu_exchange.cpp the multi-GPU delta exchange, gpu_words.cpp word mode + pair index,
// gpu_ctx.cpp what is left: construction, timers, the merge round).  Code motion only.
// Also here: the layouts of the blocks the host addresses and the kernels fill -- the pinned block (PinBlock: mailbox, read-back area, batch
// staging), the device's round block, list lengths with their tickets (the mailbox itself, RoundMailbox, is in yttm_kernels.h).
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
hipStream_t pool_take_stream(int device);           // a stream a finished context left behind (nullptr: none)
bool pool_give_stream(int device, hipStream_t st);  // false: not kept (the caller destroys it)
void *pool_take_pin();                               // the pinned staging buffer of a finished context (nullptr: none)
bool pool_give_pin(void *p);
void release_io_stage();  // gpu_upload.cpp: the upload workers' pinned chunks, streams and events

template <class T>
static T *dmalloc(size_t n) {
  return (T *)pool_alloc((n ? n : 1) * sizeof(T));
}
#define DFREE(p)            \
  do {                      \
    if (p) pool_free((void *)(p)); \
    p = nullptr;            \
  } while (0)

// Pool blocks a function holds in local raw pointers: whatever is still non-null when the scope is left -- by return or by a throw -- goes back
// to the pool (DFREE nulls what it frees; a block handed on to a member is nulled by hand).  Declare it BEFORE anything whose destructor must
// run while the blocks are still alive (destruction is in reverse order).
struct DevScope {
  std::vector<void **> held;
  template <class T> void hold(T *&p) { held.push_back((void **)&p); }
  ~DevScope() {
    for (void **pp : held)
      if (*pp) { pool_free(*pp); *pp = nullptr; }
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

}  // namespace yttm
