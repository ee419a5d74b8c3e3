// yttm_kernels.h -- host-callable launchers of the gfx950 kernels (k_frontend.hip; k_tiles.hip, k_words.hip, k_index.hip, k_pairtable.hip, k_giant.hip; k_encode.hip, k_wcache.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "yttm_config.h"
#include "yttm_device.h"

namespace yttm {

constexpr int CAND_BINS = 704;  // counts 0..255 exact, then 8 bins per power of two

struct CandRec {
  unsigned long long key;  // x<<32|y
  unsigned long long cnt;
};
constexpr unsigned int CAND_CAP = 1u << 20;  // candidates a scan can hand over (the read-back area behind the mailbox holds as many)
constexpr unsigned int CAND_FAST = 4096;     // of those, the first ones travel through the mailbox itself; the rest by a copy of their own

// The round's mailbox: what a candidate scan (scan_top in the tail of the round's last kernel, k_hot_scan's publish_round) writes into the
// host's pinned block, and what the host reads when it has seen `round_id` (GpuCtx::poll_mailbox).  The device writes everything else first,
// then __threadfence_system(), a barrier, and ONE system-scope release store of round_id; the host spins on that word (volatile) and issues
// an acquire fence before it reads the rest (k_merge_shared.h, "ORDERING OF A FUSED TAIL").
// `listed`: the length of the list the scan read, before it read it -- the TOP list after scan_top (k_top_scan, a fused tail, k_fold_list),
// the HOT list after k_hot_scan; `live`: those of its entries still at or above the list's threshold.  `hot_listed` and `top_bin` are
// written by scan_top only.
struct RoundMailbox {
  uint32_t n_cand;                     // candidates that passed (may exceed what was stored: CAND_CAP, and CAND_FAST of them here)
  uint32_t n_keys;                     // keys in the pair table (scan_top: one round old, it folds the statistics after publishing)
  uint32_t listed, live;
  uint32_t hot_listed;                 // scan_top: hot-list entries (overflow check)
  uint32_t top_bin;                    // scan_top: no histogram bin above this one is in use (every line of the pinned block the host touches is a cache miss)
  unsigned long long round_ticks;      // scan_top: the round's duration on the device (ScanArgs::timed; 100 MHz ticks)
  uint32_t round_id, pad0_;            // published last
  unsigned long long tokens_cum;       // tokens the K4 kernels streamed so far (repack trigger)
  unsigned long long touched_cum;      // tiles (word mode: words) that held a merge site so far
  unsigned long long xverdict[4];      // multi-GPU, the fold's report on the round's exchange (XSTAT_WORDS: d_xstat[0..3]); zeros on a single GPU
  unsigned long long sites_cum;        // scan_top: merge sites so far (word-mode switch)
  unsigned long long tail_marks[4];    // scan_top's timing marks (100 MHz wall clock)
  unsigned long long hist[CAND_BINS];  // histogram of the live counts
  unsigned char pad1_[6144 - 128 - 8 * CAND_BINS];
  unsigned long long xsum[5];          // multi-GPU, sums over the ranks' block headers (d_xstat[4..7]): [0] merge sites so far, [1] tokens streamed so far,
                                       // [2] class-A tiles, [3] ranks; [4] the round's apply kernels on the device clock (ticks; ScanArgs::timed)
  unsigned char pad2_[8192 - 6144 - 8 * 5];
  CandRec cand[CAND_CAP];              // the first CAND_FAST by the device; the host copies the rest behind them when it wants more
};
#define YTTM_MB_AT(field, at) static_assert(offsetof(RoundMailbox, field) == at, "RoundMailbox::" #field " moved")
YTTM_MB_AT(n_cand, 0); YTTM_MB_AT(n_keys, 4); YTTM_MB_AT(listed, 8); YTTM_MB_AT(live, 12); YTTM_MB_AT(hot_listed, 16); YTTM_MB_AT(top_bin, 20);
YTTM_MB_AT(round_ticks, 24); YTTM_MB_AT(round_id, 32); YTTM_MB_AT(tokens_cum, 40); YTTM_MB_AT(touched_cum, 48); YTTM_MB_AT(xverdict, 56);
YTTM_MB_AT(sites_cum, 88); YTTM_MB_AT(tail_marks, 96); YTTM_MB_AT(hist, 128); YTTM_MB_AT(xsum, 6144); YTTM_MB_AT(cand, 8192);
#undef YTTM_MB_AT

// The statistics block of the merge loop (d_stats, unsigned long long words): totals, then one row per workgroup.
enum StatWord : int {
  STAT_SITES = 0,          // merge sites
  STAT_TOUCHED = 1,        // tiles (word mode: words) that held one
  STAT_TOKENS = 2,         // tokens the K4 kernels streamed
  STAT_TOUCHED_TOKENS = 3, // tokens of the tiles that held a site
  STAT_INSTR_WORDS = 4,    // measurement pass (BatchArgs::instr): words that held a site ...
  STAT_INSTR_TOKENS = 5,   // ... and their tokens
  STAT_T0 = 6,             // wall_clock64() at the start of the round's first launch
  STAT_T1 = 7,             // (multi-GPU) ... when the round's apply kernels and the all-gather behind them were done (noted by the fold's first kernel)
  STAT_PROF = 8,           // [STAT_PROF_N] YTTM_K4_PROF build: per-phase cycles of the apply kernels; the last two: emits that found no room in LDS, their cycles
  STAT_TAIL = 24,          // [STAT_TAIL_N] YTTM_K4_PROF build: scan_top's phases (100 MHz ticks, summed over the rounds); the last one: the scans counted
  BLK_BASE = 32,           // workgroup b's row: the BLK_COLS words from stats[blk_at(b)] on
};
constexpr int STAT_PROF_N = 16, STAT_PROF_MISS_N = STAT_PROF + 14, STAT_PROF_MISS_CYC = STAT_PROF + 15, STAT_TAIL_N = 8, STAT_TAIL_SCANS = STAT_TAIL + 7;
static_assert(STAT_PROF + STAT_PROF_N == STAT_TAIL && STAT_TAIL + STAT_TAIL_N == BLK_BASE, "the totals fill the words below the rows");
constexpr int BLK_ROWS = 1536;  // >= the largest grid of k_tiles<.., true>
// a row's columns: the K4 counters STAT_SITES .. STAT_TOUCHED_TOKENS under their own numbers, then
enum BlkCol : int { BLK_NEW_KEYS = 4 /* pair-table slots claimed */, BLK_PROF_T0 = 5, BLK_PROF_T1 = 6, BLK_PROF_AUX = 7 /* YTTM_K4_PROF build: the workgroup's timeline */, BLK_COLS = 8 };
template <class I>
__host__ __device__ constexpr auto blk_at(I b, int col = 0) { return BLK_BASE + BLK_COLS * b + col; }  // index of a column of workgroup b's row
constexpr int STATS_WORDS = BLK_BASE + BLK_COLS * BLK_ROWS;

// lower bound of a candidate-histogram bin (inverse of cand_bin in k_merge_shared.h)
inline unsigned long long cand_bin_lower(int bin) {
  if (bin < 256) return (unsigned long long)bin;
  int e = 8 + (bin - 256) / 8, m3 = (bin - 256) % 8;
  return (unsigned long long)(8 + m3) << (e - 3);
}

// ---- front end (k_frontend.hip)
// wide_chars: many chars beyond U+07FF (three- and four-byte UTF-8): they are counted in an LDS hash instead of global atomics
// chunk_segs [fe_chunks(n)]: segment starts per 4 KB chunk of the text (out); the segment pass takes their exclusive scan
// [chunk_lo, chunk_hi): the 4 KB chunks of this launch -- all of them, or those of a part of the text that has arrived while the rest is still on
// its way over the link (gpu_ctx.cpp upload_corpus_fd); counts and histogram add up over the launches
void launch_char_hist(const uint8_t *text, unsigned long long n, unsigned long long *hist, unsigned long long *counters, bool wide_chars,
                      uint32_t *chunk_segs, hipStream_t st, unsigned long long chunk_lo = 0, unsigned long long chunk_hi = ~0ull);
unsigned long long fe_chunks(unsigned long long n);
unsigned long long fe_chunk_bytes();
void launch_seg_write(const uint8_t *text, unsigned long long n, unsigned long long *seg_pos, const unsigned long long *chunk_off, hipStream_t st,
                      unsigned long long chunk_lo = 0, unsigned long long chunk_hi = ~0ull);
void launch_hist_compact(const unsigned long long *hist, uint32_t *cps, unsigned long long *cnts, unsigned int *n_out, unsigned int cap,
                         hipStream_t st);
// word table (K2b/K2c): ht[0 .. n_slots) keys, ht[n_slots .. 2 n_slots) counts, ht[2 n_slots .. 3 n_slots) positions of the short words, see k_frontend.hip
void launch_word_table_clear(unsigned long long *ht, unsigned long long n_slots, hipStream_t st);
void launch_insert_words(const uint8_t *text, unsigned long long n, const uint32_t *cpmap, const unsigned long long *seg_pos,
                         unsigned long long n_segs, unsigned long long *ht, unsigned long long ht_mask, unsigned int *status, hipStream_t st,
                         unsigned int max_blocks = 256 * 32 /* (a part of the segments: fewer workgroups, each ends with a flush of its LDS table) */);
// chunked front end (k_frontend.hip: k2b_relocate, k2b_rehash): words whose representative lies below `chunk_end` move to the lexicon at *cursor
// (device; advanced by the bytes taken -- move == false only adds them up); the table rebuilt with new_slots (a power of two, cleared) slots
void launch_words_relocate(uint8_t *text, unsigned long long chunk_end, unsigned long long chunk_len, unsigned long long *ht, unsigned long long n_slots,
                           unsigned long long *cursor, bool move, hipStream_t st);
void launch_word_table_rehash(const uint8_t *text, unsigned long long n, const uint32_t *cpmap, const unsigned long long *old_ht, unsigned long long old_slots,
                              unsigned long long *new_ht, unsigned long long new_slots, hipStream_t st);
void launch_compact_words(const uint8_t *text, unsigned long long n, const uint32_t *cpmap, const unsigned long long *ht, unsigned long long n_slots,
                          unsigned long long *posA, uint32_t *cntA, uint32_t *lenA, unsigned long long *posB, uint32_t *cntB, uint32_t *lenB,
                          unsigned long long *posC, uint32_t *cntC, uint32_t *lenC, unsigned int *cursor, unsigned int *status,
                          unsigned long long wmax /* largest weight a word may carry (2^32 - 1; tests: less) */,
                          unsigned long long *heavy /* [HEAVY_CAP][3] words seen more often than that: pos, tokens, count still to place; their number in cursor[3] */,
                          hipStream_t st);
constexpr int HEAVY_CAP = 256;  // (a word of two bytes seen 2^32 times is 8.6 GB of text: HBM holds a few dozen such words at most -- and tests lower wmax)
void launch_exclusive_scan(const uint32_t *in, unsigned long long n, unsigned long long *out, unsigned long long *block_sums,
                           unsigned long long *total_out, hipStream_t st);
unsigned long long scan_scratch_blocks(unsigned long long n);
void launch_fill_tokens(const uint8_t *text, unsigned long long n, const uint32_t *cpmap, uint32_t space_id,
                        const unsigned long long *uw_pos, const unsigned long long *uw_off, unsigned int n_words, unsigned int nom,
                        unsigned int slot, const unsigned long long *tile_start, uint32_t *tok, hipStream_t st,
                        unsigned long long total_tokens /* of these words: picks the size of the wavefronts' LDS windows */);
void launch_tiles(const unsigned long long *uw_off, unsigned int n_words, unsigned int nom, unsigned long long *tile_start,
                  uint32_t *tile_word0, hipStream_t st);
void launch_tile_len(const unsigned long long *tile_start, unsigned int n_tiles, unsigned long long total_tokens, uint32_t *tile_len,
                     hipStream_t st);

// ---- merge loop (k_tiles.hip, k_pairtable.hip)
// cls: 0 = class A tiles (slot 1024), 1 = class B tiles (slot 4096)
// A small batch travels as a kernel argument: the apply kernel and the candidate scan build their LDS tables (token flags, rule
// hash) from it, and the round needs no prologue kernel, no rule upload and no flag table in HBM.  Used when the whole round
// runs without the filter pass (small or dense tile sets), all ids fit the LDS flag bitmap and there is no class-C tile.
constexpr int BATCH_ARGS_MAX = 128;  // (1 KB of kernel arguments; 32 until round 3: the late rounds of random text have batches of 30 .. 100 rules)
constexpr uint32_t FLAG_LDS_IDS = 32768;  // (8 KB of LDS: the batch's pair filter, or the direct pair -> rule table)
constexpr uint32_t DIRECT_MAX_V = 90;     // direct table: ids below this (90 * 90 bytes <= 8 KB)
struct BatchArgs {
  uint32_t k;                        // 0: not used (tables come from HBM)
  uint32_t xy[2 * BATCH_ARGS_MAX];   // rule j of the batch merges (xy[2j], xy[2j+1]) into z_base + j; x == y: the self rule (skipped)
  uint32_t direct_v;                 // != 0 (class-A k_tiles<.., DIRECT>): every token id in the tiles is < direct_v, and direct_v^2 bytes fit the LDS table
                                     // that maps a PAIR straight to its rule -- the first rounds of a small alphabet, the most expensive ones: one byte
                                     // read per adjacency instead of a pair filter and a hash probe
  uint32_t mark;                     // this is the round's first launch: workgroup 0 notes the time in stats[STAT_T0] (the round's duration then
                                     // comes from the device's own clock, ScanArgs::timed -- two hipEventRecord calls per round cost 4 us of host time)
  uint32_t instr;                    // measurement pass (never timed): also count the WORDS that hold a merge site and their tokens
                                     // (T_touched, W_touched) into stats[STAT_INSTR_WORDS], stats[STAT_INSTR_TOKENS]; single-site tiles take the general path
};
// The candidate scan that follows a merge round, done by the round's own apply kernel: the last workgroup to finish folds the
// statistics rows, zeroes the batch's pairs, scans (and compacts) the hot list and publishes header + histogram + candidates
// in the host's pinned mailbox -- one launch per round instead of two, and no second trip through the launch path.
struct ScanArgs {
  uint32_t on;  // 0: no tail in this launch; 1: the candidate scan; 2 (multi-GPU, word mode): the last workgroup only leaves the worklist
                // counters at zero -- the scan rides in the fold kernel behind the all-gather (k_fold_list); 3 (multi-GPU, set by
                // launch_words_apply): a one-launch word round, which leaves no worklist behind -- no ticket, no tail
  uint32_t tau_mx;
  unsigned long long tau_cnt;  // candidates: count > tau_cnt, or == tau_cnt and max(x,y) <= tau_mx
  CandRec *out;                // [cap] all candidates (the first `fast` also go to the mailbox)
  unsigned int cap, fast;
  unsigned int *done_ctr;      // ticket of finished workgroups (left at 0); nullptr: a single-workgroup launch
  RoundMailbox *mailbox;       // the host's pinned mailbox, or (round_id == 0) a staging block in HBM with the same layout
  uint32_t round_id;           // published in the mailbox when everything else is there; 0: nothing is published
  uint32_t want;               // != 0: about this many candidates are wanted -- the scan may raise the threshold by itself (scan_top: refine)
  uint32_t timed;              // the round's first launch left its start time in stats[STAT_T0]: the mailbox gets the duration (100 MHz ticks)
};
// The batch whose pairs are still to be zeroed by the next scan of a candidate list (every occurrence was merged, so their counts are exactly
// zero): its rule hash in HBM (rules, mask; self_key: its x == x rule, or PT_EMPTY), or -- a batch that travelled as a kernel argument -- ba.
// Neither: nothing is pending.
struct ZeroBatch {
  const RuleSlot *rules;
  unsigned int mask;
  unsigned long long self_key;
  const BatchArgs *ba;
};
void launch_top_scan(const PairTable &pt, const ScanArgs &sa, unsigned long long *stats, const ZeroBatch &zero,
                     unsigned long long *xstat /* multi-GPU: the exchange's report, forwarded to the mailbox */, hipStream_t st);
void launch_top_rebuild(const PairTable &pt, unsigned int listed_hint, hipStream_t st);
// id_min / n_ids: the token ids in the tiles are id_min .. id_min + n_ids - 1 (K3 runs before any merge: the alphabet); n_ids <= 32
// counts pairs in a dense LDS table, 0 (unknown / larger) in the LDS hash
void launch_pair_count(int cls, const TileSet &ts, const PairTable &pt, const DeltaBuf &db, uint32_t id_min, uint32_t n_ids, hipStream_t st);
// K3 of class A for alphabets of 65 .. K3R_MAX_IDS symbols by two-level radix partition of (pair, weight) records (k_pairradix.hip): no atomic per
// adjacency.  scratch: pair_count_radix_scratch_u32(n_ids) words; buf1, buf2: one 8-byte record per class-A token each.  false: nothing was
// launched (a grid larger than the scratch provides for): the caller counts with the general kernel.
constexpr uint32_t K3R_MAX_IDS = 8192;
size_t pair_count_radix_scratch_u32(uint32_t n_ids);
bool pair_count_radix_takes(uint32_t n_ids, unsigned long long n_tokens);
bool launch_pair_count_radix(const TileSet &ts, const PairTable &pt, const DeltaBuf &db, uint32_t id_min, uint32_t n_ids, uint32_t *scratch,
                             unsigned long long *buf1, unsigned long long *buf2, unsigned long long n_tokens, hipStream_t st);
void launch_merge_apply(int cls, const TileSet &ts, const PairTable &pt, const DeltaBuf &db, const RuleSlot *rules, unsigned int rule_mask,
                        uint32_t self_x, uint32_t self_z, uint32_t z_base, unsigned long long *stats, const BatchArgs *ba,
                        const ScanArgs *scan /* the round's last launch only */,
                        const uint32_t *bloom_g /* the batch not in ba: the batch's pair filter (pm_bloom_host) */,
                        unsigned int apply_grid /* YTTM_APPLY_GRID: class-A grid cap for small tile sets (0: none) */, hipStream_t st);
constexpr int PM_BLOOM_WORDS_H = 2048;
void pm_bloom_host(uint32_t *bloom, const uint32_t *xyz, uint32_t k);
// pair index for K4's worklists (k_index_core.h: PairIndex; k_index.hip)
// A key's posting count / fill cursor is kept in IDX_SHARDS copies (a wave adds to copy (its number) % IDX_SHARDS): a pair with a million
// adjacencies is a million atomics on ONE address otherwise (~12 ns each: 6.5 ms per pass at the word-mode switch of the 1 GB corpus).
// The copies' runs are adjacent, so a key's postings are still one run: [off[s * IDX_SHARDS], off[(s + 1) * IDX_SHARDS]).
constexpr unsigned int IDX_SHARDS = 16;
struct PairIndexArgs {
  unsigned long long *key, *off;
  uint32_t *cnt, *bloom, *post;
  unsigned int mask;
};
void launch_idx_seed(const PairTable &pt, const PairIndexArgs &a, unsigned int listed_hint, hipStream_t st);
// (class-A token slots in word mode: postings are word ids, the slots may hold TOK_HOLEs)
void launch_idx_stream(bool fill, const TileSet &ts, const PairIndexArgs &a, hipStream_t st,
                       bool agg = true /* fill pass: sum a workgroup's postings per key in LDS first (worth a second sweep only when they are many) */,
                       void *save = nullptr /* [idx_save_bytes()] the count pass's per-workgroup tables, reused by an agg fill pass */);
size_t idx_save_bytes();
// The same index by radix partition of its postings (k_index.hip): sweep (adjacency -> slot, records per level-1 group; the posting total lands in
// scratch[0..1] as a uint64) -> scatter (records to their groups, counts per slot into a.cnt) -> [exclusive scan of a.cnt, cursors cleared] -> place.
// scratch: idx_radix_scratch_u32() words, the first idx_radix_scratch_head_bytes() zeroed; slots: one word per class-A token slot; rec: one
// 8-byte record per posting.  idx_radix_takes: the index and the tile set are of a size the path is laid out for.
size_t idx_radix_scratch_u32();
size_t idx_radix_scratch_head_bytes();
bool idx_radix_takes(unsigned int mask, unsigned int n_tiles);
void launch_idx_radix_sweep(const TileSet &ts, const PairIndexArgs &a, uint32_t *scratch, uint32_t *slots, hipStream_t st);
void launch_idx_radix_scatter(const TileSet &ts, const PairIndexArgs &a, const uint32_t *scratch, const uint32_t *slots, unsigned long long *rec,
                              unsigned long long total, hipStream_t st);
void launch_idx_radix_place(const PairIndexArgs &a, const uint32_t *scratch, const unsigned long long *rec, unsigned long long total, hipStream_t st);
// ---- word mode (k_words.hip)
void launch_words_init(const TileSet &ts, unsigned long long *wmeta, hipStream_t st);
struct WGatherArgs {  // (a kernel argument of k_wgather and k_words<FUSED>)
  PairIndexArgs ix;
  uint32_t ix_valid, z_static;   // tokens below z_static existed when the index was built
  TokLists tl;
  uint32_t *stamp;               // [n_words] round that claimed the word last
  uint32_t round_id;
  uint32_t *worklist;            // WL_PARTS sub-lists, wl_seg entries apart; work_n[0..WL_PARTS) their lengths, work_n[WL_PARTS + 1] != 0: take every word
  unsigned long long wl_seg;
  unsigned int *work_n;
  unsigned int *gm;              // [WGATHER_MAXK] records matched per rule (left at zero)
  unsigned int *done_ctr;
  unsigned long long *stats;     // (BatchArgs::mark)
  const uint32_t *xyz;           // rule j = (xyz[3j], xyz[3j+1]) -> z_base + j, in HBM; nullptr: the batch is in the BatchArgs
  uint32_t k, z_base;
  uint32_t cnt[BATCH_ARGS_MAX];  // k_words<FUSED>: the count the host picked rule j by (saturated): no rule has more sites than that
};
constexpr unsigned int WGATHER_MAXK = 4096;
void launch_wgather(const WGatherArgs &a, const BatchArgs *ba, unsigned int work_hint, int grid /* YTTM_WGATHER_GRID; < 0: by the hint */, hipStream_t st);
// A word-mode round of class A: the gather (k_wgather), the words (k_words), their records (k_delta_apply) -- or fewer launches, see the fields.
struct WordsRound {
  WordSet ws;
  PairTable pt;
  DeltaBuf db;
  const RuleSlot *rules;          // the batch's rule hash in HBM (the batch not in *ba)
  unsigned int rule_mask;
  const uint32_t *bloom_g;        // ... and its pair filter
  uint32_t self_x, self_z;        // the batch's x == y rule; self_x == 0xffffffff: none
  DeltaRec *drec;                 // [WORDS_MAX_GRID * drec_cap]
  unsigned int drec_cap;
  unsigned int *drec_n;           // [WORDS_MAX_GRID]
  uint4 *irec;                    // [WORDS_MAX_GRID * drec_cap]
  const BatchArgs *ba;
  const ScanArgs *scan;           // the round's tail (nullptr: none)
  unsigned int work_hint;         // about how many words the round will visit (0: unknown / every word)
  unsigned int inline_max;        // rounds of at most this many words (by the hint) apply their records themselves
  const WGatherArgs *ga;          // the round's gather -- its worklist, instance lists, statistics block, k and z_base are k_words' too --: launched
                                  // here (k_wgather) ...
  unsigned int fuse_max;          // ... unless the hint is at most this and the batch is in the arguments: k_words gathers itself
  unsigned int avg_word_tokens;   // live tokens per word, about (0: unknown): a wave takes no more words at a time than fit its 512-token tile
  int wgather_grid, words_grid, words_wpi;  // YTTM_WGATHER_GRID, YTTM_WORDS_GRID, YTTM_WORDS_WPI (tests); < 0: the launcher's own choice
};
bool launch_words_apply(const WordsRound &r, hipStream_t st);  // true: the round was ONE launch (k_words<FUSED>)
constexpr unsigned int WORDS_MAX_GRID = 512;  // workgroups of k_words: each owns a region of the round's count-update records
void launch_repack(int cls, const TileSet &ts, const unsigned long long *off, unsigned int nom, unsigned long long total,
                   unsigned long long *gstart, unsigned int n_new, uint32_t *new_tok, uint32_t *new_len, uint32_t *new_word0, hipStream_t st);
void launch_cand_scan(const PairTable &pt, unsigned long long tau_cnt, uint32_t tau_mx, CandRec *out, unsigned int cap,
                      unsigned int *n_out, unsigned long long *hist, hipStream_t st);
// One scan of the hot list (k_hot_scan): the candidates as sa says (threshold, out, cap; on, want, timed are not looked at), their number,
// the key count, the list's length and its live entries in n_out[0..3], the histogram of the live counts in hist; then the last workgroup
// (sa.done_ctr) publishes all of it in sa.mailbox under sa.round_id.
struct HotScan {
  PairTable pt;
  ScanArgs sa;
  unsigned int *n_out;
  unsigned long long *hist;
  unsigned long long *stats;
  ZeroBatch zero;
  unsigned int listed_hint;    // about the list's length: sizes the grid
  unsigned long long *xstat;   // multi-GPU: the exchange's report, forwarded to the mailbox
};
void launch_hot_scan(const HotScan &h, hipStream_t st);
// ---- multi-GPU, per round: K4 -> ncclAllGather -> k_pt_apply_blocks -> k_fold_list (+ the round's candidate scan) [-> k_dt_clean, during the host's turn]
void launch_dt_clean(const DeltaBuf &db /* .send = the block just exchanged */, DeltaRec *other /* the block of the round to come */, unsigned int n_hint,
                     unsigned long long *stats, uint32_t tiles_a, unsigned int *done_ctr, hipStream_t st);
void launch_dt_init(DtSlot *slots, unsigned long long n, hipStream_t st);
// phase 1: the OTHER ranks' count deltas into the local replica (no list appends: pass a PairTable with the thresholds off)
void launch_pt_apply_blocks(const PairTable &pt, const DeltaRec *blocks, unsigned long long blk, int world, int rank, unsigned long long only_mask,
                            unsigned long long *xstat, unsigned long long *stats, hipStream_t st);  // (not launched for a communicator of one rank: no other rank's block exists; k_fold_list reads the header then)
// phase 2, behind phase 1's kernel boundary, ONE workgroup: every slot noted by an add of this round (PairTable::maybe: pt comes with its
// real thresholds AND the notes) whose pair ended the round at or above a list threshold joins that list -- judged by the FINAL count,
// the same on every rank, so the lists hold the same pairs everywhere and no verdict on them has to be exchanged.  Then the round's
// candidate scan (scan != nullptr) straight into the mailbox.
void launch_fold_list(const PairTable &pt, const DeltaRec *blocks, unsigned long long blk, int world, unsigned long long only_mask, const ScanArgs *scan,
                      unsigned long long *stats, const ZeroBatch &zero, unsigned long long *xstat, bool read_headers /* phase 1 was not launched */, hipStream_t st);
constexpr int XSTAT_WORDS = 8;  // d_xstat: [0] ranks whose block did not fit (bit r), [1] largest record count, [2] -, [3] a rank lost records (-> RoundMailbox::xverdict),
                                // [4..7] sums over the ranks' block headers (-> RoundMailbox::xsum[0..3])
void launch_fold_stats(unsigned long long *stats, unsigned int *n_keys, hipStream_t st);
void launch_round_begin(const RuleSlot *src_rules, unsigned int n_slots, RuleSlot *dst_rules, unsigned int *work_n_a, unsigned int *work_n_b,
                        const uint32_t *src_bloom, uint32_t *dst_bloom, hipStream_t st);
void launch_hot_rebuild(const PairTable &pt, hipStream_t st);
// class C (k_giant.hip): K3 (merge=false) / K4 (merge=true) for tiles of words longer than TILE_NOM_B tokens; scratch = 4*slot
// uint32 per tile
void launch_giant(bool merge, const TileSet &ts, unsigned int slot, const PairTable &pt, const DeltaBuf &db, const RuleSlot *rules,
                  unsigned int rule_mask, uint32_t self_x, uint32_t self_z, uint32_t *scratch, unsigned long long *stats, hipStream_t st);
void launch_pt_clear(const PairTable &pt, hipStream_t st);
void launch_pt_rehash(const PairTable &src, const PairTable &dst, hipStream_t st);
void launch_pt_zero(const PairTable &pt, const RuleSlot *rules, unsigned int n_slots, unsigned long long self_key, hipStream_t st);
void launch_pt_query(const PairTable &pt, const unsigned long long *keys, unsigned int n, unsigned long long *out, hipStream_t st);
void launch_pt_apply(const PairTable &pt, const DeltaRec *recs, unsigned long long n, hipStream_t st);
void launch_fill_u64(unsigned long long *p, unsigned long long v, unsigned long long n, hipStream_t st);

// ---- batch encode (k_encode.hip)
constexpr int ENC_BLOOM_WORDS = 8192;    // 32 KB of LDS: 8 bits per rule at 32k rules
constexpr int ENC_WAVES_PER_BLOCK = 8;   // 512 threads; 48 KB of working arrays + the 32 KB filter = 80 KB, two workgroups per CU
                                         // (measured per 1e7 sentences: 8 waves 76 ms, 10 waves x 384 tokens 104 ms, 6 waves 168 ms)
constexpr int ENC_LDS_TOKENS = 512;      // a sentence of B bytes has <= B+1 tokens: up to 511 bytes work in LDS, longer ones in HBM scratch
// One 32-bit hash of a token pair serves the rule hash (low bits = slot) and the Bloom filter (top 13 bits = word,
// 3 x 5 bits of a second multiply = bit positions).  64-bit multiplies cost ~8 VALU instructions each on CDNA; this is 9 in all.
__host__ __device__ inline uint32_t enc_hash(uint32_t a, uint32_t b) {
  uint32_t h = a * 0x9E3779B1u;
  h ^= b + 0x7F4A7C15u + (h << 6) + (h >> 2);
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}
// Blocked Bloom filter of all rule keys (one 32-bit word, 3 bits per key), resident in LDS: most adjacent pairs have no
// rule, and this answers "certainly none" without leaving the CU.  The host fills it with the same functions.
__host__ __device__ inline uint32_t enc_bloom_bits(uint32_t h) {
  const uint32_t g = h * 0x27D4EB2Fu;
  return (1u << (g >> 27)) | (1u << ((g >> 22) & 31)) | (1u << ((g >> 17) & 31));
}
__host__ __device__ inline uint32_t enc_bloom_word(uint32_t h) { return h >> 19; }  // 13 bits = ENC_BLOOM_WORDS
struct EncModel {
  const uint32_t *cpmap;      // [N_CODEPOINTS]: final token id, CP_SPACE, CP_UNK
  const RuleSlot *rules;      // hash (x<<32|y) -> RuleSlot{z, pad = rule index = priority}
  const uint32_t *rule_z;     // [n_rules] z of rule i
  const unsigned long long *rule_xy;  // [n_rules] x<<32|y of rule i
  const uint32_t *bloom;      // [ENC_BLOOM_WORDS] blocked Bloom filter of the rule keys (staged into LDS)
  unsigned int rule_mask;
  uint32_t n_rules;
  uint32_t z_affine, z_base, z_bp[4];  // rule_z[r] == z_base + r + #{k : z_bp[k] <= r} when z_affine 
  uint32_t space_id;
  int unk_id, bos_id, eos_id;
};
// offsets[n_sent + 1], ends == nullptr: sentences back to back.  ends != nullptr: item j is bytes [offsets[j], ends[j]), any order (the
// word cache's distinct words); its ids land at scratch + 2 offsets[j].
// where the ids of the word cache's distinct words are announced (k_wcache.hip): item u's table slot uslot[u] (u < n_table), or the entry
// u - n_table of the words too long to cache, becomes ids offset << 20 | count (offset, count for the long ones)
struct WordPublish {
  unsigned long long *slot;
  const uint32_t *uslot;
  unsigned long long n_table;
  unsigned long long *extra;
  unsigned long long text_bytes;  // size of the text buffer (wide loads stay inside it)
};
void launch_encode(const EncModel &m, const uint8_t *text, const unsigned long long *offsets, const unsigned long long *ends,
                   unsigned long long n_sent, int bos,
                   int eos, int reverse, int32_t *scratch_ids, uint32_t *counts, uint32_t *work, unsigned long long work_stride,
                   unsigned int n_blocks, double dropout_prob, unsigned long long seed, uint32_t *drop_scratch,
                   unsigned long long drop_stride, hipStream_t st, const WordPublish *pub = nullptr);
void launch_encode_gather(const int32_t *scratch_ids, const unsigned long long *offsets, const unsigned long long *ends,
                          const unsigned long long *out_off, unsigned long long n_sent, int32_t *ids_out, hipStream_t st);

// ---- N4: word cache of the batch encoder (k_wcache.hip) ----
struct WordCache {
  unsigned long long *slot;   // [mask + 1] key of a distinct word (PT_EMPTY = free); after launch_wcache_publish: ids offset << 20 | count
  unsigned long long *pos;    // [mask + 1] first byte of the word's first occurrence
  unsigned long long mask;
  unsigned long long short_mask;  // words of up to 7 bytes hash into the first short_mask + 1 slots (<= mask)
  uint32_t *occ;              // [(bytes + sentences) / 2 + 2] per word occurrence (index (first byte + sentence) / 2): its slot; 0xffffffff elsewhere
  unsigned long long *extra;  // [extra_cap][2] words too long to cache: begin, end; after publish: ids offset, count
  unsigned int *extra_n;
  unsigned int extra_cap;
  unsigned int *status;       // bit 0: the table was too full; bit 1: (also) for a word of up to 7 bytes
};
unsigned long long wcache_count_blocks(const WordCache &wc);
void launch_wcache_insert(const EncModel &m, const uint8_t *text, unsigned long long total, const unsigned long long *offsets, unsigned long long n_sent,
                          const WordCache &wc, hipStream_t st);
void launch_wcache_count_slots(const WordCache &wc, uint32_t *blk_cnt, hipStream_t st);
void launch_wcache_list(const WordCache &wc, const unsigned long long *blk_off, unsigned long long n_table, unsigned long long *ustart,
                        unsigned long long *uend, uint32_t *uslot, hipStream_t st);
void launch_wcache_count(const unsigned long long *offsets, unsigned long long n_sent, const WordCache &wc, int n_fixed, uint32_t *counts, hipStream_t st);
void launch_wcache_scatter(const EncModel &m, const unsigned long long *offsets, unsigned long long n_sent, const WordCache &wc, const int32_t *uids, int bos,
                           int eos, int reverse, const unsigned long long *out_off, int32_t *ids_out, hipStream_t st);

// ---- N3: device decode, and the encoder's result as a padded matrix (k_decode.h, compiled with k_encode.hip) ----
constexpr uint32_t DEC_INVALID = 0x80000000u;  // piece_off[id] with this bit: the host's id_to_subword refuses the id
struct DecTable {
  const uint8_t *blob;        // the text of every id back to back: id_to_subword(id, replace_space = true)
  const uint32_t *piece_off;  // [vocab + 1]
  uint32_t vocab;
};
struct DecIgnore {
  const uint32_t *bitmap;  // bit per id of [0, vocab)
  const int32_t *extra;    // ignored ids outside [0, vocab): they cannot sit in the bitmap, yet suppress the range error for themselves
  uint32_t n_extra;
  uint32_t any;            // 0: nothing is ignored, neither table is read
};
struct DecInput {  // sentence s = ids[offsets[s] .. offsets[s+1]), or (offsets == nullptr) ids[s * stride .. s * stride + min(width, lengths[s]))
  const int32_t *ids;
  const unsigned long long *offsets;
  const int32_t *lengths;  // padded only; nullptr: every row has `width` ids
  unsigned long long width, stride;  // padded only; 1 <= stride, width <= stride
  unsigned long long n_sent;
};
// The two-pass kernels below take both passes' arguments: write == false is the measure pass (out_len / count, and decode's bad_min), write == true
// the write pass (out_off, the exclusive scan of the measure's counts, and out, 16-byte aligned); a pass's kernel is handed null for the other's.
// n_flat: ids (ragged) or n_sent * stride (padded) -- sizes the groups of sentences.  *bad_min must hold ~0 before the measure pass.
// newline (ragged input only, the same in both passes): a '\n' behind every sentence, counted in out_len.
void launch_decode(bool write, bool newline, const DecInput &in, const DecTable &tb, const DecIgnore &ig, unsigned long long n_flat, uint32_t *out_len,
                   unsigned long long *bad_min, const unsigned long long *out_off, uint8_t *out, hipStream_t st);
void launch_enc_longest(const unsigned long long *out_off, unsigned long long n_sent, unsigned int *longest /* holds 0 before the launch */, hipStream_t st);
void launch_enc_pad(const int32_t *ids, const unsigned long long *out_off, unsigned long long n_sent, unsigned long long width, int32_t pad_value,
                    int32_t *matrix /* 4-byte aligned */, int32_t *lengths, hipStream_t st);

// ---- SUBWORD output (k_subword.h, compiled with k_encode.hip): measure -> launch_exclusive_scan -> write ----
struct SubInput {  // sentence s = text[soff[s] .. soff[s+1]) and the ids K5 left for it, ids[ioff[s] .. ioff[s+1])
  const uint8_t *text;
  const unsigned long long *soff;
  const int32_t *ids;
  const unsigned long long *ioff;
  unsigned long long n_sent;
  int32_t unk_id;
  int reverse;  // the ids are stored back to front
};
// tb: the pieces as id_to_subword(id, replace_space = false) gives them (no DEC_INVALID marks).  n_ids sizes the groups of sentences.
void launch_subword(bool write, const EncModel &m, const SubInput &in, const DecTable &tb, unsigned long long n_ids, uint32_t *out_len,
                    const unsigned long long *out_off /* [n_sent + 1] */, uint8_t *out, hipStream_t st);

// ---- byte spans (k_spans.h, compiled with k_encode.hip): one pass, 8 bytes per id ----
// piece_units[vocab]: the units an id covers (1 for unk_id, else the code points of its piece other than U+2581).  spans: uint32 [n_ids][2],
// 8-byte aligned, (start, end) of stored id k relative to its sentence's first byte.  *bad (holds 0 before the launch) becomes 1 where the ids
// of a sentence do not fit its text.  n_ids sizes the groups of sentences.
void launch_spans(const EncModel &m, const SubInput &in, const uint32_t *piece_units, uint32_t vocab, unsigned long long n_ids, uint32_t *spans, uint32_t *bad,
                  hipStream_t st);
// spans + ioff -> uint32 [n_sent, width][2], the tail of a row (0, 0).  matrix: 8-byte aligned; rows must fit.
void launch_spans_pad(const uint32_t *spans, const unsigned long long *ioff, unsigned long long n_sent, unsigned long long width, uint32_t *matrix,
                      hipStream_t st);

// ---- the lines of a text in HBM (k_lines.h, compiled with k_encode.hip): count -> launch_exclusive_scan -> write, then the longest line ----
// d_text: any address.  lines_tiles: entries of cnt (the scan's input; 0: a text of fewer than two bytes holds no newline that starts a line).
unsigned long long lines_tiles(const void *d_text, unsigned long long n_bytes);
void launch_lines_count(const uint8_t *d_text, unsigned long long n_bytes, uint32_t *cnt, hipStream_t st);
// rank: the exclusive scan of cnt; off[n_lines + 1], n_lines = (sum of cnt) + 1: line i = text[off[i] .. off[i + 1]) with its newline
void launch_lines_write(const uint8_t *d_text, unsigned long long n_bytes, const unsigned long long *rank, unsigned long long *off, unsigned long long n_lines,
                        hipStream_t st);
void launch_lines_longest(const unsigned long long *off, unsigned long long n_lines, unsigned long long *longest /* holds 0 before the launch */, hipStream_t st);

// ---- decimal id text (k_idtext.h, compiled with k_encode.hip): measure -> launch_exclusive_scan -> write, both ways ----
// the parser: line i = text[loff[i] .. loff[i + 1]) with its newline (the offsets launch_lines_write left; text: any address) -> count[n_lines],
// then the ids `while (ss >> x)` reads from each line at ids[out_off[i] ..), out_off the exclusive scan of count.  n_bytes sizes the groups of lines.
void launch_idparse(bool write, const uint8_t *text, const unsigned long long *loff, unsigned long long n_lines, unsigned long long n_bytes, uint32_t *count,
                    const unsigned long long *out_off, int32_t *ids, hipStream_t st);
// the printer: sentence s = ids[ioff[s] .. ioff[s + 1]) -> every id in decimal + one space, then '\n'.  out: 16-byte aligned; out_off: the
// exclusive scan of out_len, [n_sent + 1].  n_ids sizes the groups of sentences.
void launch_idprint(bool write, const int32_t *ids, const unsigned long long *ioff, unsigned long long n_sent, unsigned long long n_ids, uint32_t *out_len,
                    const unsigned long long *out_off, uint8_t *out, hipStream_t st);

// ---- token frequencies (k_idcount.h, compiled with k_encode.hip): one pass, nothing written per id ----
// counts[n_bins + 1] += the histogram of ids[n_ids]: counts[v] the ids equal to v, counts[n_bins] the ids outside [0, n_bins).  ids: any 4-byte
// aligned address; 1 <= n_bins <= 2^31.  The caller zeroes counts where it does not accumulate.
void launch_idcount(const int32_t *ids, unsigned long long n_ids, unsigned long long n_bins, unsigned long long *counts, hipStream_t st);

// ---- the vocabulary restriction (k_restrict.h, compiled with k_encode.hip): measure -> launch_exclusive_scan -> write ----
struct RestrictTable {
  const uint32_t *exp_off;  // [vocab + 1]
  const int32_t *exp_ids;   // the expansion of every id of [0, vocab) back to back (the forward table, or the one with every expansion reversed)
  uint32_t vocab;
};
// sentence s = ids[off[s] .. off[s + 1]) -> out_len[n_sent], the ids of its expansions, then those ids at out[out_off[s] ..), out_off the
// exclusive scan of out_len.  out: 16-byte aligned.  n_ids sizes the groups of sentences.
void launch_restrict(bool write, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent, unsigned long long n_ids,
                     const RestrictTable &tb, uint32_t *out_len, const unsigned long long *out_off, int32_t *out, hipStream_t st);

// ---- the byte fallback (k_bytefb.h, compiled with k_encode.hip): measure -> launch_exclusive_scan -> write ----
// in: the ids and the text they were made from (SubInput).  Every unk_id that stands for an unknown run of its sentence -> the ids first + b of the
// run's valid bytes; out_len[n_sent], then the ids at out[out_off[s] ..), out_off the exclusive scan of out_len.  *saw (holds 0 before the measure
// pass) becomes 1 where the ids hold an unk_id at all: only where it stayed 0 may the write pass be skipped.  out: 16-byte aligned.  n_ids sizes the groups.
void launch_bytefb(bool write, const EncModel &m, const SubInput &in, int32_t first, unsigned long long n_ids, uint32_t *out_len, uint32_t *saw,
                   const unsigned long long *out_off, int32_t *out, hipStream_t st);

// ---- the added tokens (k_added.h, compiled with k_encode.hip): the split and the join, each measure -> launch_exclusive_scan -> write ----
struct AddedTable {  // the matcher's tables (added_plan.h added_tables), only read
  unsigned long long first[4];  // bit b: a token starts with byte b
  const uint32_t *one;          // [256] the token that is this one byte, or ADDED_NO_TOKEN
  const uint32_t *dir_off;      // [ADDED_DIR + 1]
  const unsigned long long *list;  // added_entry (added_plan.h) of the tokens of two and more bytes, bucket after bucket, longest first
  const uint8_t *blob;
};
// sentence s = text[off[s] .. off[s + 1]) -> cnt[n_sent] = 2 * matches + 1, then (sub_first the exclusive scan of cnt, [n_sent + 1]) the refined
// offsets sub_off[n_sub + 1] and tok[n_sub]: the token's index for a match, -1 for a segment.  text: any address.  n_bytes sizes the groups.
void launch_added_split(bool write, const uint8_t *text, const unsigned long long *off, unsigned long long n_sent, unsigned long long n_bytes,
                        const AddedTable &tb, uint32_t *cnt, const unsigned long long *sub_first, unsigned long long *sub_off, int32_t *tok, hipStream_t st);
struct AddedJoin {  // the refined batch's ids (forward, without bos / eos) and how its sub-sentences make the caller's sentences
  const int32_t *rids;
  const unsigned long long *roff;       // [n_sub + 1]
  const int32_t *tok;                   // [n_sub]
  const unsigned long long *sub_first;  // [n_sent + 1]
  unsigned long long n_sent;
  int32_t first, bos_id, eos_id;  // first: the id of token 0
  int bos, eos, reverse;
};
// out_len[n_sent], then the ids at out[out_off[s] ..), out_off the exclusive scan of out_len.  out: 16-byte aligned.  n_ids sizes the groups.
void launch_added_join(bool write, const AddedJoin &in, unsigned long long n_ids, uint32_t *out_len, const unsigned long long *out_off, int32_t *out,
                       hipStream_t st);

// ---- training blocks (k_blocks.h, compiled with k_encode.hip): flags -> scan -> (whole: orbit) -> measure -> scan -> write (-> keep) ----
// The sequence a call packs: the open row's m sentences (f ids, open_off[m + 1]) followed by the call's S sentences (off[S + 1], off[0] = 0), as one
// stream of `total` = f + K ids in which sentence i starts at voff(i).  Only read.
struct BlkIn {
  const int32_t *open_ids;
  const unsigned long long *open_off;
  unsigned long long m, f;
  const int32_t *ids;
  const unsigned long long *off;
  unsigned long long S, total;
  __host__ __device__ unsigned long long n() const { return m + S; }
  __host__ __device__ unsigned long long voff(unsigned long long i) const { return i < m ? open_off[i] : i >= m + S ? total : f + off[i - m]; }
  __host__ __device__ int32_t id(unsigned long long p) const { return p < f ? open_ids[p] : ids[p - f]; }
};
constexpr unsigned int BLK_ORBIT = 1024;        // sentences a workgroup of the orbit pass resolves
constexpr uint32_t BLK_NONE = 0xffffffffu;      // entry[] of a block of sentences the orbit does not visit
// cnt[n] = 1 per non-empty sentence (its exclusive scan is `ne` below, [n + 1]); n = in.n() < 2^32 - 1
void launch_blk_flags(const BlkIn &in, uint32_t *cnt, hipStream_t st);
// whole mode's rows: nxt[n], hop[n], entry / rowbase[ceil(n / BLK_ORBIT)] (entry holds BLK_NONE before), rowsent[rows + 1] (at most n + 1), *bad (holds ~0
// before) = the smallest index of a sentence longer than L, info[0] = the rows of the orbit, info[1] = the ids of its last row.  n >= 1.
void launch_blk_orbit(const BlkIn &in, unsigned long long L, uint32_t *nxt, unsigned long long *hop, uint32_t *entry, uint32_t *rowbase, uint32_t *rowsent,
                      unsigned long long *bad, unsigned long long *info, hipStream_t st);
// rowsrc[n_rows + 1] and cnt[n_rows], the fragments per row; rowsent == nullptr: stream mode
void launch_blk_measure(const BlkIn &in, const unsigned long long *ne, unsigned long long L, unsigned long long n_rows, const uint32_t *rowsent, uint32_t *cnt,
                        unsigned long long *rowsrc, hipStream_t st);
// rows / seg / pos: 16-byte aligned, n_rows * L elements rounded up to a multiple of 4; frags: 8-byte aligned; 1 <= n_rows * L < 2^31
void launch_blk_write(const BlkIn &in, const unsigned long long *ne, unsigned long long L, unsigned long long n_rows, const unsigned long long *rowsrc,
                      const unsigned long long *row_frags, int32_t pad, int32_t *rows, int32_t *seg, int32_t *pos, int32_t *frags, hipStream_t st);
// the stream from p0 < total on as the next open row: new_ids[total - p0], new_off[m' + 1], info[2] = m'
void launch_blk_keep(const BlkIn &in, const unsigned long long *ne, unsigned long long p0, int32_t *new_ids, unsigned long long *new_off,
                     unsigned long long *info, hipStream_t st);

// ---- batches by length under a token budget (k_batches.h, compiled with k_encode.hip): keys -> radix sort -> cuts; measure -> scan -> write ----
// The lengths a plan sorts: l(i) = off[i + 1] - off[i] (off != nullptr) or len[i], which may be negative.  Only read.
struct BatIn {
  const unsigned long long *off;
  const int32_t *len;
  unsigned long long n;
  __host__ __device__ bool negative(unsigned long long i) const { return !off && len[i] < 0; }
  __host__ __device__ unsigned long long l(unsigned long long i) const { return off ? off[i + 1] - off[i] : (unsigned long long)(uint32_t)len[i]; }
};
struct BatRule {  // the parameters of the rule (include/yttm_mi355x.h), checked by the host; cap = min(T, max_len or T)
  unsigned long long T, M, min_len, max_len, cap;
};
// the plan as the gather reads it
struct BatPlan {
  const uint32_t *order;
  const unsigned long long *batch_first;
  unsigned long long n_batches;
};
constexpr unsigned int BAT_TILE = 4096;    // sentences a workgroup of the sort ranks per pass
constexpr unsigned int BAT_ORBIT = 8192;   // positions a workgroup of the cuts resolves in LDS
constexpr unsigned int BAT_CHUNK = 2048;   // elements a wavefront of the gather writes
constexpr uint32_t BAT_NONE = 0xffffffffu;  // entry[] of a block of positions the orbit does not visit
// the 8-bit passes that sort keys of 0 .. cap + 1
inline unsigned int bat_passes(unsigned long long cap) {
  unsigned int bits = 0;
  for (unsigned long long v = cap + 1; v; v >>= 1) bits++;
  return (bits + 7) / 8;
}
inline unsigned long long bat_tiles(unsigned long long n) { return (n + BAT_TILE - 1) / BAT_TILE; }
// key[n]; info[0] (holds ~0 before) = the smallest index of a negative length or of a kept sentence longer than T; info[1] (0 before) = n_kept
void launch_bat_keys(const BatIn &in, const BatRule &r, uint32_t *key, unsigned long long *info, hipStream_t st);
// one pass of the stable sort by the digit at `shift`: (key_in, idx_in) -> (key_out, idx_out).  idx_in == nullptr: the index is the position;
// key_out == nullptr: the last pass.  hist[256 * tiles] and hist_off[the same] are working arrays, scan_tmp / scan_total those of the scan.
void launch_bat_sort_pass(const uint32_t *key_in, const uint32_t *idx_in, unsigned long long n, unsigned int shift, uint32_t *hist,
                          unsigned long long *hist_off, unsigned long long *scan_tmp, unsigned long long *scan_total, uint32_t *key_out,
                          uint32_t *idx_out, hipStream_t st);
unsigned int bat_orbit_positions();  // the hook YTTM_BATCHES_ORBIT as launch_bat_cuts takes it
// skey[n_kept] = key[order[p]], then the cuts: nxt / hop[n_kept], entry / base[ceil(n_kept / orbit)] (entry holds BAT_NONE before),
// batch_first[n_batches + 1], info[2] = n_batches.  n_kept >= 1.  orbit: the positions a workgroup resolves, 64 .. BAT_ORBIT, a multiple of 64.
void launch_bat_cuts(const uint32_t *key, const uint32_t *order, unsigned long long n_kept, const BatRule &r, unsigned int orbit, uint32_t *skey,
                     uint32_t *nxt, unsigned long long *hop, uint32_t *entry, uint32_t *base, unsigned long long *batch_first,
                     unsigned long long *info, hipStream_t st);
// the gather of one side (ids, off[n + 1]): cnt[n_batches] = rows * width and widths[n_batches], both saturating at 2^32 - 1; *total (0 before) += the
// sum of the counts, exact
void launch_bat_measure(const BatPlan &p, const unsigned long long *off, uint32_t *widths, uint32_t *cnt, unsigned long long *total, hipStream_t st);
// out: 16-byte aligned, n_elems rounded up to a multiple of 4; 1 <= n_elems < 2^31
void launch_bat_write(const BatPlan &p, const int32_t *ids, const unsigned long long *off, const uint32_t *widths,
                      const unsigned long long *batch_off, unsigned long long n_elems, int32_t pad, bool left_pad, int32_t *out, hipStream_t st);

}  // namespace yttm
