// gpu_ctx.cpp -- the trainer's device context (gpu_ctx.h): construction, kernel-family timers, and the merge round (K4) with its one launch and one
// mailbox poll.  The rest of GpuCtx lives in gpu_pool.cpp, gpu_upload.cpp, gpu_frontend.cpp, gpu_pairs.cpp, gpu_exchange.cpp, gpu_words.cpp
// (gpu_ctx_internal.h: what went where).
#include "gpu_ctx_internal.h"

namespace yttm {

GpuCtx::GpuCtx(int device) : m_(new Mem), device_(device) {
  try {
    init();
  } catch (...) {  // (no destructor will run)
    teardown();
    throw;
  }
}

void GpuCtx::init() {
  cfg_refresh();  // the environment hooks are read here, once per context (yttm_config.h); nothing below this constructor calls getenv
  cfg_ = cfg();
  const Config &C = *cfg_;
  xchg_margin_ = C.xchg_margin.d;
  pool_reset_peak();
  pool_arm(C.test_alloc_fail.u);
  HIP_CHECK(hipSetDevice(device_));
  tl_stream = strm();
  tl_device = device_;
  st_raw_ = pool_take_stream(device_);  // (a finished context's: creating and destroying one costs ~2 ms of a training)
  if (!st_raw_) HIP_CHECK(hipStreamCreateWithFlags(&st_raw_, hipStreamNonBlocking));
  tl_stream = strm();
  tl_device = device_;
  m_->ctr.alloc(1);
  m_->d_stats.alloc(STATS_WORDS);  // (yttm_kernels.h: StatWord)
  HIP_CHECK(hipMemsetAsync(m_->d_stats, 0, STATS_WORDS * sizeof(unsigned long long), strm()));  // (stream-ordered like everything that uses them)
  m_->d_round.alloc(1);  // one block for everything the host reads back per round, so that it is ONE device-to-host copy
  hot_cap_ = std::min((unsigned int)C.hot_cap.u, HOT_CAP);
  hot_target_ = (unsigned int)C.hot_target.u;  // measured at 1 GB: 4096..16384 equal on the abcd corpus, 8192 best on Zipf text (4279 rounds)
  hot_min_ = (unsigned int)C.hot_min.u;
  fuse_enabled_ = C.no_fuse.u == 0;
  idx_enabled_ = C.no_index.u == 0;  // (no pair index: no word mode either)
  idx_radix_min_ = C.index_radix_min.u;  // (class-A live tokens from which the index is built by radix partition; tests: 0 / huge)
  idx_agg_min_ = C.index_agg_min.u;  // (fill pass of an index build: postings from which on a workgroup sums them per key in LDS first; tests: 0)
  hot_target_words_ = (unsigned int)C.hot_target_words.u;  // (measured at 1 GB, word mode: 8192 -> 6 rebuilds, candidate family 21.0 ms; 32768 -> 3, 16.9 ms; round 4: 32768 -> 3, 14.6 ms; 65536 -> 2, 12.5; 131072 -> 2, 15.0)
  // rounds of at most this many words (by the hint) whose batch travels in the kernel arguments are ONE launch, k_words<FUSED>; 0: never.
  // (1 GB random text, wall / K4 ms: never 138.3 / 86.0, 32 k 136.6 / 83.3, 256 k 133.1 / 80.2, 2 M 125.9 / 73.5, every round 125.0 / 72.5)
  words_fuse_max_ = (unsigned int)C.words_fuse_max.u;
  word_hint_floor_ = (unsigned int)C.word_hint_floor.u;  // (the words a round is sized for beyond twice the last round's sites; 1 GB random text, K4 ms on the device clock: 1024 -> 73.6, 4096 -> 72.7, 16384 -> 72.1)
  words_inline_max_ = (unsigned int)C.words_inline_max.u;  // (measured at 1 GB, K4 ms: 16 k -> 97.2, 64 k -> 95.4, 256 k -> 94.1)
  profile_events_ = C.profile_events.u != 0;
  words_enabled_ = C.word_mode.u != 0;   // (0: tiles to the end)
  direct_enabled_ = C.k4_direct.u != 0;  // (0: the pair filter + rule hash from the first round on; A/B runs)
  word_div_ = (unsigned int)C.word_div.u;  // (measured at 1 GB: 96 -> K4 135 ms, 150 -> 107, 200 -> 103.7, 300 -> 103.7, 500 -> 104; round 4, merge loop ms of random 'abcd ': 80 / 100 -> 98.7 (switch at
                                               // round 13), 120 -> 96.0 (round 20), 150 -> 96.4, 200 -> 99.4 (round 29), 400 -> 101.6 -- but the CJK-shaped corpus: 120 -> 485 ms, 200 -> 472: left at 200;
                                               // round 5, with class B's repack looks no longer a sync every second word-mode round: CJK 120 / 200 / 300 -> 493 / 493 / 492 ms, 'abcd ' 100 / 120 / 150 / 200 ->
                                               // 113.4 / 110.8 / 110.8 / 112.7 ms: 150)
  word_min_tiles_ = (unsigned int)C.word_min_tiles.u;  // (tests: 0 = switch as soon as the hot list is active)
  // a pass over the tiles must cost more than word mode's three launches: 1 GB enwik-like text (25 M tokens, 48 us per dense round) got 15 % slower
  // in word mode, the 1 GB CJK-shaped corpus (337 M tokens) 21 % faster, random 'abcd ' (94 M tokens at the switch) 10 % faster
  word_min_tokens_ = C.word_min_tokens.u;
  no_batch_args_ = C.no_batch_args.set;
  trace_rounds_ = C.trace_rounds.c_str();  // (points into cfg_, which this context keeps)
  dbg_cand_ = C.dbg_cand.c_str();
  m_->d_hot_slots.alloc(HOT_CAP);
  m_->d_hot_ctl.alloc(1);
  HIP_CHECK(hipMemsetAsync(m_->d_hot_ctl, 0, sizeof(ListCtl), strm()));
  top_cap_ = std::max(16u, std::min((unsigned int)C.top_cap.u, TOP_CAP));
  top_target_ = (unsigned int)C.top_target.u;  // about four times what the host looks at per round
  top_min_ = (unsigned int)C.top_min.u;
  m_->d_top_slots.alloc(TOP_CAP);
  m_->d_top_ctl.alloc(1);
  HIP_CHECK(hipMemsetAsync(m_->d_top_ctl, 0, sizeof(ListCtl), strm()));
  HIP_CHECK(hipMemsetAsync(m_->d_round, 0, offsetof(RoundBlock, cand), strm()));  // k_hot_scan leaves its counters zeroed for the next call
  cand_cap_ = CAND_CAP;
  m_->d_rules.alloc(RULES_CAP);
  rules_cap_ = RULES_CAP;
  h_pin_ = (PinBlock *)pool_take_pin();  // pinned staging: one buffer is kept across contexts (hipHostMalloc of 17 MB costs milliseconds)
  if (!h_pin_) HIP_CHECK(hipHostMalloc((void **)&h_pin_, PIN_BYTES, hipHostMallocDefault));
  memset(&h_pin_->mailbox, 0, offsetof(RoundMailbox, cand));  // (round_id: no round is published)
}

GpuCtx::~GpuCtx() { teardown(); }

// The stream is synchronised, then every block goes back to the pool, then the pool is told that the stream is idle (its blocks may go to
// anybody); only then the pin block and the stream are handed on.
void GpuCtx::teardown() {
  (void)hipSetDevice(device_);
  tl_stream = strm();
  tl_device = device_;
  if (st_raw_) (void)hipStreamSynchronize(strm());
  for (hipEvent_t e : all_events_) (void)hipEventDestroy(e);
  m_.reset();
  pool_quiesce(strm());
  if (h_pin_ && pool_give_pin(h_pin_)) h_pin_ = nullptr;
  if (h_pin_) (void)hipHostFree(h_pin_);
  if (st_raw_ && pool_give_stream(device_, st_raw_)) st_raw_ = nullptr;  // (synchronised above: nothing is pending on it)
  if (st_raw_) (void)hipStreamDestroy(st_raw_);
}

bool GpuCtx::one_launch_rounds() const {
  if (!(word_global_ && words_fuse_max_ != 0 && fuse_enabled_ && !instrument && hot_state_ == HOT_ACTIVE && top_state_ == TOP_ACTIVE)) return false;
  return multi() || (word_mode_ && idx_valid_ && !m_->cls[2].n_tiles);
}

void GpuCtx::sync() { HIP_CHECK(hipStreamSynchronize(strm())); }
void GpuCtx::read_stats(int first, int n, unsigned long long *out) {
  HIP_CHECK(hipMemcpyAsync(out, m_->d_stats + first, (size_t)n * 8, hipMemcpyDeviceToHost, strm()));
  sync();
}

// Kernel-family timers (profile mode): HIP events on the context's stream.  Events come from a process-wide pool, and an
// interval that starts where the previous one ended shares that event (t_end(..., chain=true) followed by t_begin): a
// merge round costs two hipEventRecord calls instead of four -- on Zipf text (4279 rounds) the four cost 17 % of a step.
static std::vector<hipEvent_t> g_event_pool;
static hipEvent_t event_get() {
  {
    std::lock_guard<std::mutex> g(pool_mutex());
    if (!g_event_pool.empty()) {
      hipEvent_t e = g_event_pool.back();
      g_event_pool.pop_back();
      return e;
    }
  }
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  return e;
}
void GpuCtx::t_begin(int which) {
  (void)which;
  if (!profile) return;
  if (chain_event_) {  // nothing was enqueued since the interval that ended there
    cur_a_ = chain_event_;
    chain_event_ = nullptr;
    return;
  }
  cur_a_ = event_get();
  all_events_.push_back(cur_a_);
  HIP_CHECK(hipEventRecord(cur_a_, strm()));
}
void GpuCtx::t_end(int which, unsigned long long bytes, bool chain) {
  kt.launches[which]++;
  kt.bytes[which] += bytes;
  if (!profile) return;
  hipEvent_t b = event_get();
  all_events_.push_back(b);
  HIP_CHECK(hipEventRecord(b, strm()));
  evs_.push_back(Ev{cur_a_, b, which});
  cur_a_ = nullptr;
  chain_event_ = chain ? b : nullptr;
}
void GpuCtx::resolve_timers() {
  sync();
  {
    // K4 algorithmic traffic: every live token is read once (4 B); the tiles that had a merge site are
    // counted once more as re-read and rewritten (8 B per token of those -- an upper bound since single-site tiles are
    // rewritten from the registers they were loaded into)
    unsigned long long st[8] = {0};
    if (pt_cap_) launch_fold_stats(m_->d_stats, pt_.n_keys, strm());
    sync();
    if (hipMemcpy(st, m_->d_stats, sizeof st, hipMemcpyDeviceToHost) == hipSuccess) {
      merge_sites = st[STAT_SITES];
      kt.bytes[KT_MERGE] = 4 * st[STAT_TOKENS] + 8 * st[STAT_TOUCHED_TOKENS];
      touched_tiles = st[STAT_TOUCHED];
      touched_tile_tokens = st[STAT_TOUCHED_TOKENS];
      touched_words = st[STAT_INSTR_WORDS];
      touched_word_tokens = st[STAT_INSTR_TOKENS];
    }
  }
  FILE *trace = cfg_->trace.set ? fopen(cfg_->trace.raw.c_str(), "w") : nullptr;  // per-launch times for tuning
  for (auto &e : evs_) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) kt.ms[e.which] += ms;
    if (trace) fprintf(trace, "%d %.4f\n", e.which, ms);
  }
  evs_.clear();
  if (trace)  // (rounds timed by the device: already in kt.ms; listed after the event-timed ones -- nearly every round of a single-GPU training)
    for (float ms : dev_round_ms_) fprintf(trace, "%d %.4f\n", (int)KT_MERGE, ms);
  dev_round_ms_.clear();
  {
    std::lock_guard<std::mutex> g(pool_mutex());
    g_event_pool.insert(g_event_pool.end(), all_events_.begin(), all_events_.end());
  }
  all_events_.clear();
  chain_event_ = nullptr;
  if (trace) fclose(trace);
}

// ------------------------------------------------------------------------------------------------- K4
// One merge round's values, carried between the steps of merge_apply.
struct GpuCtx::Round {
  const uint32_t *xyz;
  uint32_t k;
  const unsigned long long *rule_counts;
  uint32_t vmax = 0, z_base = 0;
  unsigned int cap = 64;                       // slots of the batch's rule hash
  uint32_t self_x = 0xffffffffu, self_z = 0;   // at most one x == y rule, passed by value
  bool by_args = false;                        // the batch travels in the kernel arguments (ba.k != 0)
  BatchArgs ba{};
  ScanArgs sa{};                               // the candidate scan that rides in the round's last kernel (sa.on == 0: none)
  ScanArgs xa{};                               // multi-GPU: what the word-mode launches get instead
  bool dev_timing = false, marked = false;
  int last_cls = 0;
  PairTable kpt{};
  // at most this many distinct pairs can the round touch on a rank: per rule at most five updates per site (sites <= the pair's global count) and
  // at most four pairs per token type ((a,x), (a,z), (y,b), (z,b)) plus the self pairs.  The same number on every rank (it is computed from the
  // batch and the global counts).
  unsigned long long touch_bound() const {
    unsigned long long b = 0;
    for (uint32_t j = 0; j < k; j++) b += std::min<unsigned long long>(rule_counts ? 5 * rule_counts[j] : ~0ull >> 8, 4ull * (vmax + 1) + 4);
    return b;
  }
  BatchArgs first_ba() {  // the BatchArgs of the round's next launch: the first one carries the mark
    BatchArgs b = ba;
    if (dev_timing && !marked) { b.mark = 1u; marked = true; }
    return b;
  }
};

void GpuCtx::merge_apply(const uint32_t *xyz, uint32_t k, const unsigned long long *rule_counts, const unsigned long long *next_tau_cnt,
                         uint32_t next_tau_mx, uint32_t next_want) {
  HIP_CHECK(hipSetDevice(device_));
  tl_stream = strm();
  tl_device = device_;
  if (!k) return;
  if (!n_tiles && !multi()) return;  // a rank without words still takes part in the exchange
  if (k > RULES_CAP / 2) throw GpuError{"merge_apply: batch too large"};
  Round r{xyz, k, rule_counts};
  round_capacity(r);
  round_word_mode(r);
  round_batch(r);
  round_scan(r, next_tau_cnt, next_tau_mx, next_want);
  if (multi()) round_block_size(r);
  round_launch(r);
  merge_rounds++;
  round_trace(r);
  round_finish(r);
  // single GPU: no sync here -- the candidate filter that always follows reads n_keys back together with its results
  // (its sync also makes the pinned rule staging reusable for the next round)
  // every occurrence of the batch's pairs has been merged (on every rank): their counts are exactly zero.  The candidate
  // filter that follows zeroes them while it reads the hot list; any other reader goes through flush_pending_zero().
}

// the batch's shape, and room for what it can add: the pair table and (multi-GPU) the delta table
void GpuCtx::round_capacity(Round &r) {
  // new pairs this round: every site adds <= 2 neighbours (+ the z,z run pair); distinct new keys per rule are also
  // bounded by the number of live token types on either side
  r.z_base = r.xyz[2];
  for (uint32_t j = 0; j < r.k; j++) {
    r.vmax = std::max(r.vmax, r.xyz[3 * j + 2]);
    if (r.xyz[3 * j + 2] != r.z_base + j) throw GpuError{"merge_apply: the new ids of a batch must be consecutive"};
  }
  if (r.vmax >= (1u << 29)) throw GpuError{"merge_apply: token ids must be below 2^29"};
  unsigned long long bound_new = 0;
  for (uint32_t j = 0; j < r.k; j++) {
    unsigned long long by_tokens = 2ull * (r.vmax + 1) + 1;
    unsigned long long by_count = r.rule_counts ? 3 * r.rule_counts[j] : by_tokens;
    bound_new += std::min(by_tokens, by_count);
  }
  // (the key count the scans report is one round old -- they fold the statistics after publishing: the previous round's bound covers it)
  ensure_table_capacity(n_keys_host + bound_prev_ + bound_new);
  bound_prev_ = bound_new;
  if (multi() && !delta_cap_forced_) {
    // distinct pairs this rank's round can touch (Round::touch_bound): every rank regrows its table in the same round -- an overflow is a
    // bug, not a workload.
    const unsigned long long dt_bound = r.touch_bound();
    if (dt_bound > send_cap_) {
      unsigned long long cap = db_.mask + 1;
      while (cap / 2 < dt_bound) cap <<= 1;
      chain_event_ = nullptr;
      alloc_delta_table(cap);
      delta_regrows++;
    }
  }
}

// Word mode pays when the last round's merge sites are few against the tokens a pass over the tiles streams, and a pass is expensive
// (numbers of one context, or summed over `ranks` of them).
bool GpuCtx::word_mode_pays(unsigned long long tiles_a, unsigned long long sites, unsigned long long tokens, unsigned long long ranks) const {
  return tiles_a >= (unsigned long long)word_min_tiles_ * ranks && tiles_a && sites != ~0ull && tokens && tokens >= word_min_tokens_ * ranks &&
         (word_div_ == 0 || sites * (unsigned long long)word_div_ < tokens);
}

void GpuCtx::round_word_mode(const Round &r) {
  // Word mode: on when word_mode_pays (and then for good).  Single GPU: this context's numbers.  Multi-GPU: the ranks' numbers summed
  // (block headers -> mailbox), per rank on average -- the same verdict on every rank in the same round; a rank without class-A tiles
  // follows the decision without switching.
  if (!word_global_ && words_enabled_ && idx_enabled_ && !instrument && hot_state_ == HOT_ACTIVE) {
    const bool go = multi() ? word_mode_pays(g_tiles_a_, g_sites_last_, g_tokens_last_, (unsigned long long)comm_->world)
                            : word_mode_pays(m_->cls[0].n_tiles, sites_last_, live_tokens_last_, 1);
    if (go) {
      word_global_ = true;
      if (m_->cls[0].n_tiles) enter_word_mode(r.z_base);
      else word_switch_round = merge_rounds;
    }
  }
  if (word_mode_) {
    if (*(volatile unsigned int *)tl_.broken) idx_pending_ = true;  // (the last round is over: its mailbox has been read)
    if (idx_pending_) build_index(r.z_base);
  }
}

void build_rule_hash(RuleSlot *tab, unsigned int cap, const uint32_t *rules, unsigned int stride, uint32_t k) {
  for (unsigned int i = 0; i < cap; i++) { tab[i].key = PT_EMPTY; tab[i].z = 0; tab[i].pad = 0; }
  for (uint32_t j = 0; j < k; j++) {
    const uint32_t x = rules[stride * j], y = rules[stride * j + 1];
    if (x == y) continue;
    const unsigned long long key = pair_key(x, y);
    unsigned int h = pair_hash32(key) & (cap - 1);
    while (tab[h].key != PT_EMPTY) h = (h + 1) & (cap - 1);
    tab[h].key = key;
    tab[h].z = stride > 2 ? rules[stride * j + 2] : 0;
  }
}

// the batch: rule hash (x != y rules) + at most one x == y rule passed by value
void GpuCtx::round_batch(Round &r) {
  while (r.cap < 2 * r.k) r.cap <<= 1;
  for (uint32_t j = 0; j < r.k; j++) {
    const uint32_t x = r.xyz[3 * j], y = r.xyz[3 * j + 1], z = r.xyz[3 * j + 2];
    if (x >= id_cap_ || y >= id_cap_ || z >= id_cap_) throw GpuError{"merge_apply: token id out of range"};
    if (x == y) {
      if (r.self_x != 0xffffffffu) throw GpuError{"merge_apply: more than one x==y rule in a batch"};
      r.self_x = x;
      r.self_z = z;
    }
  }
  // A small batch goes to the kernels as an argument and nothing is uploaded (yttm_kernels.h: BatchArgs); a larger one (or any, with
  // class-C tiles: k_giant reads the rule hash from HBM) travels through k_round_begin.
  r.by_args = r.k <= (uint32_t)BATCH_ARGS_MAX && !m_->cls[2].n_tiles && !no_batch_args_;
  // (the common small batch needs no rule hash: the host's share of a round is on the critical path)
  if (!r.by_args) build_rule_hash(h_pin_->rules, r.cap, r.xyz, 3, r.k);
  r.ba.instr = instrument ? 1u : 0u;
  const uint32_t max_in = max_id_;  // largest id a tile can hold BEFORE this round (the ids the site search looks up)
  max_id_ = std::max(max_id_, r.vmax);
  if (r.by_args) {
    r.ba.k = r.k;
    r.ba.direct_v = direct_enabled_ && max_in + 1 <= DIRECT_MAX_V ? max_in + 1 : 0u;  // (the first rounds of a small alphabet: k_tiles<.., DIRECT>)
    for (uint32_t j = 0; j < r.k; j++) { r.ba.xy[2 * j] = r.xyz[3 * j]; r.ba.xy[2 * j + 1] = r.xyz[3 * j + 1]; }
  }
}

// One launch per round: the candidate scan rides in the tail of the round's last kernel -- single GPU: the apply kernel of class A (class
// B goes first: the one-wave workgroups of class B took longer over the tail than the launch it saved; class-C tiles -- words of more
// than 2048 tokens -- keep the separate scan); multi-GPU: the fold kernel behind the all-gather (exchange_round), whatever the classes.
void GpuCtx::round_scan(Round &r, const unsigned long long *next_tau_cnt, uint32_t next_tau_mx, uint32_t next_want) {
  ScanArgs &sa = r.sa;
  fused_pending_ = false;
  r.last_cls = m_->cls[0].n_tiles ? 0 : 1;
  if (next_tau_cnt && fuse_enabled_ && hot_state_ == HOT_ACTIVE && top_state_ == TOP_ACTIVE && !instrument &&
      (multi() || ((m_->cls[0].n_tiles || m_->cls[1].n_tiles) && !m_->cls[2].n_tiles))) {
    sa = scan_args(*next_tau_cnt, next_tau_mx, ++mail_round_);
    if (sa.tau_cnt < pt_.top_tau) {  // the list is complete only from top_tau up (as in candidates())
      sa.tau_cnt = pt_.top_tau;
      sa.tau_mx = 0xffffffffu;
    }
    sa.want = next_want;  // (the scan may raise the threshold to about this many candidates: scan_top)
    sa.done_ctr = &m_->d_hot_ctl->ticket;
    fused_pending_ = true;
    fused_tau_ = *next_tau_cnt;
    fused_mx_ = next_tau_mx;
    fused_round_ = sa.round_id;
  }
  // Multi-GPU: what the word-mode launches get instead of the scan (ScanArgs::on == 2): the round's last workgroup only leaves the
  // worklist counters at zero; a one-launch round has not even that to do (launch_words_apply: on = 3).  (Packing the delta table in this
  // tail as well was measured: ONE workgroup walking ten thousand claimed slots across XCDs took 45 us -- k_dt_pack's hundred take 6.)
  if (multi()) {
    r.xa.on = 2u;
    r.xa.done_ctr = &m_->d_hot_ctl->ticket;
  }
  // A fused round is timed by the device itself (its first launch notes the time, the tail reports the difference in the mailbox):
  // no hipEventRecord on the round's critical path (two per round were 4 us of host time: 8 % of a Zipf step).  YTTM_PROFILE_EVENTS=1
  // keeps the events (cross-check).
  r.dev_timing = profile && sa.on && !profile_events_;
  sa.timed = r.dev_timing ? 1u : 0u;
  dev_timing_pending_ = r.dev_timing;
}

// multi-GPU, this round's blocks: sized for what the busiest rank will send, predicted from the batch -- its summed pair counts are its merge sites
// over all ranks -- and the records per site of the last two rounds, with a margin of three (a block that is too small costs a second
// exchange and a scan of its own, ~60 us; one that is too large costs bytes on the links); never more than the round can touch at all
// (Round::touch_bound).  Every input is the same on every rank.
void GpuCtx::round_block_size(const Round &r) {
  unsigned long long sites = 0;
  for (uint32_t j = 0; j < r.k; j++) sites += r.rule_counts ? r.rule_counts[j] : 0;
  const unsigned long long bound = r.touch_bound();
  xch_sites_ = sites;
  const double margin = xchg_margin_;  // (YTTM_XCHG_MARGIN; tests: a margin below one forces the repeat path)
  const double pred = r.rule_counts ? std::max(xrate_[0], xrate_[1]) * (double)sites * margin : (double)bound;
  unsigned long long need = (unsigned long long)std::min((double)std::min<unsigned long long>(bound, send_cap_), pred) + XHDR;
  unsigned long long b2 = blk_min_;
  while (b2 < need) b2 <<= 1;
  blk_ = b2;
}

// the tail of class ci's launch: the scan (single GPU) or the exchange tail (multi-GPU) in the round's last tile-class launch, nothing elsewhere
const ScanArgs *GpuCtx::tail_of(const Round &r, int ci) const {
  if (ci != r.last_cls) return nullptr;
  if (multi()) return ci == 0 && word_mode_ ? &r.xa : nullptr;  // (the tile kernels have nothing to do in a tail)
  return r.sa.on ? &r.sa : nullptr;
}

static int hook_or_auto(const Hook &h) { return h.set && !h.raw.empty() ? (int)h.i : -1; }  // (a test's grid hook; -1: the launcher's own choice)

void GpuCtx::round_launch(Round &r) {
  if (!r.dev_timing) t_begin(KT_MERGE);
  if (!r.by_args) {
    pm_bloom_host(h_pin_->bloom, r.xyz, r.k);  // the batch's pair filter for the apply kernels (built here: a few hundred hashes)
    if (!m_->d_bloom) m_->d_bloom.alloc(PM_BLOOM_WORDS_H);
    launch_round_begin(h_pin_->rules, r.cap, m_->d_rules, m_->cls[0].n_tiles ? m_->cls[0].d_work_n.p : nullptr, m_->cls[1].n_tiles ? m_->cls[1].d_work_n.p : nullptr, h_pin_->bloom, m_->d_bloom, strm());
  }
  r.kpt = multi() ? pt_nolist() : pt_;  // (multi-GPU: the lists are filled behind the exchange, by the final counts -- k_fold_list)
  // Class B, then class A (tiles, or word mode's k_words), on the context's one stream: stream order is the only synchronisation between
  // the round's launches, and the last of them carries the tail (tail_of).
  for (int ci = 1; ci >= 0; ci--) {
    if (!m_->cls[ci].n_tiles) continue;
    if (ci == 0 && word_mode_) {
      round_launch_words(r);
      continue;
    }
    const BatchArgs tba = r.first_ba();
    launch_merge_apply(ci, m_->cls[ci].ts, r.kpt, db_, m_->d_rules, r.cap - 1, r.self_x, r.self_z, r.z_base, m_->d_stats, &tba, tail_of(r, ci), m_->d_bloom,
                       (unsigned int)cfg_->apply_grid.i, strm());
    if (ci == 1 && word_mode_) classb_word_rounds++;
  }
  launch_giant(true, m_->cls[2].ts, m_->cls[2].slot, r.kpt, db_, m_->d_rules, r.cap - 1, r.self_x, r.self_z, m_->cls[2].d_scratch, m_->d_stats, strm());
  if (r.dev_timing) kt.launches[KT_MERGE]++;
  else t_end(KT_MERGE, 0, /*chain=*/!r.sa.on);  // (a fused round is followed by the host's turn, not by another kernel: its end event must not start the next interval)
}

// class A in word mode: the batch's rules -> worklist of words (k_wgather; it also allots the new tokens' instance lists), then the words (k_words)
void GpuCtx::round_launch_words(Round &r) {
  WordClass &c = m_->cls[0];
  const uint32_t *d_xyz = nullptr;
  if (!r.by_args) {
    memcpy(h_pin_->xyz, r.xyz, (size_t)r.k * 12);
    HIP_CHECK(hipMemcpyAsync(m_->d_xyz, h_pin_->xyz, (size_t)r.k * 12, hipMemcpyHostToDevice, strm()));
    d_xyz = m_->d_xyz;
  }
  if (r.k > WGATHER_MAXK) throw GpuError{"merge_apply: batch too large for the word-mode gather"};
  WGatherArgs ga{};  // (the worklist's length is at zero: enter_word_mode, then every round's k_delta_apply)
  ga.ix = idx_;
  ga.ix_valid = idx_valid_ ? 1u : 0u;
  ga.z_static = idx_valid_ ? idx_zbuild_ : 0xffffffffu;  // (no index: every rule is "not found", the round takes every word)
  ga.tl = tl_;
  ga.stamp = m_->d_stamp;
  ga.round_id = (uint32_t)(merge_rounds + 1);
  ga.worklist = m_->d_wworklist;
  ga.wl_seg = c.n_unique + 64;
  ga.work_n = c.d_work_n;
  ga.gm = m_->d_gather->matched;
  ga.done_ctr = &m_->d_gather->ticket;
  ga.xyz = d_xyz;
  ga.k = r.k;
  ga.z_base = r.z_base;
  if (r.by_args)
    for (uint32_t j = 0; j < r.k; j++) ga.cnt[j] = r.rule_counts ? (uint32_t)std::min<unsigned long long>(r.rule_counts[j], 0xffffffffull) : 0xffffffffu;
  if (!m_->d_stamp) {  // (the index could not be built yet: no stamps either -- the gather must not claim words)
    stamp_cap_ = (unsigned int)(c.n_unique + c.n_unique / 8 + 64);
    m_->d_stamp.alloc(stamp_cap_);
    HIP_CHECK(hipMemsetAsync(m_->d_stamp, 0, (size_t)stamp_cap_ * 4, strm()));
    ga.stamp = m_->d_stamp;
  }
  // live tokens per class-A word, about: what the class held when it left the tiles, less a token per merge site since (a round or two behind)
  if (sites_last_ != ~0ull && word_sites_seen_ != sites_cum_) {
    word_live_tokens_ -= std::min(word_live_tokens_, sites_cum_ - std::min(sites_cum_, word_sites_seen_));
    word_sites_seen_ = sites_cum_;
  }
  ga.stats = m_->d_stats;
  const BatchArgs gba = r.first_ba();
  WordsRound wr{};
  wr.ws = WordSet{c.d_tok, m_->d_wmeta, c.d_wcnt, (uint32_t)c.n_unique};
  wr.pt = r.kpt;
  wr.db = db_;
  wr.rules = m_->d_rules;
  wr.rule_mask = r.cap - 1;
  wr.bloom_g = m_->d_bloom;
  wr.self_x = r.self_x;
  wr.self_z = r.self_z;
  wr.drec = m_->d_drec;
  wr.drec_cap = drec_cap_;
  wr.drec_n = m_->d_drec_n;
  wr.irec = m_->d_irec;
  wr.ba = &gba;
  wr.scan = tail_of(r, 0);
  wr.work_hint = sites_last_ != ~0ull && idx_valid_ ? (unsigned int)std::min<unsigned long long>(2 * sites_last_ + word_hint_floor_, 1ull << 30) : 0u;
  wr.inline_max = words_inline_max_;
  wr.ga = &ga;
  wr.fuse_max = words_fuse_max_;
  wr.avg_word_tokens = (unsigned int)std::min<unsigned long long>(std::max<unsigned long long>(1, word_live_tokens_ / std::max<unsigned long long>(1, c.n_unique)), 1u << 16);
  wr.wgather_grid = hook_or_auto(cfg_->wgather_grid);
  wr.words_grid = hook_or_auto(cfg_->words_grid);
  wr.words_wpi = hook_or_auto(cfg_->words_wpi);
  if (launch_words_apply(wr, strm())) word_fused_rounds++;
  word_rounds++;
  if (!idx_valid_) word_all_rounds++;
}

// tuning aids, after the round's launches: cumulative device statistics after every round (YTTM_TRACE_ROUNDS), the measurement pass's snapshot
void GpuCtx::round_trace(const Round &r) {
  const char *trace_rounds = trace_rounds_;
  if (trace_rounds) {
    chain_event_ = nullptr;  // (adds a sync)
    unsigned long long stt[STAT_TAIL];
    launch_fold_stats(m_->d_stats, pt_.n_keys, strm());
    HIP_CHECK(hipMemcpyAsync(stt, m_->d_stats, sizeof stt, hipMemcpyDeviceToHost, strm()));
    sync();
    if (cfg_->trace_blocks.set && merge_rounds % 50 == 0) {  // PROF build: per-workgroup start / end / dirty tiles of this round
      std::vector<unsigned long long> rows(STATS_WORDS);
      HIP_CHECK(hipMemcpy(rows.data(), m_->d_stats, STATS_WORDS * 8, hipMemcpyDeviceToHost));
      std::string name = cfg_->trace_blocks.raw + "." + std::to_string(merge_rounds);
      if (FILE *fb = fopen(name.c_str(), "w")) {
        for (int b = 0; b < BLK_ROWS; b++) {
          const unsigned long long *row = rows.data() + blk_at(b);
          fprintf(fb, "%d %llu %llu %llu\n", b, row[BLK_PROF_T0], row[BLK_PROF_T1], row[BLK_PROF_AUX]);
        }
        fclose(fb);
      }
    }
    FILE *f = fopen(trace_rounds, merge_rounds == 1 ? "w" : "a");
    if (f) {
      fprintf(f, "%llu %u %llu %llu %llu %llu %u", merge_rounds, r.k, stt[STAT_SITES], stt[STAT_TOUCHED], stt[STAT_TOKENS], stt[STAT_TOUCHED_TOKENS], m_->cls[0].n_tiles);
      for (int i = STAT_PROF; i < STAT_PROF + STAT_PROF_N; i++) fprintf(f, " %llu", stt[i]);
      fprintf(f, "\n");
      fclose(f);
    }
  }
  if (instrument && split_round && merge_rounds == split_round) {  // (measurement pass only: a sync does not matter)
    unsigned long long st[8] = {0};
    launch_fold_stats(m_->d_stats, pt_.n_keys, strm());
    HIP_CHECK(hipMemcpyAsync(st, m_->d_stats, sizeof st, hipMemcpyDeviceToHost, strm()));
    sync();
    split_sites = st[STAT_SITES];
    split_touched_words = st[STAT_INSTR_WORDS];
    split_touched_word_tokens = st[STAT_INSTR_TOKENS];
  }
}

// what the round leaves for later: the batch whose pairs are still to be zeroed, the repack schedule, (multi-GPU) the exchange
void GpuCtx::round_finish(const Round &r) {
  {  // the sites this round may add to what the mailbox has reported so far (maybe_repack)
    unsigned long long s3 = 0;
    for (uint32_t j = 0; j < r.k; j++) s3 += r.rule_counts ? r.rule_counts[j] : (~0ull >> 8);
    rp_recent_[2] = rp_recent_[1];
    rp_recent_[1] = rp_recent_[0];
    rp_recent_[0] = std::min<unsigned long long>(s3, ~0ull >> 4);
  }
  pending_zero_ = !r.sa.on || multi();  // (a fused round zeroes its batch's pairs itself; multi-GPU: exchange_round hands the batch to the fold's scan)
  zero_valid_ = true;
  zero_ba_ = r.ba;
  zero_cap_ = r.cap;
  zero_self_key_ = r.self_x != 0xffffffffu ? pair_key(r.self_x, r.self_x) : PT_EMPTY;
  // repack when the tiles are less than half full.  With the hot-list filter the fill is known for free (the previous
  // round's filters report the tokens they streamed); otherwise look every 8 rounds.
  if (hot_state_ == HOT_ACTIVE && live_tokens_last_) {
    const unsigned long long nominal = (unsigned long long)m_->cls[0].n_tiles * m_->cls[0].nom + (unsigned long long)m_->cls[1].n_tiles * m_->cls[1].nom;
    // (word mode: class A no longer lives in tiles, and "tokens streamed last round" is small against the nominal size of everything whatever
    // the fill of class B: its looks are spaced out -- a late repack of the few long words costs less than a look every other round)
    if (live_tokens_last_ * 2 <= nominal && ++rounds_since_check_ >= (word_mode_ ? 64u : 2u)) {
      rounds_since_check_ = 0;
      for (int ci = 0; ci < 2; ci++) maybe_repack(ci);
    }
  } else if (++rounds_since_check_ >= 8) {
    rounds_since_check_ = 0;
    for (int ci = 0; ci < 2; ci++) maybe_repack(ci);
  }
  if (multi()) exchange_round(0, r.sa.on ? &r.sa : nullptr);  // (stream-ordered; the scan in the fold's tail reports blocks that were too small)
}

}  // namespace yttm
