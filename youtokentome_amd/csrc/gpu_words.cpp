// gpu_words.cpp -- word mode (class-A words processed from worklists) and the pair index behind it: set-up and rebuilds; the rounds themselves are GpuCtx::merge_apply.
// (Round 5: cut out of gpu_ctx.cpp, code motion only; gpu_ctx_internal.h says what went where.)
#include "gpu_ctx_internal.h"

namespace yttm {

void GpuCtx::free_words() {
  m_->d_wmeta.reset(); m_->d_gather.reset(); m_->d_xyz.reset(); m_->d_wworklist.reset(); m_->d_drec.reset(); m_->d_drec_n.reset(); m_->d_irec.reset();
  m_->tl = {};
  tl_ = TokLists{};
  word_mode_ = false;
  word_global_ = false;
  sites_last_ = ~0ull;
  g_sites_last_ = ~0ull;
  g_sites_cum_ = g_tokens_cum_ = g_tokens_last_ = g_tiles_a_ = 0;
}

// The switch to word mode (k_words.hip): from here on class-A words live in the slots they have now and a round visits the words
// that hold a merge site.  Called between rounds.
void GpuCtx::enter_word_mode(uint32_t z_next) {
  WordClass &c = m_->cls[0];
  chain_event_ = nullptr;
  m_->d_wmeta.alloc(c.n_unique + 1);
  launch_words_init(c.ts, m_->d_wmeta, strm());
  m_->d_wworklist.alloc(c.n_unique + 64);
  HIP_CHECK(hipMemsetAsync(c.d_work_n, 0, 64, strm()));
  m_->d_gather.alloc(1);
  HIP_CHECK(hipMemsetAsync(m_->d_gather, 0, sizeof(GatherCtl), strm()));
  m_->d_xyz.alloc(3 * (size_t)RULES_CAP);
  drec_cap_ = (unsigned int)cfg_->word_drec.u;  // (tests: a region that overflows)
  m_->d_drec.alloc((size_t)WORDS_MAX_GRID * drec_cap_);
  m_->d_drec_n.alloc(WORDS_MAX_GRID);
  m_->d_irec.alloc((size_t)WORDS_MAX_GRID * drec_cap_);
  auto &t = m_->tl;  // (tl_ is the view of it that the kernels get)
  t.base.alloc(id_cap_);
  t.cap.alloc(id_cap_);
  t.fill.alloc(id_cap_);
  HIP_CHECK(hipMemsetAsync(t.base, 0, (size_t)id_cap_ * 8, strm()));
  HIP_CHECK(hipMemsetAsync(t.cap, 0, (size_t)id_cap_ * 4, strm()));
  HIP_CHECK(hipMemsetAsync(t.fill, 0, (size_t)id_cap_ * 4, strm()));
  t.cursor.alloc(2);
  HIP_CHECK(hipMemsetAsync(t.cursor, 0, 16, strm()));
  // every record ever matched is a site at most once through each of its two neighbours, and a site removes a token: a few records per
  // live token bound the log between two index builds; should it fill up all the same, the round says so and the index is rebuilt
  const unsigned long long live = std::max<unsigned long long>(live_tokens_last_, 1ull << 16);
  const unsigned long long log_env = cfg_->word_log.u;  // (tests: a log that overflows)
  tl_.log_cap = log_env ? log_env : 2 * live + (1ull << 20);
  t.rec_word.alloc(tl_.log_cap);
  t.rec_l.alloc(tl_.log_cap);
  t.rec_r.alloc(tl_.log_cap);
  tl_.base = t.base; tl_.cap = t.cap; tl_.fill = t.fill; tl_.cursor = t.cursor;
  tl_.rec_word = t.rec_word; tl_.rec_l = t.rec_l; tl_.rec_r = t.rec_r;
  tl_.broken = &h_pin_->broken;  // (the kernels write it with system-scope stores)
  *(volatile unsigned int *)tl_.broken = 0;
  word_mode_ = true;
  word_global_ = true;
  word_live_tokens_ = std::min<unsigned long long>(c.n_tokens0, live_tokens_last_ ? live_tokens_last_ : c.n_tokens0);
  word_sites_seen_ = sites_cum_;
  word_switch_round = merge_rounds;
  idx_valid_ = false;
  idx_pending_ = true;
  if (cfg_->trace.set) fprintf(stderr, "[yttm] word mode from round %llu on: %llu words, last round %llu sites, %llu tokens streamed; log %llu records\n", merge_rounds,
                                  c.n_unique, sites_last_, live_tokens_last_, tl_.log_cap);
  build_index(z_next);
}

// (Re)builds the pair index of word mode from the hot list as it is now and the class-A words as they are now (see k_index_core.h PairIndex).
// Called between rounds.
void GpuCtx::build_index(uint32_t z_next) {
  idx_pending_ = false;
  idx_valid_ = false;
  WordClass &c = m_->cls[0];
  if (!c.n_tiles || hot_state_ != HOT_ACTIVE || !word_mode_) return;
  chain_event_ = nullptr;
  unsigned int listed = 0;  // (the list has grown since the scan that last reported its length)
  HIP_CHECK(hipMemcpyAsync(&listed, &m_->d_hot_ctl->n, 4, hipMemcpyDeviceToHost, strm()));
  sync();
  if (listed > hot_cap_) return;  // overflowed: the next scan rebuilds the list, and the index after it
  unsigned long long want = 1024;
  while (want < 2ull * ((unsigned long long)listed + 256)) want <<= 1;
  if (want > idx_cap_) {
    m_->idx.key.reset();  // (all three back in the pool before any is taken again: the order decides which blocks are reused)
    m_->idx.cnt.reset();
    m_->idx.off.reset();
    m_->idx.key.alloc(want);
    m_->idx.cnt.alloc(want * IDX_SHARDS + 1);
    m_->idx.off.alloc(want * IDX_SHARDS + 2);
    m_->idx_scan_tmp.alloc(scan_scratch_blocks(want * IDX_SHARDS + 1));
    idx_cap_ = want;
  }
  if (!m_->idx.bloom) m_->idx.bloom.alloc(ENC_BLOOM_WORDS);
  idx_.key = m_->idx.key;
  idx_.cnt = m_->idx.cnt;
  idx_.off = m_->idx.off;
  idx_.bloom = m_->idx.bloom;
  idx_.mask = (unsigned int)(want - 1);
  launch_fill_u64(idx_.key, PT_EMPTY, want, strm());
  HIP_CHECK(hipMemsetAsync(idx_.cnt, 0, want * IDX_SHARDS * 4, strm()));
  HIP_CHECK(hipMemsetAsync(idx_.bloom, 0, ENC_BLOOM_WORDS * 4, strm()));
  // The radix build (k_index.hip) wants 4 B per class-A token slot for the resolved adjacencies and, once the postings are counted, 8 B per
  // posting for their records: it runs from idx_radix_min_ live tokens on and when all of that -- sized for a posting per token slot -- fits what
  // is free with room to spare (as the radix K3 decides, gpu_pairs.cpp); else the streaming build.
  const unsigned long long slots_n = (unsigned long long)c.n_tiles * c.slot;
  const bool radix = word_live_tokens_ >= idx_radix_min_ && idx_radix_takes(idx_.mask, c.n_tiles) &&
                     12ull * slots_n + 4ull * idx_radix_scratch_u32() + (64ull << 20) <= free_device_bytes() / 4 * 3;
  PoolBuf<uint32_t> rx_scratch, rx_slots;
  PoolBuf<unsigned long long> rx_rec;
  t_begin(KT_CAND);
  launch_idx_seed(pt_, idx_, listed, strm());
  unsigned long long total = 0;
  if (radix) {
    rx_scratch.alloc(idx_radix_scratch_u32());
    rx_slots.alloc(slots_n);
    HIP_CHECK(hipMemsetAsync(rx_scratch, 0, idx_radix_scratch_head_bytes(), strm()));
    launch_idx_radix_sweep(c.ts, idx_, rx_scratch, rx_slots, strm());
    HIP_CHECK(hipMemcpyAsync(&total, rx_scratch, 8, hipMemcpyDeviceToHost, strm()));
  } else {
    if (!m_->idx_save) m_->idx_save.alloc(idx_save_bytes());
    launch_idx_stream(false, c.ts, idx_, strm(), true, m_->idx_save);
    // offsets = exclusive scan of the counts (one extra zero count behind the last slot: off[mask + 1] = the total)
    HIP_CHECK(hipMemsetAsync(idx_.cnt + want * IDX_SHARDS, 0, 4, strm()));
    launch_exclusive_scan(idx_.cnt, want * IDX_SHARDS + 1, idx_.off, m_->idx_scan_tmp, &m_->ctr->index_scan_total, strm());
    HIP_CHECK(hipMemsetAsync(idx_.cnt, 0, want * IDX_SHARDS * 4, strm()));  // the fill pass's cursors
    HIP_CHECK(hipMemcpyAsync(&total, &m_->ctr->index_scan_total, 8, hipMemcpyDeviceToHost, strm()));
  }
  sync();
  index_builds++;
  if (cfg_->trace.set) fprintf(stderr, "[yttm] index build at round %llu: %u listed pairs, %llu postings, %u tiles, last round touched %llu tiles%s\n", merge_rounds, listed, total, c.n_tiles, touched_last_, radix ? " (radix)" : "");
  if (total == 0 || total > 0xfffffff0ull) {  // (no postings, or more than the 32-bit run offsets hold: the rounds take every word)
    t_end(KT_CAND, 4ull * c.n_tiles * c.nom);
    return;
  }
  if (total > post_cap_) {
    post_cap_ = total + total / 4 + 1024;
    m_->idx.post.alloc(post_cap_);
    idx_.post = m_->idx.post;
  }
  if (radix) {
    rx_rec.alloc(total);
    launch_idx_radix_scatter(c.ts, idx_, rx_scratch, rx_slots, rx_rec, total, strm());
    // (all of a key's postings are counted in its shard 0: the run bounds off[s * IDX_SHARDS] come out of the same scan)
    HIP_CHECK(hipMemsetAsync(idx_.cnt + want * IDX_SHARDS, 0, 4, strm()));
    launch_exclusive_scan(idx_.cnt, want * IDX_SHARDS + 1, idx_.off, m_->idx_scan_tmp, &m_->ctr->index_scan_total, strm());
    HIP_CHECK(hipMemsetAsync(idx_.cnt, 0, want * IDX_SHARDS * 4, strm()));  // the place pass's cursors
    launch_idx_radix_place(idx_, rx_scratch, rx_rec, total, strm());
    index_radix_builds++;
  } else {
    launch_idx_stream(true, c.ts, idx_, strm(), /*agg=*/total > idx_agg_min_, m_->idx_save);
  }
  t_end(KT_CAND, 8ull * c.n_tiles * c.nom);
  const unsigned long long stamps = c.n_unique;  // (a posting is a word, and a round claims words)
  if (stamps > stamp_cap_) {
    stamp_cap_ = (unsigned int)(stamps + stamps / 8 + 64);
    m_->d_stamp.alloc(stamp_cap_);
  }
  HIP_CHECK(hipMemsetAsync(m_->d_stamp, 0, (size_t)stamp_cap_ * 4, strm()));
  {  // every token that exists now is covered by the postings: the instance lists start over
    HIP_CHECK(hipMemsetAsync(tl_.cursor, 0, 16, strm()));
    sync();
    *(volatile unsigned int *)tl_.broken = 0;
  }
  idx_valid_ = true;
  idx_zbuild_ = z_next;
}

void GpuCtx::download_index(std::vector<unsigned long long> &keys, std::vector<unsigned long long> &lo, std::vector<unsigned long long> &hi, std::vector<uint32_t> &post) {
  if (fused_pending_) throw GpuError{"download_index: a candidate scan rides in the last merge round -- call candidates first"};
  keys.clear(); lo.clear(); hi.clear(); post.clear();
  if (!idx_valid_) return;
  const size_t slots = (size_t)idx_.mask + 1;
  std::vector<unsigned long long> k(slots), off(slots * IDX_SHARDS + 1);
  HIP_CHECK(hipMemcpyAsync(k.data(), idx_.key, slots * 8, hipMemcpyDeviceToHost, strm()));
  HIP_CHECK(hipMemcpyAsync(off.data(), idx_.off, off.size() * 8, hipMemcpyDeviceToHost, strm()));
  sync();
  post.resize(off.back());
  if (!post.empty()) HIP_CHECK(hipMemcpyAsync(post.data(), idx_.post, post.size() * 4, hipMemcpyDeviceToHost, strm()));
  sync();
  for (size_t s = 0; s < slots; s++) {
    if (k[s] == PT_EMPTY) continue;
    keys.push_back(k[s]);
    lo.push_back(off[s * IDX_SHARDS]);
    hi.push_back(off[(s + 1) * IDX_SHARDS]);
  }
}

}  // namespace yttm
