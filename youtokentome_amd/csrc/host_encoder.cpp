// host_encoder.cpp -- BaseEncoder (bpe.h:22-82): model load, HBM-resident rule tables, batch encode through K5,
// and the tiny host-side helpers of the drop-in surface (id<->subword, decode, vocabulary).
#include <cstdlib>
#include <cstdio>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <thread>
#include <sys/mman.h>
#include <chrono>
#include <random>

#include "enc_lanes.h"
// tests/hipsim/Makefile compiles host_decode.cpp and host_lines.cpp itself and says so with -DYTTM_ENCODER_UNITS.  An emulator makefile
// without the flag, as the one of the commit before the split, lists this file alone and gets the other two through it.  hipcc never does.
#if !defined(__HIP__) && !defined(YTTM_ENCODER_UNITS)
#include "host_decode.cpp"
#include "host_lines.cpp"
#endif

namespace yttm {

static const std::string UNK_TOKEN = "<UNK>", PAD_TOKEN = "<PAD>", BOS_TOKEN = "<BOS>", EOS_TOKEN = "<EOS>";  // bpe.h:12-15

BaseEncoder::BaseEncoder(const std::string &model_path, int _n_threads, Status *ret_status, int device) : n_threads(_n_threads), device_(device) {
  Status status = bpe_state.load(model_path);  // bpe.cpp:1643-1656
  if (!status.ok()) { *ret_status = status; return; }
  fill_from_state();
  *ret_status = on_device(device_, [&]() -> Status {
    dev_ = new EncoderDevice();
    for (EncodeLane &l : dev_->lane) l.init();
    cfg_refresh();  // the environment hooks are read here, once per encoder (yttm_config.h) ...
    const std::shared_ptr<const Config> C = cfg();
    dev_->cfg = C;  // ... and kept: the entry points below bind this snapshot, not whatever a later refresh made the process-wide one
    if (C->encode_cache.set) dev_->cache_mode = C->encode_cache.i ? 1 : 0;
    if (C->encode_cache_min_mb.set) dev_->cache_min_bytes = C->encode_cache_min_mb.u << 20;
    if (C->dropout_seed.set) {
      dev_->seed_salt = C->dropout_seed.u;
    } else {
      std::random_device rd;
      dev_->seed_salt = ((unsigned long long)rd() << 32) ^ (unsigned long long)rd();
    }
    // code point -> final id / CP_SPACE / CP_UNK.  is_space wins over char2id (words are split first, bpe.cpp:1509-1510).
    std::vector<uint32_t> cpmap(N_CODEPOINTS, CP_UNK);
    for (auto &c : bpe_state.char2id)
      if (c.first < N_CODEPOINTS) cpmap[c.first] = c.second;
    for (uint32_t s : {9u, 10u, 11u, 12u, 13u, 32u, 9601u}) cpmap[s] = CP_SPACE;
    dev_->cpmap.alloc(N_CODEPOINTS);
    HIP_CHECK(hipMemcpy(dev_->cpmap, cpmap.data(), (size_t)N_CODEPOINTS * 4, hipMemcpyHostToDevice));
    {  // working tokens of the encode kernel keep two flag bits: ids must stay below 2^30 - 16
      uint32_t max_id = 0;
      for (auto &c : char2id) max_id = std::max(max_id, c.second);
      for (auto &r : bpe_state.rules) max_id = std::max(max_id, std::max(r.z, std::max(r.x, r.y)));
      if (max_id >= 0x3ffffff0u) return Status(1, "token ids of 2^30 and above are not supported by the MI355X encoder");
    }
    // rule hash: (x,y) -> rule index; later rules overwrite earlier duplicates like rule2id (bpe.cpp:1672-1674)
    const size_t nr = bpe_state.rules.size();
    unsigned int cap = 64;
    while (cap < 4 * nr + 2) cap <<= 1;  // load factor <= 1/4: nine lookups in ten end at the first slot
    std::vector<RuleSlot> slots(cap);
    for (auto &s : slots) { s.key = PT_EMPTY; s.z = 0; s.pad = 0; }
    std::vector<uint32_t> rz(nr ? nr : 1, 0);
    std::vector<unsigned long long> rxy(nr ? nr : 1, 0);
    for (size_t i = 0; i < nr; i++) {
      const BPE_Rule &r = bpe_state.rules[i];
      rz[i] = r.z;
      rxy[i] = pair_key(r.x, r.y);
      const unsigned long long key = pair_key(r.x, r.y);
      unsigned int h = enc_hash(r.x, r.y) & (cap - 1);
      while (slots[h].key != PT_EMPTY && slots[h].key != key) h = (h + 1) & (cap - 1);
      slots[h].key = key;
      slots[h].z = r.z;
      slots[h].pad = (uint32_t)i;
    }
    dev_->rules.alloc(cap);
    HIP_CHECK(hipMemcpy(dev_->rules, slots.data(), (size_t)cap * sizeof(RuleSlot), hipMemcpyHostToDevice));
    dev_->rule_z.alloc(rz.size());
    HIP_CHECK(hipMemcpy(dev_->rule_z, rz.data(), rz.size() * 4, hipMemcpyHostToDevice));
    dev_->rule_xy.alloc(rxy.size());
    HIP_CHECK(hipMemcpy(dev_->rule_xy, rxy.data(), rxy.size() * 8, hipMemcpyHostToDevice));
    std::vector<uint32_t> bloom(ENC_BLOOM_WORDS, 0);
    for (size_t i = 0; i < nr; i++) {
      const uint32_t h = enc_hash(bpe_state.rules[i].x, bpe_state.rules[i].y);
      bloom[enc_bloom_word(h)] |= enc_bloom_bits(h);
    }
    dev_->bloom.alloc(ENC_BLOOM_WORDS);
    HIP_CHECK(hipMemcpy(dev_->bloom, bloom.data(), (size_t)ENC_BLOOM_WORDS * 4, hipMemcpyHostToDevice));
    EncModel &m = dev_->m;
    m.bloom = dev_->bloom;
    m.cpmap = dev_->cpmap;
    m.rules = dev_->rules;
    m.rule_z = dev_->rule_z;
    m.rule_xy = dev_->rule_xy;
    m.rule_mask = cap - 1;
    m.n_rules = (uint32_t)nr;
    {  // merged tokens are numbered in rule order with the special ids skipped (bpe.cpp:814-837): z(r) without a load
      m.z_affine = nr > 0;
      m.z_base = nr ? rz[0] : 0;
      for (uint32_t &b : m.z_bp) b = 0xffffffffu;
      int nbp = 0;
      for (size_t i = 1; i < nr && m.z_affine; i++) {
        const long long step = (long long)rz[i] - (long long)rz[i - 1] - 1;
        if (step < 0 || nbp + step > 4) m.z_affine = 0;
        else for (long long k = 0; k < step; k++) m.z_bp[nbp++] = (uint32_t)i;
      }
    }
    auto it = char2id.find(SPACE_TOKEN);
    m.space_id = it == char2id.end() ? 0u : it->second;
    m.unk_id = bpe_state.special_tokens.unk_id;
    m.bos_id = bpe_state.special_tokens.bos_id;
    m.eos_id = bpe_state.special_tokens.eos_id;
    return Status();
  });
  if (ret_status->ok() && n_threads == -1) n_threads = 1;  // accepted for API compatibility; encode runs on the GPU
}

BaseEncoder::~BaseEncoder() {
  if (dev_) {
    (void)hipSetDevice(device_);
    delete dev_;
  }
}

void BaseEncoder::fill_from_state() {  // bpe.cpp:1667-1690
  for (auto &x : bpe_state.char2id) { char2id[x.first] = x.second; id2char[x.second] = x.first; }
  for (auto &x : id2char) recipe[x.first] = {x.first};
  for (auto &r : bpe_state.rules) {
    std::vector<uint32_t> v = recipe[r.x];
    const std::vector<uint32_t> &w = recipe[r.y];
    v.insert(v.end(), w.begin(), w.end());
    recipe[r.z] = std::move(v);
  }
  for (auto &kv : recipe) {
    std::vector<uint32_t> cps;
    for (uint32_t id : kv.second) cps.push_back(id2char.at(id));
    reversed_recipe[encode_utf8(cps)] = kv.first;
  }
  reversed_recipe[BOS_TOKEN] = (uint32_t)bpe_state.special_tokens.bos_id;
  reversed_recipe[EOS_TOKEN] = (uint32_t)bpe_state.special_tokens.eos_id;
}

int BaseEncoder::vocab_size() const {
  return (int)(bpe_state.rules.size() + bpe_state.char2id.size() + bpe_state.special_tokens.n_special_tokens());
}

// One K5 launch over n_items items of the text (sentences back to back, or the word cache's distinct words [offsets[j], ends[j])):
// ids into the lane's scratch, counts into `counts`.
static void k5_pass(EncoderDevice &D, EncodeLane &d, const void *d_bytes, const unsigned long long *d_offsets, const unsigned long long *d_ends,
                    unsigned long long n_items, unsigned long long total_bytes, unsigned long long max_item_bytes, bool bos, bool eos, bool reverse,
                    double dropout_prob, uint32_t *counts, const WordPublish *pub = nullptr) {
  d.k5.scratch.grow((size_t)(2 * total_bytes + 2 * n_items + 2));
  unsigned int max_blocks = 256 * 2;  // 2 workgroups per CU (80 KB LDS each)
  const unsigned long long tok_cap = std::max<unsigned long long>(ENC_LDS_TOKENS, 2 * max_item_bytes + 2);  // tokens per item
  unsigned long long stride = 0, drop_stride = 0;
  {
    // per-wave HBM scratch: 3 working arrays for items that do not fit LDS, + (dropout) word starts and event queues
    unsigned long long per_wave = 0;
    if (tok_cap > (unsigned long long)ENC_LDS_TOKENS) per_wave += 3 * tok_cap * 4;
    if (dropout_prob > 0) per_wave += 7 * tok_cap * 4;
    if (per_wave) {
      unsigned long long waves = std::max<unsigned long long>(1, (4ull << 30) / per_wave);
      max_blocks = (unsigned int)std::max<unsigned long long>(1, std::min<unsigned long long>(max_blocks, waves / ENC_WAVES_PER_BLOCK));
    }
  }
  unsigned long long nb = (n_items + ENC_WAVES_PER_BLOCK - 1) / ENC_WAVES_PER_BLOCK;
  const unsigned int n_blocks = (unsigned int)std::min<unsigned long long>(nb, max_blocks);
  if (tok_cap > (unsigned long long)ENC_LDS_TOKENS) {
    stride = tok_cap;
    d.k5.work.grow((size_t)(3 * stride * (unsigned long long)(n_blocks + 1) * ENC_WAVES_PER_BLOCK));  // (+ 1: k5_words rounds its waves up to 16)
  }
  if (dropout_prob > 0) {
    drop_stride = tok_cap;
    d.k5.drop.grow((size_t)(7 * drop_stride * (unsigned long long)n_blocks * ENC_WAVES_PER_BLOCK));
  }
  const unsigned long long seed = mix64(D.seed_salt + 0x5bd1e995ull * (D.dropout_calls.fetch_add(1) + 1));
  launch_encode(D.m, (const uint8_t *)d_bytes, d_offsets, d_ends, n_items, bos, eos, reverse, d.k5.scratch, counts, d.k5.work, stride, n_blocks,
                dropout_prob, seed, d.k5.drop, drop_stride, d.st, pub);
}

unsigned long long scan_counts(EncodeLane &d, const uint32_t *counts, unsigned long long n, unsigned long long *off) {
  d.k5.scan_tmp.grow((size_t)scan_scratch_blocks(n));
  launch_exclusive_scan(counts, n, off, d.k5.scan_tmp, d.k5.total, d.st);
  unsigned long long total = 0;
  HIP_CHECK(hipMemcpyAsync(off + n, d.k5.total, 8, hipMemcpyDeviceToDevice, d.st));  // (device to device: no host source that must outlive the call)
  HIP_CHECK(hipMemcpyAsync(&total, d.k5.total, 8, hipMemcpyDeviceToHost, d.st));
  HIP_CHECK(hipStreamSynchronize(d.st));
  return total;
}

// N4, the word cache (k_wcache.hip): distinct words of the batch -> K5 -> the sentences' ids by lookup.  Leaves ids + offsets in the
// lane's buffers like the direct path.
static void encode_cached(EncoderDevice &D, EncodeLane &d, const void *d_bytes, const unsigned long long *d_offsets, unsigned long long n_sent,
                          unsigned long long total_bytes, unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse,
                          unsigned long long *n_ids_out) {
  const uint8_t *text = (const uint8_t *)d_bytes;
  unsigned long long cap = 1024;
  // a slot per 16 bytes of text or more: text has far fewer distinct words (1e7 random 'abcd ' sentences: one per 64 bytes), and the passes
  // over the table -- clearing it, listing its words -- cost by its size; a batch that does fill it is inserted again into twice the slots
  while (cap < total_bytes / 16 && cap < (1ull << 31)) cap <<= 1;
  WordCache wc{};
  unsigned long long n_table = 0;
  unsigned int misc[2] = {0, 0};
  unsigned long long short_cap = 1ull << 20;  // slots the words of up to 7 bytes start in (k_wcache.hip wc_insert_word): 8 MB of keys
  if (cfg()->wc_short_slots.set) {  // (measurements, tests) -- rounded up to a power of two: the region's size is used as a mask
    const unsigned long long want = std::max<unsigned long long>(16, cfg()->wc_short_slots.u);
    short_cap = 16;
    while (short_cap < want && short_cap < (1ull << 40)) short_cap <<= 1;
  }
  for (;;) {
    d.wc.slot.grow((size_t)cap);
    d.wc.pos.grow((size_t)cap);
    d.wc.occ.grow((size_t)((total_bytes + n_sent) / 2 + 2));
    const unsigned long long extra_cap = total_bytes / 65536 + 2;
    d.wc.extra.grow((size_t)(2 * extra_cap));
    wc.slot = d.wc.slot;
    wc.pos = d.wc.pos;
    wc.mask = cap - 1;
    wc.short_mask = std::min(cap, short_cap) - 1;
    wc.occ = d.wc.occ;
    wc.extra = d.wc.extra;
    wc.extra_n = d.wc.misc;
    wc.extra_cap = (unsigned int)extra_cap;
    wc.status = d.wc.misc + 1;
    launch_fill_u64(wc.slot, PT_EMPTY, cap, d.st);
    HIP_CHECK(hipMemsetAsync(wc.occ, 0xff, (size_t)((total_bytes + n_sent) / 2 + 2) * 4, d.st));  // (no word starts anywhere yet)
    HIP_CHECK(hipMemsetAsync(d.wc.misc, 0, 8, d.st));
    launch_wcache_insert(D.m, text, total_bytes, d_offsets, n_sent, wc, d.st);
    const unsigned long long n_blk = wcache_count_blocks(wc);
    d.wc.blk.grow((size_t)n_blk);
    d.wc.blk_off.grow((size_t)n_blk + 1);
    launch_wcache_count_slots(wc, d.wc.blk, d.st);
    HIP_CHECK(hipMemcpyAsync(misc, d.wc.misc, 8, hipMemcpyDeviceToHost, d.st));
    n_table = scan_counts(d, d.wc.blk, n_blk, d.wc.blk_off);  // (syncs)
    if (!(misc[1] & 1u)) break;
    // too full for the probe limit: start over -- with the short words spread wider if it WAS one of them that found no slot (the kernel
    // says so: status bit 1), else with twice the slots at once (a batch of mostly distinct LONG words, the usual cause of a full
    // table, paid up to three insert passes over gigabytes of text for a region that was not the problem)
    if ((misc[1] & 2u) && short_cap < cap) {
      short_cap = std::min(cap, short_cap << 3);
      continue;
    }
    if (cap >= (1ull << 31)) throw GpuError{"encode: the word table does not fit"};
    cap <<= 1;
    short_cap = cap;
  }
  const unsigned long long n_extra = misc[0], n_words = n_table + n_extra;
  d.wc.distinct_words = n_words;
  D.last_distinct_words.store(n_words);
  d.wc.ustart.grow((size_t)n_words + 1);
  d.wc.uend.grow((size_t)n_words + 1);
  d.wc.uslot.grow((size_t)n_table + 1);
  d.wc.ucounts.grow((size_t)n_words + 1);
  launch_wcache_list(wc, d.wc.blk_off, n_table, d.wc.ustart, d.wc.uend, d.wc.uslot, d.st);
  if (n_words) {  // (the distinct words' ids stay where K5 puts them, in the lane's scratch: the sentences are assembled from there)
    // (k5_words leaves in every word's table slot where its ids are and how many)
    const WordPublish pub{wc.slot, d.wc.uslot, n_table, wc.extra, total_bytes};
    k5_pass(D, d, d_bytes, d.wc.ustart, d.wc.uend, n_words, total_bytes, max_sentence_bytes, false, false, false, 0.0, d.wc.ucounts, &pub);
  }
  launch_wcache_count(d_offsets, n_sent, wc, (bos ? 1 : 0) + (eos ? 1 : 0), d.k5.counts, d.st);
  const unsigned long long total = scan_counts(d, d.k5.counts, n_sent, d.res.off);
  d.res.ids.grow((size_t)total + 1);
  launch_wcache_scatter(D.m, d_offsets, n_sent, wc, d.k5.scratch, bos, eos, reverse, d.res.off, d.res.ids, d.st);
  HIP_CHECK(hipStreamSynchronize(d.st));
  d.res.n_ids = total;
  if (n_ids_out) *n_ids_out = total;
}

Status check_bos_eos(const BaseEncoder &enc, bool bos, bool eos) {
  if (bos && enc.bpe_state.special_tokens.bos_id == -1) return Status(1, "Can't add <BOS> token. Model was trained without it.");
  if (eos && enc.bpe_state.special_tokens.eos_id == -1) return Status(1, "Can't add <EOS> token. Model was trained without it.");
  return Status();
}

// ---- the restricted vocabulary (k_restrict.h; the rule is in include/yttm_mi355x.h) ---------------------------------------------------------
Status restrict_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                        unsigned long long n_ids, bool reverse, bool pending, unsigned long long *n_out, double *kernel_ms) {
  return on_device(device, [&]() -> Status {
    if (kernel_ms) *kernel_ms = 0;
    if (n_out) *n_out = 0;
    unsigned long long total = 0;
    bool skip = false;
    if (n_sent) {
      const RestrictTable tb{D.voc.exp_off, reverse ? D.voc.exp_rev : D.voc.exp_fwd, D.voc.vocab};
      const Status s = two_pass_on_lane(
          d, n_sent, d.rs.len, d.rs.off, kernel_ms, &total,
          [&](bool write) {
            if (write && skip) return;
            launch_restrict(write, ids, off, n_sent, n_ids, tb, d.rs.len, d.rs.off, d.rs.ids, d.st);
          },
          [] { return Status(); },
          [&](unsigned long long need) {
            skip = pending && need == n_ids;  // (every expansion has an id, and one of a single id is that id: nothing splits)
            if (skip) return;
            d.rs.ids.grow((size_t)need + 4);
            if (((uintptr_t)d.rs.ids.p & 15u) != 0) throw GpuError{"restrict: the output is not 16-byte aligned"};
          });
      if (!s.ok()) return s;
      if (!skip) {
        std::swap(d.res.ids, d.rs.ids);
        std::swap(d.res.off, d.rs.off);
      }
    }
    if (!pending) {
      d.res.n_sent = n_sent;
      d.res.made = true;
      d.sp.valid = false;  // (spans belong to the ids they were made from)
    }
    d.res.n_ids = total;
    if (n_out) *n_out = total;
    D.voc.stats[0] += 1;
    if (total == n_ids) D.voc.stats[1] += 1;
    D.voc.stats[2] += n_ids;
    D.voc.stats[3] += total;
    return Status();
  });
}

// The tail of encode_on_lane: with a vocabulary set, the pass over the ids the encode has just left on the lane.
static Status restrict_tail(EncoderDevice &D, EncodeLane &d, int device, bool reverse, unsigned long long *n_ids_out, double *kernel_ms) {
  if (!D.voc.set) return Status();
  double ms = 0;
  unsigned long long n = 0;
  const Status s = restrict_on_lane(D, d, device, d.res.ids, d.res.off, d.res.n_sent, d.res.n_ids, reverse, true, &n, kernel_ms ? &ms : nullptr);
  if (!s.ok()) return s;
  if (n_ids_out) *n_ids_out = n;
  if (kernel_ms) *kernel_ms += ms;
  return Status();
}

// ---- the byte fallback (k_bytefb.h; the rule is in include/yttm_mi355x.h) -----------------------------------------------------------------
// measure -> scan -> write into the lane's second pair of buffers (rs, the restriction's: the two passes run one after the other), which then
// becomes the lane's encode result.  pending: the input IS that result; where the measure pass met no unk_id the write pass is skipped and the
// result stays where it is.  Otherwise the input is the caller's and the result is installed as after an encode of n_sent sentences.
static Status bytefb_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off,
                             const void *d_text, const void *d_soff, unsigned long long n_sent, unsigned long long n_ids, bool reverse, bool pending,
                             unsigned long long *n_out, double *kernel_ms) {
  return on_device(device, [&]() -> Status {
    if (kernel_ms) *kernel_ms = 0;
    if (n_out) *n_out = 0;
    unsigned long long total = 0;
    bool skip = false;
    if (n_sent) {
      const SubInput in{(const uint8_t *)d_text, (const unsigned long long *)d_soff, ids, off, n_sent, (int32_t)enc.bpe_state.special_tokens.unk_id, reverse ? 1 : 0};
      const int32_t first = (int32_t)enc.vocab_size();
      uint32_t saw = 0;
      const Status s = two_pass_on_lane(
          d, n_sent, d.rs.len, d.rs.off, kernel_ms, &total,
          [&](bool write) {
            if (write && skip) return;
            if (!write) HIP_CHECK(hipMemsetAsync(d.fb.saw, 0, 4, d.st));
            launch_bytefb(write, D.m, in, first, n_ids, d.rs.len, d.fb.saw, d.rs.off, d.rs.ids, d.st);
            if (!write) HIP_CHECK(hipMemcpyAsync(&saw, d.fb.saw, 4, hipMemcpyDeviceToHost, d.st));  // (here once the scan has synchronised)
          },
          [] { return Status(); },
          [&](unsigned long long need) {
            skip = pending && !saw;  // (NOT need == n_ids: a run of one ASCII char keeps the total and changes the id)
            if (skip) return;
            d.rs.ids.grow((size_t)need + 4);
            if (((uintptr_t)d.rs.ids.p & 15u) != 0) throw GpuError{"byte fallback: the output is not 16-byte aligned"};
          });
      if (!s.ok()) return s;
      if (!skip) {
        std::swap(d.res.ids, d.rs.ids);
        std::swap(d.res.off, d.rs.off);
      }
    }
    if (!pending) {
      d.res.n_sent = n_sent;
      d.res.made = true;
    }
    d.sp.valid = false;  // (spans belong to the ids they were made from)
    d.res.n_ids = total;
    if (n_out) *n_out = total;
    D.bfb.stats[0] += 1;
    if (skip) D.bfb.stats[1] += 1;
    D.bfb.stats[2] += n_ids;
    D.bfb.stats[3] += total;
    return Status();
  });
}

// The tail of encode_on_lane, behind the restriction's: with the setting on, the pass over the ids the encode has just left on the lane.  (The two
// commute -- byte ids lie outside [0, V) and pass through E, unk_id is a leaf --, and the restriction first walks the shorter array.)
static Status bytefb_tail(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, const void *d_soff, bool reverse,
                          unsigned long long *n_ids_out, double *kernel_ms) {
  if (!D.bfb.on.load()) return Status();
  double ms = 0;
  unsigned long long n = 0;
  const Status s = bytefb_on_lane(enc, D, d, device, d.res.ids, d.res.off, d_text, d_soff, d.res.n_sent, d.res.n_ids, reverse, true, &n, kernel_ms ? &ms : nullptr);
  if (!s.ok()) return s;
  if (n_ids_out) *n_ids_out = n;
  if (kernel_ms) *kernel_ms += ms;
  return Status();
}

Status BaseEncoder::set_byte_fallback(bool on) const {
  if (!dev_) return Status(2, "encoder has no device state");
  if ((unsigned long long)vocab_size() > BFB_VOCAB_MAX) return Status(1, "set_byte_fallback: the vocabulary leaves no room for 256 byte ids");
  EncoderDevice &D = *dev_;
  std::lock_guard<std::mutex> lk0(D.lane[0].mu), lk1(D.lane[1].mu);  // (always in this order; a result already pending stays as it is)
  D.bfb.on.store(on);
  if (D.add.n.load()) {  // (under added tokens the decode table marks [V, V + 256) invalid while the byte fallback is off: it is made again)
    std::lock_guard<std::mutex> lkd(D.dec_mu);
    D.dec_ready = D.sub_ready = false;
  }
  return Status();
}
bool BaseEncoder::byte_fallback() const { return dev_ && dev_->bfb.on.load(); }
void BaseEncoder::byte_fallback_stats(unsigned long long out[4]) const {
  for (int i = 0; i < 4; i++) out[i] = dev_ ? dev_->bfb.stats[i].load() : 0ull;
}

Status BaseEncoder::byte_fallback_ids_device(const void *d_ids, const void *d_id_offsets, const void *d_bytes, const void *d_text_offsets,
                                             unsigned long long n_sent, unsigned long long n_ids, unsigned long long total_bytes, bool reverse,
                                             unsigned long long *n_out, double *kernel_ms) const {
  if (n_out) *n_out = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && (!d_id_offsets || !d_text_offsets)) return Status(2, "byte_fallback_ids_device: no offsets");
  if (n_ids && !d_ids) return Status(2, "byte_fallback_ids_device: no ids");
  if (total_bytes && !d_bytes) return Status(2, "byte_fallback_ids_device: no text");
  if (((uintptr_t)d_ids & 3u) != 0) return Status(2, "byte_fallback_ids_device: the ids must be 4-byte aligned");
  const Lane0 l(*dev_);
  if (!dev_->bfb.on.load()) return Status(1, "byte_fallback_ids_device: byte fallback is not set");  // (before any work: what was pending stays)
  return bytefb_on_lane(*this, *dev_, l.d, device_, (const int32_t *)d_ids, (const unsigned long long *)d_id_offsets, d_bytes, d_text_offsets, n_sent, n_ids,
                        reverse, false, n_out, ms.next());
}

// ---- the added tokens (k_added.h; the rule is in include/yttm_mi355x.h) ---------------------------------------------------------------------
// The split on a lane's stream (which ends synchronised): measure -> scan -> write into cnt / first / off / tok (the lane's, or the encoder's
// slot).  no_write_without_match: where the text holds no match the write pass is skipped (the refined batch is the batch) and off / tok stay as
// they were.  *n_sub: the sub-sentences, n_sent + 2 * matches.
static Status split_on_lane(EncoderDevice &D, EncodeLane &d, const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                            bool no_write_without_match, DevBuf<uint32_t> &cnt, DevBuf<unsigned long long> &first, DevBuf<unsigned long long> &off,
                            DevBuf<int32_t> &tok, unsigned long long *n_sub, double *kernel_ms) {
  const AddedTable tb = D.add.table();
  bool skip = false;
  return two_pass_on_lane(
      d, n_sent, cnt, first, kernel_ms, n_sub,
      [&](bool write) {
        if (write && skip) return;
        launch_added_split(write, (const uint8_t *)d_bytes, (const unsigned long long *)d_offsets, n_sent, total_bytes, tb, cnt, first, off, tok, d.st);
      },
      [] { return Status(); },
      [&](unsigned long long need) {
        skip = no_write_without_match && need == n_sent;  // (2 * matches + 1 sub-sentences per sentence: no match anywhere)
        if (skip) return;
        off.grow((size_t)need + 1);
        tok.grow((size_t)need);
      });
}

// The join of the refined batch's ids pending on the lane (forward, without bos / eos) into the lane's second pair of buffers, which then becomes
// the lane's encode result of the caller's n_sent sentences.
static Status join_on_lane(const BaseEncoder &enc, EncodeLane &d, unsigned long long n_sent, bool bos, bool eos, bool reverse, unsigned long long *n_out,
                           double *kernel_ms) {
  const SpecialTokens &sp = enc.bpe_state.special_tokens;
  const AddedJoin in{d.res.ids, d.res.off, d.ad.tok, d.ad.first, n_sent, (int32_t)added_first((uint32_t)enc.vocab_size()), (int32_t)sp.bos_id, (int32_t)sp.eos_id,
                     bos ? 1 : 0, eos ? 1 : 0, reverse ? 1 : 0};
  unsigned long long total = 0;
  const Status s = two_pass_on_lane(
      d, n_sent, d.rs.len, d.rs.off, kernel_ms, &total,
      [&](bool write) { launch_added_join(write, in, d.res.n_ids, d.rs.len, d.rs.off, d.rs.ids, d.st); }, [] { return Status(); },
      [&](unsigned long long need) {
        d.rs.ids.grow((size_t)need + 4);
        if (((uintptr_t)d.rs.ids.p & 15u) != 0) throw GpuError{"added tokens: the output is not 16-byte aligned"};
      });
  if (!s.ok()) return s;
  std::swap(d.res.ids, d.rs.ids);
  std::swap(d.res.off, d.rs.off);
  d.res.n_sent = n_sent;
  d.res.n_ids = total;
  *n_out = total;
  return Status();
}

Status BaseEncoder::set_added_tokens(const uint8_t *blob, const unsigned long long *tok_offsets, unsigned long long n) const {
  if (!dev_) return Status(2, "encoder has no device state");
  EncoderDevice &D = *dev_;
  const CfgBind bind(D.cfg);
  if (blob) {  // (before any lock: an invalid set leaves the setting as it was)
    if (!tok_offsets) return Status(1, "set_added_tokens: no offsets");
    const std::string bad = added_validate(blob, tok_offsets, n, (uint32_t)vocab_size());
    if (!bad.empty()) return Status(1, bad);
  }
  std::lock_guard<std::mutex> lk0(D.lane[0].mu), lk1(D.lane[1].mu);  // (always in this order; a result already pending stays as it is)
  std::lock_guard<std::mutex> lkd(D.dec_mu);
  if (!blob) {
    D.add.n.store(0);
    D.add.toks.clear();
    D.add.index.clear();
    D.dec_ready = D.sub_ready = false;  // (the piece tables are made again, without the tokens' entries)
    return Status();
  }
  const AddedTables t = added_tables(blob, tok_offsets, (uint32_t)n);
  const size_t n_blob = (size_t)(tok_offsets[n] - tok_offsets[0]);
  const Status s = on_device(device_, [&]() -> Status {
    // all are allocated and filled, then handed to the encoder together: a failure on the way leaves the tokens as they were
    DevBuf<uint32_t> d_one, d_dir;
    DevBuf<unsigned long long> d_list;
    DevBuf<uint8_t> d_blob;
    d_one.alloc(t.one.size());
    d_dir.alloc(t.dir_off.size());
    d_list.alloc(t.list.size());
    d_blob.alloc(n_blob);
    HIP_CHECK(hipMemcpy(d_one, t.one.data(), t.one.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_dir, t.dir_off.data(), t.dir_off.size() * 4, hipMemcpyHostToDevice));
    if (!t.list.empty()) HIP_CHECK(hipMemcpy(d_list, t.list.data(), t.list.size() * 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_blob, blob + tok_offsets[0], n_blob, hipMemcpyHostToDevice));
    D.add.one = std::move(d_one);
    D.add.dir_off = std::move(d_dir);
    D.add.list = std::move(d_list);
    D.add.blob = std::move(d_blob);
    return Status();
  });
  if (!s.ok()) return s;
  for (int i = 0; i < 4; i++) D.add.first[i] = (unsigned long long)t.first[2 * i] | ((unsigned long long)t.first[2 * i + 1] << 32);
  D.add.toks.clear();
  D.add.index.clear();
  for (unsigned long long k = 0; k < n; k++) {
    D.add.toks.emplace_back((const char *)blob + tok_offsets[k], (size_t)(tok_offsets[k + 1] - tok_offsets[k]));
    D.add.index.emplace(D.add.toks.back(), (uint32_t)k);
  }
  D.add.n.store((uint32_t)n);
  D.dec_ready = D.sub_ready = false;  // (the piece tables are made again, with the tokens' entries)
  return Status();
}
unsigned long long BaseEncoder::n_added_tokens() const { return dev_ ? dev_->add.n.load() : 0ull; }
std::vector<std::string> BaseEncoder::added_tokens() const {
  if (!dev_) return {};
  std::lock_guard<std::mutex> lk(dev_->dec_mu);
  return dev_->add.toks;
}
void BaseEncoder::added_tokens_stats(unsigned long long out[4]) const {
  for (int i = 0; i < 4; i++) out[i] = dev_ ? dev_->add.stats[i].load() : 0ull;
}
unsigned long long BaseEncoder::id_bound() const { return dev_ ? dev_->id_bound((uint32_t)vocab_size()) : (unsigned long long)vocab_size(); }

Status BaseEncoder::added_split_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                                       unsigned long long *n_sub, unsigned long long *n_matches, double *kernel_ms) const {
  if (n_sub) *n_sub = 0;
  if (n_matches) *n_matches = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && !d_offsets) return Status(2, "added_split_device: no offsets");
  if (total_bytes && !d_bytes) return Status(2, "added_split_device: no text");
  const Lane0 l(*dev_);
  EncoderDevice &D = *dev_;
  if (!D.add.n.load()) return Status(1, "added_split_device: no added tokens are set");  // (before any work: the slot stays)
  return on_device(device_, [&]() -> Status {
    auto &sl = D.add.slot;
    sl.valid = false;
    unsigned long long total = 0;
    if (n_sent) {
      const Status s = split_on_lane(D, l.d, d_bytes, d_offsets, n_sent, total_bytes, false, sl.cnt, sl.first, sl.off, sl.tok, &total, ms.next());
      if (!s.ok()) return s;
    }
    sl.n_sent = n_sent;
    sl.n_sub = total;
    sl.valid = true;
    if (n_sub) *n_sub = total;
    if (n_matches) *n_matches = (total - n_sent) / 2;
    return Status();
  });
}

Status BaseEncoder::take_added_split(void *sub_first, void *sub_off, void *tok, unsigned long long n_sent, unsigned long long n_sub, bool to_device) const {
  const char *who = "added_split: no matching split result";
  if (!dev_) return Status(1, who);
  const Lane0 l(*dev_);
  auto &sl = dev_->add.slot;
  if (!sl.valid || n_sent != sl.n_sent || n_sub != sl.n_sub) return Status(1, who);
  return on_device(device_, [&]() -> Status {
    const auto take = [&](void *dst, const void *src, size_t bytes) {  // (a null destination is skipped)
      if (!dst || !bytes) return;
      if (to_device) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, l.d.st));
      else copy_down(device_, dst, src, bytes, l.d.st);
    };
    if (!n_sent) {  // (nothing was launched and no buffer exists: the one entry of sub_first and of sub_offsets is 0)
      const unsigned long long zero = 0;
      for (void *dst : {sub_first, sub_off}) {
        if (dst && to_device) HIP_CHECK(hipMemcpyAsync(dst, &zero, 8, hipMemcpyHostToDevice, l.d.st));
        else if (dst) *(unsigned long long *)dst = 0;
      }
      HIP_CHECK(hipStreamSynchronize(l.d.st));
      return Status();
    }
    take(sub_first, sl.first, (size_t)(n_sent + 1) * 8);
    take(sub_off, sl.off, (size_t)(n_sub + 1) * 8);
    take(tok, sl.tok, (size_t)n_sub * 4);
    HIP_CHECK(hipStreamSynchronize(l.d.st));
    return Status();
  });
}

Status BaseEncoder::set_vocabulary(const uint8_t *allowed, unsigned long long n, unsigned long long *info) const {
  if (info) info[0] = info[1] = info[2] = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  const size_t V = (size_t)vocab_size();
  if (allowed && n != V)
    return Status(1, "set_vocabulary: n must be the vocabulary's size. Current value: vocab_size = " + std::to_string(V) + "; n = " + std::to_string(n) + ";");
  EncoderDevice &D = *dev_;
  const CfgBind bind(D.cfg);
  std::lock_guard<std::mutex> lk0(D.lane[0].mu), lk1(D.lane[1].mu);  // (always in this order; a result already pending stays as it is)
  if (!allowed) {
    D.voc.set = false;
    D.voc.info[0] = D.voc.info[1] = D.voc.info[2] = 0;
    return Status();
  }
  // E(v) in rule order: x and y are made before z (a char, or an earlier rule's z), so no recursion is needed
  std::vector<std::vector<int32_t>> E(V);
  for (size_t v = 0; v < V; v++) E[v].assign(1, (int32_t)v);
  unsigned long long n_allowed = 0, n_split = 0, longest = 1, total = V;
  for (size_t v = 0; v < V; v++) n_allowed += allowed[v] ? 1 : 0;
  for (const BPE_Rule &r : bpe_state.rules) {
    if (r.z >= V || r.x >= V || r.y >= V) return Status(2, "set_vocabulary: a rule names an id outside the vocabulary");
    if (allowed[r.z]) continue;
    std::vector<int32_t> e = E[r.x];
    e.insert(e.end(), E[r.y].begin(), E[r.y].end());
    total += e.size() - E[r.z].size();
    if (total >= 0xfffffff0ull) return Status(2, "set_vocabulary: the expansions do not fit 2^32 ids");
    E[r.z] = std::move(e);
  }
  std::vector<uint32_t> exp_off(V + 1, 0);
  std::vector<int32_t> fwd, rev;
  fwd.reserve((size_t)total);
  rev.reserve((size_t)total);
  for (size_t v = 0; v < V; v++) {
    exp_off[v] = (uint32_t)fwd.size();
    fwd.insert(fwd.end(), E[v].begin(), E[v].end());
    rev.insert(rev.end(), E[v].rbegin(), E[v].rend());
    if (E[v].size() > 1) n_split++;
    longest = std::max<unsigned long long>(longest, E[v].size());
  }
  exp_off[V] = (uint32_t)fwd.size();
  const Status s = on_device(device_, [&]() -> Status {
    // all three are allocated and filled, then handed to the encoder together: a failure on the way leaves the vocabulary as it was
    DevBuf<uint32_t> d_off;
    DevBuf<int32_t> d_fwd, d_rev;
    d_off.alloc(exp_off.size());
    d_fwd.alloc(fwd.size());
    d_rev.alloc(rev.size());
    HIP_CHECK(hipMemcpy(d_off, exp_off.data(), exp_off.size() * 4, hipMemcpyHostToDevice));
    if (!fwd.empty()) HIP_CHECK(hipMemcpy(d_fwd, fwd.data(), fwd.size() * 4, hipMemcpyHostToDevice));
    if (!rev.empty()) HIP_CHECK(hipMemcpy(d_rev, rev.data(), rev.size() * 4, hipMemcpyHostToDevice));
    D.voc.exp_off = std::move(d_off);
    D.voc.exp_fwd = std::move(d_fwd);
    D.voc.exp_rev = std::move(d_rev);
    return Status();
  });
  if (!s.ok()) return s;
  D.voc.vocab = (uint32_t)V;
  D.voc.info[0] = n_allowed;
  D.voc.info[1] = n_split;
  D.voc.info[2] = longest;
  D.voc.set = true;
  if (info) for (int i = 0; i < 3; i++) info[i] = D.voc.info[i];
  return Status();
}

void BaseEncoder::vocabulary_stats(unsigned long long out[4]) const {
  for (int i = 0; i < 4; i++) out[i] = dev_ ? dev_->voc.stats[i].load() : 0ull;
}

Status BaseEncoder::restrict_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, bool reverse,
                                        unsigned long long *n_out, double *kernel_ms) const {
  if (n_out) *n_out = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && !d_offsets) return Status(2, "restrict_ids_device: no offsets");
  if (n_ids && !d_ids) return Status(2, "restrict_ids_device: no ids");
  if (((uintptr_t)d_ids & 3u) != 0) return Status(2, "restrict_ids_device: the ids must be 4-byte aligned");
  const Lane0 l(*dev_);
  if (!dev_->voc.set) return Status(1, "restrict_ids_device: no vocabulary is set");  // (before any work: what was pending stays)
  return restrict_on_lane(*dev_, l.d, device_, (const int32_t *)d_ids, (const unsigned long long *)d_offsets, n_sent, n_ids, reverse, false, n_out, ms.next());
}

// the encode of a batch as its offsets cut it: K5 (or the word cache), the gather, and the tails of the restriction and the byte fallback
static Status encode_plain_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_bytes, const void *d_offsets,
                                   unsigned long long n_sent, unsigned long long total_bytes, unsigned long long max_sentence_bytes, bool bos, bool eos,
                                   bool reverse, double dropout_prob, unsigned long long *n_ids_out, double *kernel_ms) {
  return on_device(device, [&]() -> Status {
    d.res.n_sent = n_sent;
    d.res.n_ids = 0;
    d.res.made = true;
    d.sp.valid = false;  // (spans belong to the ids they were made from)
    if (n_ids_out) *n_ids_out = 0;
    if (n_sent == 0) return Status();
    d.k5.counts.grow((size_t)n_sent);
    d.res.off.grow((size_t)n_sent + 1);
    const auto tails = [&]() -> Status {  // both exits: the passes over the ids the encode has left, with the lane's own text and offsets
      const Status r = restrict_tail(D, d, device, reverse, n_ids_out, kernel_ms);
      return r.ok() ? bytefb_tail(enc, D, d, device, d_bytes, d_offsets, reverse, n_ids_out, kernel_ms) : r;
    };
    EventPair ev(d.st, kernel_ms != nullptr);
    ev.start();
    // the word cache: no dropout (its draws are per occurrence), a batch worth the extra passes, a buffer the 8-byte loads can walk
    const bool cached = dropout_prob <= 0 && D.cache_mode != 0 && (D.cache_mode == 1 || total_bytes >= D.cache_min_bytes) &&
                        ((uintptr_t)d_bytes & 7u) == 0 && total_bytes < (1ull << 40) && total_bytes > 0;
    d.wc.distinct_words = 0;
    D.last_distinct_words.store(0);
    if (cached) {
      encode_cached(D, d, d_bytes, (const unsigned long long *)d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, n_ids_out);
      ev.stop(true);
      if (kernel_ms) *kernel_ms = ev.elapsed_ms();
      return tails();
    }
    k5_pass(D, d, d_bytes, (const unsigned long long *)d_offsets, nullptr, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob,
            d.k5.counts);
    ev.stop();
    const unsigned long long total = scan_counts(d, d.k5.counts, n_sent, d.res.off);
    d.res.ids.grow((size_t)total);
    launch_encode_gather(d.k5.scratch, (const unsigned long long *)d_offsets, nullptr, d.res.off, n_sent, d.res.ids, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
    d.res.n_ids = total;
    if (n_ids_out) *n_ids_out = total;
    return tails();
  });
}

// With added tokens set: split; without a match in the batch the encode as before on the caller's offsets; else the encode of the refined batch
// (its sentences are every sentence's segments and matches in text order) forward and without bos / eos -- its tails get the refined offsets, so
// the restriction and the byte fallback compose by construction --, then the join, which leaves the caller's n_sent sentences.
Status encode_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_bytes, const void *d_offsets,
                      unsigned long long n_sent, unsigned long long total_bytes, unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse,
                      double dropout_prob, unsigned long long *n_ids_out, double *kernel_ms) {
  const Status tokens = check_bos_eos(enc, bos, eos);
  if (!tokens.ok()) return tokens;
  if (!D.add.n.load() || n_sent == 0)
    return encode_plain_on_lane(enc, D, d, device, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, n_ids_out, kernel_ms);
  double ms_split = 0, ms_enc = 0, ms_join = 0;
  unsigned long long n_sub = 0;
  Status s = on_device(device, [&]() -> Status {
    return split_on_lane(D, d, d_bytes, d_offsets, n_sent, total_bytes, true, d.ad.cnt, d.ad.first, d.ad.off, d.ad.tok, &n_sub, kernel_ms ? &ms_split : nullptr);
  });
  if (!s.ok()) return s;
  D.add.stats[0] += 1;
  if (n_sub == n_sent) {
    D.add.stats[1] += 1;
    D.add.stats[3] += n_sent;
    s = encode_plain_on_lane(enc, D, d, device, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, n_ids_out, kernel_ms);
    if (kernel_ms) *kernel_ms += ms_split;
    return s;
  }
  D.add.stats[2] += (n_sub - n_sent) / 2;
  D.add.stats[3] += n_sub;
  unsigned long long n_refined = 0;
  s = encode_plain_on_lane(enc, D, d, device, d_bytes, d.ad.off.p, n_sub, total_bytes, max_sentence_bytes, false, false, false, dropout_prob, &n_refined,
                           kernel_ms ? &ms_enc : nullptr);
  if (s.ok()) {
    s = on_device(device, [&]() -> Status {
      unsigned long long n_out = 0;
      const Status j = join_on_lane(enc, d, n_sent, bos, eos, reverse, &n_out, kernel_ms ? &ms_join : nullptr);
      if (j.ok() && n_ids_out) *n_ids_out = n_out;
      return j;
    });
  }
  if (!s.ok()) {  // (a refined batch must not stay pending as if it were the caller's)
    d.res.n_sent = n_sent;
    d.res.n_ids = 0;
    d.res.made = false;
    if (n_ids_out) *n_ids_out = 0;
    return s;
  }
  if (kernel_ms) *kernel_ms = ms_split + ms_enc + ms_join;
  return Status();
}

static size_t staged_from() {
  const std::shared_ptr<const Config> C = cfg();  // (tests: every copy through the chunks)
  return C->enc_staged_from.set ? (size_t)C->enc_staged_from.u : (size_t)(16u << 20);
}
void copy_up(int device, void *d_dst, const void *src, size_t n, hipStream_t st) {
  if (n >= staged_from() && n) {
    staged_transfer(device, (uint8_t *)d_dst, n, true, [&](void *chunk, unsigned long long off, size_t len) {
      memcpy(chunk, (const uint8_t *)src + off, len);
      return true;
    }, nullptr, ENC_CHUNK);
  } else if (n) {
    HIP_CHECK(hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, st));
  }
}
void copy_down(int device, void *dst, const void *d_src, size_t n, hipStream_t st) {
  if (n >= staged_from() && n) {
    staged_transfer(device, (uint8_t *)const_cast<void *>(d_src), n, false, [&](void *chunk, unsigned long long off, size_t len) {
      memcpy((uint8_t *)dst + off, chunk, len);
      return true;
    }, nullptr, ENC_CHUNK);
  } else if (n) {
    HIP_CHECK(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, st));
  }
}

Status copy_out_device(int device, EncodeLane &d, void *dst_a, const void *src_a, size_t n_a, void *dst_off, const unsigned long long *src_off,
                       unsigned long long n_sent) {
  return on_device(device, [&]() -> Status {
    if (n_sent == 0) {
      if (dst_off) HIP_CHECK(hipMemsetAsync(dst_off, 0, 8, d.st));
    } else {
      if (dst_a && n_a) HIP_CHECK(hipMemcpyAsync(dst_a, src_a, n_a, hipMemcpyDeviceToDevice, d.st));
      if (dst_off) HIP_CHECK(hipMemcpyAsync(dst_off, src_off, (size_t)(n_sent + 1) * 8, hipMemcpyDeviceToDevice, d.st));
    }
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

static Status fetch_lane(EncodeLane &d, int device, int32_t *ids, unsigned long long *out_off, unsigned long long n_sent) {
  return on_device(device, [&]() -> Status {
    if (n_sent == 0) { if (out_off) out_off[0] = 0; return Status(); }
    // (the lane's stream is idle: encode_on_lane synchronised it)
    if (ids && d.res.n_ids) copy_down(device, ids, d.res.ids, (size_t)d.res.n_ids * 4, d.st);
    if (out_off) copy_down(device, out_off, d.res.off, (size_t)(n_sent + 1) * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// The device-resident pair (what bench.py times): encode_device leaves its result in lane 0, fetch_device_result copies it
// out.  Each call locks the lane; the PAIR is not atomic -- one host thread at a time may use these two on an encoder.
Status BaseEncoder::encode_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                                  unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                                  unsigned long long *n_ids_out, double *kernel_ms) const {
  if (!dev_) return Status(2, "encoder has no device state");
  const CfgBind bind(dev_->cfg);
  std::lock_guard<std::mutex> lk(dev_->lane[0].mu);
  return encode_on_lane(*this, *dev_, dev_->lane[0], device_, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse,
                        dropout_prob, n_ids_out, kernel_ms);
}

std::shared_ptr<const Config> BaseEncoder::config() const { return dev_ ? dev_->cfg : nullptr; }
void BaseEncoder::set_cache(int mode, unsigned long long min_bytes) const {
  if (!dev_) return;
  dev_->cache_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  dev_->cache_min_bytes = min_bytes;
}
unsigned long long BaseEncoder::cache_words() const {
  if (!dev_) return 0;
  return dev_->last_distinct_words.load();  // (of the most recent batch, whichever lane ran it)
}

Status BaseEncoder::fetch_device_result(int32_t *ids, unsigned long long *out_off, unsigned long long n_sent) const {
  if (!dev_) return Status(2, "fetch_device_result: no matching result");
  const CfgBind bind(dev_->cfg);
  std::lock_guard<std::mutex> lk(dev_->lane[0].mu);
  if (n_sent != dev_->lane[0].res.n_sent) return Status(2, "fetch_device_result: no matching result");
  return fetch_lane(dev_->lane[0], device_, ids, out_off, n_sent);
}

// upload -> K5 -> download on one lane; the output arrays come from the caller's allocator once their sizes are known
template <class AllocIds, class AllocOff>
static Status encode_host_to_host(const BaseEncoder &enc, EncoderDevice *dev, int device, const uint8_t *bytes, const unsigned long long *offsets,
                                  unsigned long long n_sent, bool bos, bool eos, bool reverse, double dropout_prob, AllocIds alloc_ids, AllocOff alloc_off) {
  Status s = check_bos_eos(enc, bos, eos);
  if (!s.ok()) return s;
  if (n_sent == 0) {
    unsigned long long *o = alloc_off(1);
    if (o) o[0] = 0;
    (void)alloc_ids(0);
    return Status();
  }
  if (!dev) return Status(2, "encoder has no device state");
  const bool trace = cfg()->trace.set;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); };
  unsigned long long total_bytes = offsets[n_sent] - offsets[0], max_len = 0;
  // (the longest sentence sizes K5's scratch; a pass over 80 MB of offsets for 10^7 sentences -- on its own thread while the bytes go up)
  std::thread scan;
  auto longest = [&] { for (unsigned long long i = 0; i < n_sent; i++) max_len = std::max(max_len, offsets[i + 1] - offsets[i]); };
  if (n_sent >= (1u << 20)) scan = std::thread(longest);
  else longest();
  struct Joiner {
    std::thread &t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{scan};
  std::unique_lock<std::mutex> lk;
  EncodeLane &d = dev->acquire(lk);  // held until the ids are back on the host
  const auto t1 = now();
  s = on_device(device, [&]() -> Status {
    d.in.bytes.grow((size_t)total_bytes + 16);
    d.in.off.grow((size_t)n_sent + 1);
    copy_up(device, d.in.bytes, bytes + offsets[0], (size_t)total_bytes, d.st);
    std::vector<unsigned long long> rel;  // offsets are rebased to the first byte of the batch
    if (offsets[0] != 0) {
      rel.resize((size_t)n_sent + 1);
      for (unsigned long long i = 0; i <= n_sent; i++) rel[i] = offsets[i] - offsets[0];
    }
    copy_up(device, d.in.off, rel.empty() ? offsets : rel.data(), ((size_t)n_sent + 1) * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
  if (!s.ok()) return s;
  if (scan.joinable()) scan.join();
  const double ms_up = ms_since(t1);
  const auto t2 = now();
  unsigned long long n_ids = 0;
  s = encode_on_lane(enc, *dev, d, device, d.in.bytes, d.in.off, n_sent, total_bytes, max_len, bos, eos, reverse, dropout_prob, &n_ids, nullptr);
  if (!s.ok()) return s;
  const double ms_enc = ms_since(t2);
  const auto t3 = now();
  int32_t *ids = alloc_ids((size_t)n_ids);
  unsigned long long *off = alloc_off((size_t)n_sent + 1);
  if ((n_ids && !ids) || !off) return Status(2, "out of memory");
  const double ms_alloc = ms_since(t3);
  const auto t4 = now();
  s = fetch_lane(d, device, ids, off, n_sent);
  if (trace)
    fprintf(stderr, "[yttm] encode host -> host: %llu sentences, %.1f MB up, %.1f MB down: copy up %.1f ms, encode %.1f ms, result arrays %.1f ms, copy down %.1f ms\n",
            n_sent, (double)(total_bytes + 8 * n_sent) / 1e6, (double)(4 * n_ids + 8 * n_sent) / 1e6, ms_up, ms_enc, ms_alloc, ms_since(t4));
  return s;
}

Status BaseEncoder::encode_as_ids(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos,
                                  bool reverse, double dropout_prob, std::vector<int32_t> *ids, std::vector<unsigned long long> *out_off) const {
  ids->clear();
  out_off->clear();
  const CfgBind bind(config());
  return encode_host_to_host(
      *this, dev_, device_, bytes, offsets, n_sent, bos, eos, reverse, dropout_prob,
      [&](size_t n) { ids->resize(n); return ids->data(); }, [&](size_t n) { out_off->assign(n, 0); return out_off->data(); });
}

// A large one is asked for in huge pages: the first touch of 1.2 GB of fresh 4 KB pages -- 3e5 page faults -- took 130 ms of a 10^7-sentence
// call, four times the link time of the copy that does the touching (MI355X box, transparent huge pages on "madvise").
void *result_alloc(size_t bytes) {
  constexpr size_t HUGE = 2u << 20;
  if (bytes < 4 * HUGE) return malloc(bytes);
  void *p = nullptr;
  if (posix_memalign(&p, HUGE, (bytes + HUGE - 1) / HUGE * HUGE) != 0) return malloc(bytes);
#ifdef MADV_HUGEPAGE
  (void)madvise(p, (bytes + HUGE - 1) / HUGE * HUGE, MADV_HUGEPAGE);
#endif
  return p;
}

Status run_two_lanes(const char *who, const std::shared_ptr<const Config> &cfg, int device, size_t n_items,
                     const std::function<Status(size_t i, bool *exhausted)> &upload, const std::function<Status(size_t i)> &work,
                     const std::function<Status(size_t i)> &download, size_t *n_done) {
  std::mutex mu;
  std::condition_variable cv;
  size_t up_n = 0, work_n = 0, down_n = 0;  // items each leg has finished (these, n_items and `failure` are guarded by mu)
  Status failure;
  // One leg: item i once the leg it follows has finished item i - lag, until there is no item i or somebody has failed.
  auto leg = [&](const char *name, const size_t &before, size_t lag, size_t &done, const std::function<Status(size_t)> &item) {
    const CfgBind bind(cfg);  // (the caller's snapshot: this thread's copies read the hooks too)
    Status s;
    try {
      s = on_device(device, [&]() -> Status {
        for (size_t i = 0;; i++) {
          {
            std::unique_lock<std::mutex> g(mu);
            cv.wait(g, [&] { return !failure.ok() || i >= n_items || before + lag > i; });
            if (!failure.ok() || i >= n_items) return Status();
          }
          const Status r = item(i);
          if (!r.ok()) return r;
          std::lock_guard<std::mutex> g(mu);
          if (i >= n_items) return Status();  // (the upload found the input exhausted)
          done = i + 1;
          cv.notify_all();
        }
      });
    } catch (const std::exception &e) {  // (bad_alloc from a grow, ...: an error of this call, never std::terminate of the host process)
      s = Status(2, std::string(who) + " (" + name + " thread): " + e.what());
    } catch (...) {
      s = Status(2, std::string(who) + " (" + name + " thread): unknown exception");
    }
    std::lock_guard<std::mutex> g(mu);
    if (!s.ok() && failure.ok()) failure = s;  // the first failure wins
    cv.notify_all();
  };
  std::thread up([&] {
    leg("upload", down_n, 2, up_n, [&](size_t i) {
      bool exhausted = false;
      const Status r = upload(i, &exhausted);
      if (exhausted) {
        std::lock_guard<std::mutex> g(mu);
        n_items = i;
        cv.notify_all();
      }
      return r;
    });
  });
  std::thread down([&] { leg("download", work_n, 0, down_n, download); });
  leg("work", up_n, 0, work_n, work);
  up.join();
  down.join();
  if (n_done) *n_done = work_n;
  return failure;
}

// A very large batch in sub-batches through both lanes: while sub-batch i is being encoded, i + 1 crosses the link upwards and the ids of
// i - 1 downwards (run_two_lanes).  One after the other the three legs of 10^7 sentences are 25 + 28 + 25 ms; the
// link works both ways at once (measured: 79 -> 64 ms in sub-batches of 320 MB; smaller ones lose it again to the word cache's fixed costs
// and to words that recur across sub-batches).  The ids' array is asked for at its upper bound -- a sentence of B bytes has at most B + 1 tokens
// (enc_tokenize) -- in pages that are only ever touched up to the real size; returns false (nothing done) when that much address space is
// not to be had or a lane is busy: the caller then takes the plain path.
static bool encode_pipelined(const BaseEncoder &enc, EncoderDevice *dev, int device, const uint8_t *bytes, const unsigned long long *offsets,
                             unsigned long long n_sent, bool bos, bool eos, bool reverse, double dropout_prob, int32_t **ids_out,
                             unsigned long long **off_out, Status *result) {
  const unsigned long long total_bytes = offsets[n_sent] - offsets[0];
  const std::shared_ptr<const Config> C = cfg();
  unsigned long long sub_bytes = (unsigned long long)std::max<long long>(1, C->enc_sub_mb.i) << 20;
  if (C->enc_sub_kb.set) sub_bytes = (unsigned long long)std::max<long long>(1, C->enc_sub_kb.i) << 10;  // (tests)
  const unsigned long long min_bytes = C->enc_pipe_from.u;
  if (total_bytes < min_bytes || n_sent < 4) return false;
  // sub-batches of about sub_bytes each, cut at sentence starts
  std::vector<unsigned long long> cut{0};
  while (cut.back() < n_sent) {
    const unsigned long long want = offsets[cut.back()] + sub_bytes;
    unsigned long long s = (unsigned long long)(std::upper_bound(offsets + cut.back() + 1, offsets + n_sent + 1, want) - offsets) - 1;
    if (s <= cut.back()) s = cut.back() + 1;
    cut.push_back(std::min(s, n_sent));
  }
  const size_t K = cut.size() - 1;
  if (K < 2) return false;
  std::unique_lock<std::mutex> lk0(dev->lane[0].mu, std::try_to_lock), lk1(dev->lane[1].mu, std::try_to_lock);
  if (!lk0.owns_lock() || !lk1.owns_lock()) return false;
  const unsigned long long ids_cap = total_bytes + n_sent * (1ull + (bos ? 1 : 0) + (eos ? 1 : 0)) + 1;
  int32_t *ids = (int32_t *)result_alloc(ids_cap * sizeof(int32_t));
  unsigned long long *off = (unsigned long long *)result_alloc((n_sent + 1) * sizeof(unsigned long long));
  if (!ids || !off) {
    free(ids);
    free(off);
    return false;
  }
  std::vector<unsigned long long> n_ids(K, 0), max_len(K, 0);
  unsigned long long ids_base = 0;  // (the download leg's: ids of the sub-batches before this one)
  auto upload = [&](size_t i, bool *) {
    EncodeLane &d = dev->lane[i & 1];
    const unsigned long long s0 = cut[i], ns = cut[i + 1] - s0, b0 = offsets[s0], nb = offsets[s0 + ns] - b0;
    unsigned long long mx = 0;
    for (unsigned long long j = 0; j < ns; j++) mx = std::max(mx, offsets[s0 + j + 1] - offsets[s0 + j]);
    max_len[i] = mx;
    d.in.bytes.grow((size_t)nb + 16);
    d.in.off.grow((size_t)ns + 1);
    if (nb)
      staged_transfer(device, d.in.bytes, nb, true, [&](void *chunk, unsigned long long o, size_t len) {
        memcpy(chunk, bytes + b0 + o, len);
        return true;
      }, nullptr, ENC_CHUNK);
    staged_transfer(device, (uint8_t *)d.in.off.p, (ns + 1) * 8, true, [&](void *chunk, unsigned long long o, size_t len) {
      unsigned long long *dst = (unsigned long long *)chunk;  // (offsets relative to the sub-batch's first byte)
      const unsigned long long *src = offsets + s0 + o / 8;
      for (size_t j = 0; j < len / 8; j++) dst[j] = src[j] - b0;
      return true;
    }, nullptr, ENC_CHUNK);
    return Status();
  };
  auto work = [&](size_t i) {
    EncodeLane &d = dev->lane[i & 1];
    const unsigned long long s0 = cut[i], ns = cut[i + 1] - s0, nb = offsets[s0 + ns] - offsets[s0];
    return encode_on_lane(enc, *dev, d, device, d.in.bytes, d.in.off, ns, nb, max_len[i], bos, eos, reverse, dropout_prob, &n_ids[i], nullptr);
  };
  auto download = [&](size_t i) {
    EncodeLane &d = dev->lane[i & 1];
    const unsigned long long s0 = cut[i], ns = cut[i + 1] - s0;
    if (n_ids[i])
      staged_transfer(device, (uint8_t *)d.res.ids.p, n_ids[i] * 4, false, [&](void *chunk, unsigned long long o, size_t len) {
        memcpy((uint8_t *)(ids + ids_base) + o, chunk, len);
        return true;
      }, nullptr, ENC_CHUNK);
    staged_transfer(device, (uint8_t *)d.res.off.p, (ns + 1) * 8, false, [&](void *chunk, unsigned long long o, size_t len) {
      const unsigned long long *src = (const unsigned long long *)chunk;  // (the sub-batch's offsets start at 0: moved behind the ids so far;
      unsigned long long *dst = off + s0 + o / 8;                         //  its last entry is the next one's first, written twice, the same)
      for (size_t j = 0; j < len / 8; j++) dst[j] = src[j] + ids_base;
      return true;
    }, nullptr, ENC_CHUNK);
    ids_base += n_ids[i];
    return Status();
  };
  *result = run_two_lanes("encode", C, device, K, upload, work, download);
  if (!result->ok()) {
    free(ids);
    free(off);
    return true;
  }
  if (cfg()->trace.set) fprintf(stderr, "[yttm] encode host -> host: %llu sentences in %zu sub-batches through both lanes\n", n_sent, K);
  {
    // The array was asked for at its upper bound (four bytes per input byte and more); what the caller keeps until its free() is the ids
    // themselves: the tail -- never touched, so never backed by memory, but address space under RLIMIT_AS / strict overcommit -- goes back
    // now.  A shrinking realloc of an mmap'ed block is an mremap; the alignment of the block's start stays what it was.
    const unsigned long long used = off[n_sent];
    if (void *small = realloc(ids, (size_t)std::max<unsigned long long>(used, 1) * sizeof(int32_t))) ids = (int32_t *)small;
  }
  *ids_out = ids;
  *off_out = off;
  return true;
}

// the same into malloc'ed arrays (released by the caller with free()): what the C ABI hands out, without a copy in between
Status BaseEncoder::encode_as_ids_malloc(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos,
                                         bool reverse, double dropout_prob, int32_t **ids, unsigned long long **out_off) const {
  *ids = nullptr;
  *out_off = nullptr;
  const CfgBind bind(config());
  if (dev_ && n_sent && check_bos_eos(*this, bos, eos).ok()) {
    Status piped;
    if (encode_pipelined(*this, dev_, device_, bytes, offsets, n_sent, bos, eos, reverse, dropout_prob, ids, out_off, &piped)) return piped;
  }
  Status s = encode_host_to_host(
      *this, dev_, device_, bytes, offsets, n_sent, bos, eos, reverse, dropout_prob,
      [&](size_t n) { *ids = (int32_t *)result_alloc((n ? n : 1) * sizeof(int32_t)); return *ids; },
      [&](size_t n) { *out_off = (unsigned long long *)result_alloc((n ? n : 1) * sizeof(unsigned long long)); return *out_off; });
  if (!s.ok()) {
    free(*ids);
    free(*out_off);
    *ids = nullptr;
    *out_off = nullptr;
  }
  return s;
}

Status BaseEncoder::encode_as_subwords(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos,
                                       bool reverse, double dropout_prob, std::vector<std::string> *pieces,
                                       std::vector<unsigned long long> *piece_off) const {
  // ids come from the GPU (forward order, no bos/eos); pieces are a host lookup (bpe.cpp:1597-1613).  The k-th unk id
  // of a sentence is the k-th run of unknown chars, whose text is recovered from the sentence itself.
  const CfgBind bind(config());
  if (n_added_tokens() && !byte_fallback()) return Status(1, SUBWORD_UNDER_ADDED_TOKENS);
  Status s = check_bos_eos(*this, bos, eos);
  if (!s.ok()) return s;
  std::vector<int32_t> ids;
  std::vector<unsigned long long> off;
  s = encode_as_ids(bytes, offsets, n_sent, false, false, false, dropout_prob, &ids, &off);
  if (!s.ok()) return s;
  pieces->clear();
  piece_off->assign(1, 0);
  const int unk = bpe_state.special_tokens.unk_id;
  for (unsigned long long i = 0; i < n_sent; i++) {
    std::vector<std::string> sent;
    if (bos) sent.push_back(BOS_TOKEN);
    // unknown runs of this sentence, in order
    std::vector<std::string> unk_runs;
    {
      std::vector<uint32_t> text = decode_utf8((const char *)bytes + offsets[i], (const char *)bytes + offsets[i + 1]);
      std::vector<uint32_t> run;
      for (uint32_t c : text) {
        const bool known = !is_space(c) && char2id.count(c);
        if (!is_space(c) && !known) { run.push_back(c); continue; }
        if (!run.empty()) { unk_runs.push_back(encode_utf8(run)); run.clear(); }
      }
      if (!run.empty()) unk_runs.push_back(encode_utf8(run));
    }
    size_t next_unk = 0;
    for (unsigned long long k = off[i]; k < off[i + 1]; k++) {
      const int id = ids[k];
      if (id == unk) {
        sent.push_back(next_unk < unk_runs.size() ? unk_runs[next_unk++] : std::string());
      } else {
        std::string piece;
        id_to_subword(id, &piece, false);
        sent.push_back(piece);
      }
    }
    if (eos) sent.push_back(EOS_TOKEN);
    if (reverse) std::reverse(sent.begin(), sent.end());
    for (auto &p : sent) pieces->push_back(std::move(p));
    piece_off->push_back(pieces->size());
  }
  return Status();
}

Status BaseEncoder::id_to_subword(int id, std::string *subword, bool replace_space) const {  // bpe.cpp:1774-1807
  if (bytefb_is_byte_id(id, (uint32_t)vocab_size(), byte_fallback())) {  // (the name; decode() and the decode table put the raw byte)
    *subword = bytefb_name((uint32_t)(id - vocab_size()));
    return Status();
  }
  if (added_is_added_id(id, (uint32_t)vocab_size(), (uint32_t)n_added_tokens())) {  // the token verbatim
    *subword = dev_->add.toks[(size_t)id - added_first((uint32_t)vocab_size())];
    return Status();
  }
  if (id < 0 || vocab_size() <= id)
    return Status(1, "id must be in the range [0, vocab_size - 1]. Current value: vocab_size = " + std::to_string(vocab_size()) +
                         "; id=" + std::to_string(id) + ";");
  const SpecialTokens &sp = bpe_state.special_tokens;
  if (sp.unk_id == id) { *subword = UNK_TOKEN; return Status(); }
  if (sp.pad_id == id) { *subword = PAD_TOKEN; return Status(); }
  if (sp.bos_id == id) { *subword = BOS_TOKEN; return Status(); }
  if (sp.eos_id == id) { *subword = EOS_TOKEN; return Status(); }
  auto it = recipe.find((uint32_t)id);
  if (it == recipe.end()) { subword->clear(); return Status(); }
  std::vector<uint32_t> cps;
  for (uint32_t t : it->second) cps.push_back(id2char.at(t));
  if (replace_space && !cps.empty() && cps[0] == SPACE_TOKEN) {
    *subword = " " + encode_utf8(std::vector<uint32_t>(cps.begin() + 1, cps.end()));
    return Status();
  }
  *subword = encode_utf8(cps);
  return Status();
}

int BaseEncoder::subword_to_id(const std::string &token) const {  // bpe.cpp:1809-1826
  const SpecialTokens &sp = bpe_state.special_tokens;
  if (UNK_TOKEN == token) return sp.unk_id;
  if (PAD_TOKEN == token) return sp.pad_id;
  if (BOS_TOKEN == token) return sp.bos_id;
  if (EOS_TOKEN == token) return sp.eos_id;
  if (byte_fallback() && bytefb_parse_name(token) >= 0) return vocab_size() + bytefb_parse_name(token);
  if (n_added_tokens()) {
    auto at = dev_->add.index.find(token);
    if (at != dev_->add.index.end()) return (int)(added_first((uint32_t)vocab_size()) + at->second);
  }
  auto it = reversed_recipe.find(token);
  if (it != reversed_recipe.end()) return (int)it->second;
  return sp.unk_id;
}

Status BaseEncoder::decode(const std::vector<int> &ids, std::string *sentence, const std::unordered_set<int> *ignore_ids) const {
  // bpe.cpp:1843-1861
  bool first_iter = true;
  for (int id : ids) {
    std::string subword;
    if (!ignore_ids || ignore_ids->count(id) == 0) {
      if (bytefb_is_byte_id(id, (uint32_t)vocab_size(), byte_fallback())) {  // the raw byte, and no strip rule
        *sentence += (char)(id - vocab_size());
        first_iter = false;
        continue;
      }
      if (added_is_added_id(id, (uint32_t)vocab_size(), (uint32_t)n_added_tokens())) {  // the token verbatim, and no strip rule
        *sentence += dev_->add.toks[(size_t)id - added_first((uint32_t)vocab_size())];
        first_iter = false;
        continue;
      }
      Status status = id_to_subword(id, &subword, true);
      if (!status.ok()) return status;
      *sentence += subword;
      if (first_iter && !sentence->empty() && sentence->at(0) == ' ') *sentence = sentence->substr(1);
      first_iter = false;
    }
  }
  return Status();
}

std::vector<std::string> BaseEncoder::vocabulary() const {  // bpe.cpp:1884-1894
  int n = vocab_size();
  std::vector<std::string> vocab((size_t)n);
  for (int i = 0; i < n; i++) id_to_subword(i, &vocab[(size_t)i]);
  return vocab;
}

}  // namespace yttm
