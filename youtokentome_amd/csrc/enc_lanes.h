// enc_lanes.h -- what the encoder's host units (host_encoder.cpp, host_decode.cpp, host_lines.cpp) share: the lanes and their device buffers,
// the model's device state, and the small helpers every entry point is built from.  Internal: nothing outside these units includes it.
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "added_plan.h"
#include "bytefb_plan.h"
#include "gpu_ctx.h"
#include "host_core.h"

namespace yttm {

// One device allocation and its capacity in elements, freed with its owner.
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~DevBuf() { release(); }
  operator T *() const { return p; }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void alloc(size_t n) {  // exactly n elements (at least one), whatever was there before
    release();
    void *q = nullptr;
    HIP_CHECK(hipMalloc(&q, (n ? n : 1) * sizeof(T)));
    p = (T *)q;
    cap = n ? n : 1;
  }
  void grow(size_t need) {  // room for `need` elements and a quarter more; the contents are NOT kept (freed first: never two generations at once)
    if (need > cap) alloc(need + need / 4 + 64);
  }
};

// One batch in flight: a stream and the batch buffers, reused and grown on demand.  Two lanes per encoder, so that two host
// threads (Python threads calling encode() on one BPE object -- ctypes releases the GIL, the reference's Cython binding did
// not --, or the two workers of encode_cli) overlap their copies and kernels instead of racing on one set of buffers.
// The results of the device-resident entries (encode, decode, line split) live side by side in buffers of their own: each is pending until the
// next call of its own kind, whatever the others do.
struct EncodeLane {
  std::mutex mu;  // held for the whole of upload -> encode -> fetch
  hipStream_t st = nullptr;
  struct {  // a host-to-host batch or a file piece: its text and offsets
    DevBuf<uint8_t> bytes;
    DevBuf<unsigned long long> off;
  } in;
  struct {  // K5: ids per item as the kernel leaves them, its per-wave HBM scratch, the counts and their scan (scan_counts, also the other groups')
    DevBuf<int32_t> scratch;
    DevBuf<uint32_t> work, drop, counts;
    DevBuf<unsigned long long> scan_tmp, total;
  } k5;
  struct {  // the encode result
    DevBuf<int32_t> ids;
    DevBuf<unsigned long long> off, misc;  // misc[0]: longest row (k_enc_longest)
    unsigned long long n_ids = 0, n_sent = 0;
    bool made = false;  // an encode or a parse has left a result here (n_sent == 0 is a result too)
  } res;
  struct {  // the vocabulary restriction (k_restrict.h): the second pair of buffers its pass writes, swapped with res's; the lengths it measures
    DevBuf<int32_t> ids;
    DevBuf<unsigned long long> off;
    DevBuf<uint32_t> len;
  } rs;
  struct {  // the byte fallback (k_bytefb.h) writes into rs's buffers too, one pass after the other; saw[0]: the measure pass met an unk_id
    DevBuf<uint32_t> saw;
  } fb;
  struct {  // the added tokens (k_added.h): the split of the batch in flight -- cnt[n_sent], first[n_sent + 1], the refined off[n_sub + 1], tok[n_sub]
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> first, off;
    DevBuf<int32_t> tok;
  } ad;
  struct {  // word cache (k_wcache.hip): the batch's table of distinct words, the slot of every occurrence, the list K5 encodes, its ids
    DevBuf<unsigned long long> slot, pos, extra, blk_off, ustart, uend;
    DevBuf<uint32_t> occ, blk, uslot, ucounts;
    DevBuf<unsigned int> misc;                 // [0] number of uncached words, [1] status
    unsigned long long distinct_words = 0;     // of the last cached batch (0: the batch went straight through K5)
  } wc;
  struct {  // device decode (host_decode.cpp); the SUBWORD formatter leaves its text here too (len, off, bytes)
    DevBuf<uint32_t> len, ign;  // ign: ignore bitmap, then the ignored ids outside [0, vocab)
    DevBuf<unsigned long long> off, misc;  // misc[0]: smallest flat index of an invalid id
    DevBuf<uint8_t> bytes;
    unsigned long long n_sent = 0, n_bytes = 0;
    bool valid = false;
  } dec;
  struct {  // byte spans of the encode result pending beside them (host_decode.cpp, k_spans.h): uint32 [n_ids][2]; any later encode empties the slot
    DevBuf<uint32_t> spans, misc;  // misc[0]: the kernel's "the ids do not fit the text"
    unsigned long long n_sent = 0, n_ids = 0;
    bool valid = false;
  } sp;
  struct {  // line split (host_lines.cpp): newlines per tile, their scan, the lines' offsets
    DevBuf<uint32_t> cnt;
    DevBuf<unsigned long long> rank, off, misc;  // misc[0]: longest line (k_lines_longest)
    unsigned long long n_lines = 0, n_bytes = 0, longest = 0;
    bool valid = false;
  } ln;

  void init() {  // (on the encoder's device) the stream and the small fixed blocks
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    k5.total.alloc(2);
    wc.misc.alloc(2);
    res.misc.alloc(1);
    fb.saw.alloc(1);
    dec.misc.alloc(1);
    sp.misc.alloc(1);
    ln.misc.alloc(1);
  }
  ~EncodeLane() {
    if (st) (void)hipStreamDestroy(st);
  }
};

struct EncoderDevice {
  DevBuf<uint32_t> cpmap, rule_z, bloom;
  DevBuf<RuleSlot> rules;
  DevBuf<unsigned long long> rule_xy;
  EncModel m{};
  std::shared_ptr<const Config> cfg;  // the hooks as they stood at creation (BaseEncoder::config)
  // BPE-dropout draws: counter-based, seeded per call from a per-encoder random salt (the reference draws from a
  // std::random_device-independent global mt19937, bpe.cpp:1415; YTTM_DROPOUT_SEED pins the salt for reproducible runs)
  std::atomic<unsigned long long> dropout_calls{0};
  unsigned long long seed_salt = 0;
  // word cache: 0 = never, 1 = whenever it applies (no dropout), 2 = for batches of at least cache_min_bytes (YTTM_ENCODE_CACHE = 0 | 1;
  // YTTM_ENCODE_CACHE_MIN_MB moves the threshold)
  int cache_mode = 2;
  unsigned long long cache_min_bytes = 8ull << 20;  // (tools/dbg/cache_crossover.py: text 0.9x at 4 MB, 1.1x at 8, 2.3x at 32, 3.2x at 128; random words break even at ~10 MB)
  static constexpr int N_LANES = 2;
  EncodeLane lane[N_LANES];
  std::atomic<unsigned int> next_lane{0};
  std::atomic<unsigned long long> last_distinct_words{0};  // of the most recent batch (cache_words())
  // piece table of the device decode (host_decode.cpp), made at the first device decode
  std::mutex dec_mu;
  bool dec_ready = false;
  DevBuf<uint8_t> piece_blob;
  DevBuf<uint32_t> piece_off;
  uint32_t dec_vocab = 0;
  // piece table of the SUBWORD formatter (host_decode.cpp): id_to_subword(id, replace_space = false), made at the first format (under dec_mu)
  bool sub_ready = false;
  DevBuf<uint8_t> sub_blob;
  DevBuf<uint32_t> sub_off;
  DevBuf<uint32_t> sub_units;  // [vocab] the units an id covers (k_spans.h), filled beside the pieces
  // token frequencies (host_decode.cpp, k_idcount.h): uint64 [n_bins + 1], the encoder's own and no lane's -- no encode, decode, parse or file
  // call empties it.  Read and written under lane 0's mutex, which every entry that counts or takes the counts holds.
  struct {
    DevBuf<unsigned long long> counts;
    unsigned long long n_bins = 0;
    bool valid = false;
  } idc;
  // training blocks (host_decode.cpp, k_blocks.h), the encoder's own like the counts and under lane 0's mutex: the slot of the last blocks call
  // (rows, seg, pos: [n_rows][L] rounded up to a multiple of 4 elements; frags [n_frags][2]; row_frags [n_rows + 1]), the open row in two
  // generations (a call reads one and writes the other), and the passes' working arrays.
  struct {
    DevBuf<int32_t> rows, seg, pos, frags;
    DevBuf<unsigned long long> row_frags;
    unsigned long long n_rows = 0, n_frags = 0, L = 0;
    bool valid = false;
    DevBuf<int32_t> open_ids[2];
    DevBuf<unsigned long long> open_off[2];
    int gen = 0;                                              // the generation that holds the open row
    unsigned long long open_f = 0, open_m = 0, open_L = 0;    // its ids and fragments; the (L, mode) it is bound to while open_f > 0
    int open_mode = 0;
    DevBuf<uint32_t> cnt, nxt, entry, rowbase, rowsent, rowcnt;
    DevBuf<unsigned long long> ne, hop, rowsrc, info;  // info[0 .. 2] (k_blocks.h), info[3]: a sentence longer than L
  } blk;
  // batches by length under a token budget (host_decode.cpp, k_batches.h), the encoder's own like the blocks' slot and under lane 0's mutex: the
  // plan (order [n], batch_first [n_batches + 1]) of the last plan call, the gathered part (widths [n_batches], batch_off [n_batches + 1], out
  // [n_elems] rounded up to a multiple of 4) of the last gather under that plan, and the passes' working arrays.  A gather measures into
  // w_widths / w_off and exchanges them with the gathered part once nothing can refuse the call any more.
  struct {
    DevBuf<uint32_t> order;
    DevBuf<unsigned long long> batch_first;
    unsigned long long n = 0, n_kept = 0, n_batches = 0;
    bool planned = false;
    DevBuf<uint32_t> widths;
    DevBuf<unsigned long long> batch_off;
    DevBuf<int32_t> out;
    unsigned long long n_elems = 0;
    bool gathered = false;
    DevBuf<uint32_t> key, key1, key2, idx1, idx2, skey, hist, nxt, entry, base, cnt, w_widths;
    DevBuf<unsigned long long> hist_off, hop, w_off, info;  // info[0]: a sentence the rule refuses, [1]: n_kept, [2]: n_batches, [3]: the elements
  } bat;
  // the restricted vocabulary (host_encoder.cpp set_vocabulary, k_restrict.h): exp_ids[exp_off[v] .. exp_off[v + 1]) = E(v), and the same with every
  // expansion back to front.  Written with every lane locked, read by a call that holds its lane: a call never sees half a table.
  struct {
    bool set = false;
    DevBuf<uint32_t> exp_off;
    DevBuf<int32_t> exp_fwd, exp_rev;
    uint32_t vocab = 0;
    unsigned long long info[3] = {0, 0, 0};               // allowed ids, ids that split, the longest expansion
    std::atomic<unsigned long long> stats[4] = {{0}, {0}, {0}, {0}};  // restricted calls, calls where nothing split, ids in, ids out
  } voc;
  // the byte fallback (host_encoder.cpp set_byte_fallback, k_bytefb.h): a setting of the encoder like the vocabulary, switched with every lane locked.
  // id_bound(V): the ids the decode, the SUBWORD formatter and the ignore bitmap accept (bytefb_plan.h); their tables always hold V + 256 entries.
  struct {
    std::atomic<bool> on{false};
    std::atomic<unsigned long long> stats[4] = {{0}, {0}, {0}, {0}};  // calls, calls whose write pass was skipped, ids in, ids out
  } bfb;
  // the added tokens (host_encoder.cpp set_added_tokens, k_added.h): a setting of the encoder like the two above, replaced with every lane locked.
  // n == 0: off.  The host's copy (toks, index) serves the names and the host decode; the device tables are those of added_plan.h's added_tables.
  // slot: the result of the last stand-alone split (yttm_added_split_device), the encoder's own and under lane 0's mutex like the counts.
  struct {
    std::atomic<uint32_t> n{0};
    std::vector<std::string> toks;
    std::unordered_map<std::string, uint32_t> index;
    unsigned long long first[4] = {0, 0, 0, 0};
    DevBuf<uint32_t> one, dir_off;
    DevBuf<unsigned long long> list;
    DevBuf<uint8_t> blob;
    std::atomic<unsigned long long> stats[4] = {{0}, {0}, {0}, {0}};  // calls with the setting on, calls without a match, matches, sub-sentences encoded
    struct {
      DevBuf<uint32_t> cnt;
      DevBuf<unsigned long long> first, off;
      DevBuf<int32_t> tok;
      unsigned long long n_sent = 0, n_sub = 0;
      bool valid = false;
    } slot;
    AddedTable table() const { return AddedTable{{first[0], first[1], first[2], first[3]}, one, dir_off, list, blob}; }
  } add;
  // the ids the decode, the SUBWORD formatter, the ignore bitmap and the counts' default bins accept: [0, id_bound) (added_plan.h)
  uint32_t id_bound(uint32_t V) const { return added_bound(V, bfb.on.load(), add.n.load()); }
  // a free lane, locked (falls back to waiting for the caller's turn-based choice)
  // (Lane 0 last: the device-resident pair encode_device / fetch_device_result keeps its result there, unlocked, between the two
  // calls -- a host-to-host encode from another thread in between takes another lane while one is free.)
  EncodeLane &acquire(std::unique_lock<std::mutex> &lk) {
    for (int k = N_LANES - 1; k >= 0; k--) {
      lk = std::unique_lock<std::mutex>(lane[k].mu, std::try_to_lock);
      if (lk.owns_lock()) return lane[k];
    }
    EncodeLane &l = lane[N_LANES - 1 - next_lane.fetch_add(1) % N_LANES];
    lk = std::unique_lock<std::mutex>(l.mu);
    return l;
  }
};

// Start and stop events on a lane's stream for a call that reports its kernel time; does nothing when made with on == false.
struct EventPair {
  hipStream_t st;
  bool on;
  hipEvent_t a = nullptr, b = nullptr;
  EventPair(hipStream_t stream, bool enabled) : st(stream), on(enabled) {}
  EventPair(const EventPair &) = delete;
  EventPair &operator=(const EventPair &) = delete;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void start() {
    if (!on) return;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, st));
  }
  void stop(bool wait = false) {  // wait: for the stop event itself (else the caller synchronises the stream before elapsed_ms)
    if (!on) return;
    HIP_CHECK(hipEventRecord(b, st));
    if (wait) HIP_CHECK(hipEventSynchronize(b));
  }
  double elapsed_ms() const {
    float ms = 0;
    if (on) HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
  }
};

// The kernel time of an entry that runs several stages: each stage reports into its own slot (next(): null where the caller did not ask), the
// caller's *kernel_ms is 0 from the start and the sum of the stages that ran, in their order, at the end.
struct StageClock {
  double *const out;
  double slot[4] = {0, 0, 0, 0};
  int n = 0;
  explicit StageClock(double *kernel_ms) : out(kernel_ms) {
    if (out) *out = 0;
  }
  StageClock(const StageClock &) = delete;
  StageClock &operator=(const StageClock &) = delete;
  double *next() { return out ? &slot[n++] : nullptr; }
  ~StageClock() {
    if (!out) return;
    double sum = slot[0];
    for (int i = 1; i < n; i++) sum += slot[i];
    *out = sum;
  }
};

// What every device-resident entry holds while it works: the encoder's hooks bound to the thread, and lane 0 locked.
struct Lane0 {
  const CfgBind bind;
  EncodeLane &d;
  const std::lock_guard<std::mutex> lk;
  explicit Lane0(EncoderDevice &D) : bind(D.cfg), d(D.lane[0]), lk(d.mu) {}
};

// body() -> Status on `device`; a GpuError thrown inside it becomes the call's status
template <class F>
Status on_device(int device, F &&body) {
  try {
    HIP_CHECK(hipSetDevice(device));
    return body();
  } catch (const GpuError &e) {
    return Status(2, "GPU error: " + e.msg);
  }
}

// what every spans entry answers while the byte fallback is on, before any work (several ids would share one unit)
constexpr const char *SPANS_UNDER_BYTE_FALLBACK = "spans are not defined under byte fallback: switch it off (set_byte_fallback) for this call";
constexpr const char *SPANS_UNDER_ADDED_TOKENS = "spans are not defined under added tokens: clear them (set_added_tokens) for this call";
constexpr const char *SUBWORD_UNDER_ADDED_TOKENS = "SUBWORD output under added tokens needs byte fallback on as well (set_byte_fallback)";
Status check_bos_eos(const BaseEncoder &enc, bool bos, bool eos);  // bpe.cpp:1702-1707: the reference's two messages, before any work

// K5 on one lane (locked by the caller): input already in HBM, ids + offsets left in the lane's result buffers
Status encode_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_bytes, const void *d_offsets,
                      unsigned long long n_sent, unsigned long long total_bytes, unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse,
                      double dropout_prob, unsigned long long *n_ids_out, double *kernel_ms);
// counts -> offsets (exclusive scan, the total behind the last one and on the host); synchronises the lane's stream
unsigned long long scan_counts(EncodeLane &d, const uint32_t *counts, unsigned long long n, unsigned long long *off);

// SUBWORD text of the encode result pending on the lane (locked by the caller; sentence s = d_text[d_soff[s] .. d_soff[s+1]), the input that
// result was made from), left in the lane's text slot (dec) as a decode leaves its text: measure -> scan -> write (k_subword.h)
Status format_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, const void *d_soff, bool reverse,
                      unsigned long long *n_text_bytes, double *kernel_ms);

// Byte spans of the encode result pending on the lane (locked by the caller; the same d_text / d_soff as format_on_lane), left in the lane's span
// slot (sp): one pass (k_spans.h).  Ids that do not fit their text: code 2, and no spans are pending.
Status spans_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, const void *d_soff, bool reverse,
                     double *kernel_ms);

// Device decode of ids in HBM on the lane (locked by the caller), the text left in the lane's text slot: measure -> scan -> write (k_decode.h).
// n_flat: the ids the kernels walk; newline (ragged input only): a '\n' behind every sentence.  An id that is neither ignored nor valid: the
// host path's message, code 1, and no text is pending.
Status decode_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, DecInput in, unsigned long long n_flat,
                      const int32_t *ignore_ids, unsigned long long n_ignore, unsigned long long *n_bytes, double *kernel_ms, bool newline);
// The decimal text of the encode result pending on the lane (locked by the caller), left in the lane's text slot (k_idtext.h)
Status idtext_on_lane(EncodeLane &d, int device, unsigned long long *n_text_bytes, double *kernel_ms);

// ids[n_ids] in HBM counted into the encoder's counts slot (D.idc; lane 0 locked by the caller) on lane d's stream, which is synchronised
// (k_idcount.h).  n_bins: 1 .. 2^31.  accumulate on a slot of another n_bins: code 1 before anything is changed; on an empty slot it starts from 0.
Status count_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *d_ids, unsigned long long n_ids, unsigned long long n_bins, bool accumulate,
                     double *kernel_ms);

// Training blocks of ids[n_ids] / off[n_sent + 1] in HBM behind the encoder's open row, into the encoder's blocks slot (D.blk; lane 0 locked by the
// caller) on lane d's stream, which ends synchronised (k_blocks.h).  Every error is found before anything is changed: the slot and the open row
// stay.  first_line: what the message about a sentence longer than seq_len (whole mode) adds to its index, and what it calls it.
struct BlkParams {
  unsigned long long L;
  int mode;  // 0 stream, 1 whole
  int32_t pad;
  int tail;  // 0 pad, 1 keep, 2 drop
};
Status blocks_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                      unsigned long long n_ids, const BlkParams &p, const char *what, unsigned long long first_index, unsigned long long *n_rows,
                      unsigned long long *n_frags, double *kernel_ms);

// Batches by length under a token budget (k_batches.h; D.bat, lane 0 locked by the caller) on lane d's stream, which ends synchronised.
// plan_on_lane: the plan of `in`'s lengths; gather_on_lane: the planned batches of the side ids / off[n_sent + 1].  Every error is found before
// anything of the slot is changed.
struct BatParams {
  unsigned long long T, M, min_len, max_len;
};
Status plan_on_lane(EncoderDevice &D, EncodeLane &d, int device, const BatIn &in, const BatParams &p, unsigned long long *n_kept,
                    unsigned long long *n_batches, double *kernel_ms);
Status gather_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                      int32_t pad, bool left_pad, unsigned long long *n_elems, double *kernel_ms);

// The vocabulary restriction of ids[n_ids] / off[n_sent + 1] in HBM on the lane (locked by the caller; a vocabulary is set): measure -> scan ->
// write (k_restrict.h) into the lane's second pair of buffers, which then becomes the lane's encode result.  pending: the input IS that result
// (d.res); where nothing splits the write pass is skipped and the result stays where it is.  Otherwise the input is the caller's and the result
// is installed as after an encode of n_sent sentences.  *n_out: the ids of the result.
Status restrict_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                        unsigned long long n_ids, bool reverse, bool pending, unsigned long long *n_out, double *kernel_ms);

// The two-pass sequence of a kernel family that measures, then writes (k_decode.h, k_subword.h, k_idtext.h), on the lane (locked by the caller,
// on its device): launch(false) leaves n counts, scan_counts turns them into off[n + 1] and synchronises, check() may end the call there with
// its status (what launch(false) copied to the host is here), room(total) makes the output's room, launch(true) writes, and the stream is
// synchronised.  *kernel_ms (may be null): from the first launch to the last.  Returns the total in *total.  Throws GpuError.
template <class Launch, class Check, class Room>
Status two_pass_on_lane(EncodeLane &d, unsigned long long n, DevBuf<uint32_t> &counts, DevBuf<unsigned long long> &off, double *kernel_ms,
                        unsigned long long *total_out, Launch &&launch, Check &&check, Room &&room) {
  counts.grow((size_t)n);
  off.grow((size_t)n + 1);
  EventPair ev(d.st, kernel_ms != nullptr);
  ev.start();
  launch(false);
  const unsigned long long total = scan_counts(d, counts, n, off);  // (syncs)
  const Status checked = check();
  if (!checked.ok()) return checked;
  room(total);
  launch(true);
  ev.stop();
  HIP_CHECK(hipStreamSynchronize(d.st));
  if (kernel_ms) *kernel_ms = ev.elapsed_ms();
  *total_out = total;
  return Status();
}

// Host arrays of a large batch cross the link through the trainer's pinned chunks (gpu_ctx.cpp staged_transfer; 1e7 sentences are 1.3 GB up
// and 1.2 GB down: a plain copy from / to pageable memory moves them at a fraction of the link's rate, and the first touch of a freshly
// allocated result array is paid by one thread); small ones as plain copies on the lane's stream.
constexpr size_t ENC_CHUNK = 2u << 20;  // (the encoder's arrays in chunks of 2 MB: 10^7 sentences host -> host 79 -> 75 ms against 8 MB, 64 against 70 in sub-batches)
void copy_up(int device, void *d_dst, const void *src, size_t n, hipStream_t st);
void copy_down(int device, void *dst, const void *d_src, size_t n, hipStream_t st);
// A result of the lane device to device, into memory the caller owns (a framework's tensors): n_a bytes of src_a and the offsets[n_sent + 1] on
// the lane's stream, then the stream's sync; a null destination is skipped.  n_sent == 0: nothing was launched and no buffer exists, the one
// offset is 0.
Status copy_out_device(int device, EncodeLane &d, void *dst_a, const void *src_a, size_t n_a, void *dst_off, const unsigned long long *src_off,
                       unsigned long long n_sent);
void *result_alloc(size_t bytes);  // a result array the caller releases with free(); a large one in huge pages

// Items 0, 1, 2, ... through the encoder's two lanes (both locked by the caller), item i on lane i & 1, as three legs at once: upload(i) on a
// thread of its own, work(i) on the calling thread, download(i) on a third.  upload(i) starts once download(i - 2) has finished (the lane's buffers
// are free again), work(i) after upload(i), download(i) after work(i).  There are n_items items, or -- n_items == PIPE_UNTIL_EXHAUSTED -- as
// many as upload finds: it sets *exhausted where there is no item i.  Every thread binds `cfg` and sets the device; the first failure -- a
// leg's status with its code, or anything a leg throws, named after `who` -- ends all three and is returned.  *n_done: the items worked on.
constexpr size_t PIPE_UNTIL_EXHAUSTED = ~(size_t)0;
Status run_two_lanes(const char *who, const std::shared_ptr<const Config> &cfg, int device, size_t n_items,
                     const std::function<Status(size_t i, bool *exhausted)> &upload, const std::function<Status(size_t i)> &work,
                     const std::function<Status(size_t i)> &download, size_t *n_done = nullptr);

}  // namespace yttm
