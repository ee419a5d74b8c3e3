// host_core.h -- host-side (C++17) half of the drop-in: model state + file format, alphabet, the trainer's ordered
// pick, and the encoder object.  Mirrors the C++ surface declared in the reference's bpe.h / utils.h (same names,
// argument meaning and error strings) on top of the HIP kernels; nothing here computes the hot path on the CPU.
#pragma once
#include <stdint.h>

#include <memory>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace yttm {

constexpr uint32_t SPACE_TOKEN = 9601;  // utils.h:9

struct Status {  // utils.h:56-64
  int code = 0;
  std::string message;
  Status() = default;
  Status(int c, std::string m) : code(c), message(std::move(m)) {}
  bool ok() const { return code == 0; }
};

struct SpecialTokens {  // utils.h:22-43 (note the constructor order pad, unk, bos, eos)
  int pad_id = -1, unk_id = -1, bos_id = -1, eos_id = -1;
  bool taken_id(int id) const { return id == unk_id || id == pad_id || id == bos_id || id == eos_id; }
  uint64_t n_special_tokens() const { return (unk_id != -1) + (pad_id != -1) + (bos_id != -1) + (eos_id != -1); }
};

struct BpeConfig {  // utils.h:45-54
  double character_coverage = 1;
  int n_threads = 0;
  SpecialTokens special_tokens;
};

struct BPE_Rule {  // utils.h:11-20
  uint32_t x = 0, y = 0, z = 0;
};

struct BPEState {  // utils.h:66-74; chars are kept in MODEL-FILE order (the reference's hash-slot order)
  std::vector<std::pair<uint32_t, uint32_t>> char2id;  // (code point, id)
  std::vector<BPE_Rule> rules;
  SpecialTokens special_tokens;
  Status dump(const std::string &file_name) const;  // utils.cpp:50-66
  Status load(const std::string &file_name);        // utils.cpp:68-91
};

// Slot order of a ska::flat_hash_map<uint32_t,...> after inserting `keys` in order into an empty map and
// copy-constructing it once (bpe.cpp:1289 copies char2id into BPEState; utils.cpp:57-59 iterates the copy).
std::vector<uint32_t> flat_hash_map_order(const std::vector<uint32_t> &keys);

// bpe.cpp:316-355 compute_alphabet_helper.  Returns chars in INSERTION order (▁ first, then by descending
// (count, code point)) with compact ids n_special, n_special+1, ...
void compute_alphabet(const std::vector<uint32_t> &cps, const std::vector<unsigned long long> &cnts, unsigned long long data_len,
                      const BpeConfig &cfg, std::vector<std::pair<uint32_t, uint32_t>> &char2id_insertion, uint64_t &n_removed);

Status check_config(BpeConfig &cfg, int vocab_size);  // bpe.cpp:1295-1350

struct TrainReport {
  double seconds_total = 0, seconds_frontend = 0, seconds_merge = 0, seconds_io = 0, seconds_upload = 0;  // upload: file/host -> HBM (train_bpe only)
  unsigned long long corpus_bytes = 0, n_unique = 0, n_tokens = 0, rounds = 0, rules = 0, cand_rescans = 0, repacks = 0, merge_sites = 0, hot_rebuilds = 0, fused_rounds = 0, fused_overflows = 0, exchange_retries = 0, word_table_retries = 0, front_end_overlapped = 0, top_refills = 0, index_builds = 0, index_radix_builds = 0, word_rounds = 0, word_switch_round = 0, word_all_rounds = 0, word_fused_rounds = 0,
                     rounds_exhausted = 0 /* batches closed for lack of candidates, not at an intersection */, batch_extensions = 0 /* extra scans that refilled the pick */, batch_splits = 0 /* batches cut to the first BATCH_ARGS_MAX rules: word mode, two one-launch rounds instead of a four-launch one */,
                     classb_word_rounds = 0 /* word-mode rounds that launched class-B tiles */, k3_radix = 0 /* 1: the pair count of a large alphabet ran by radix partition */, front_end_chunks = 0 /* > 0: the corpus crossed the device in this many chunks (it did not fit the HBM at once) */, peak_device_bytes = 0 /* high-water mark of the device memory pool during the call */,
                     replicated_merge_loop = 0 /* multi-GPU: the shards were gathered, every rank ran the merge loop alone (no per-round collective) */;
  // K4 totals: tiles with a merge site and their tokens; words with a merge site and their tokens (measurement pass only, else 0)
  unsigned long long touched_tiles = 0, touched_tile_tokens = 0, touched_words = 0, touched_word_tokens = 0;
  // ... the same after `split_round` rounds (YTTM_MEASURE_SPLIT_ROUND; 0: none), and the device-clock time of the word-mode rounds
  unsigned long long split_round = 0, split_touched_words = 0, split_touched_word_tokens = 0, split_sites = 0, merge_launches_words = 0;
  double merge_ms_words = 0;
  // per kernel family: ms, launches, algorithmic bytes (gpu_ctx.h KT_*)
  double kt_ms[8] = {0};
  unsigned long long kt_launches[8] = {0}, kt_bytes[8] = {0};
};

class GpuCtx;
struct Comm;

// bpe.h:19 train_bpe -- file based.  `device` = HIP device ordinal.
Status train_bpe(const std::string &input_path, const std::string &model_path, int vocab_size, BpeConfig cfg, int device = 0,
                 TrainReport *report = nullptr, Comm *comm = nullptr, int profile = 0 /* 1: per-kernel timers in the report */);
// same, corpus already in host memory / already resident in HBM (bench: timed region starts with the bytes in HBM)
Status train_bpe_from_memory(const uint8_t *text, unsigned long long n, const std::string &model_path, int vocab_size, BpeConfig cfg,
                             int device = 0, TrainReport *report = nullptr, Comm *comm = nullptr);
Status train_bpe_from_device(const void *d_text, unsigned long long n, const std::string &model_path, int vocab_size, BpeConfig cfg,
                             int device = 0, TrainReport *report = nullptr, Comm *comm = nullptr, int profile = 0 /* 1: HIP-event kernel times; 2: K4 measurement pass (touched words), never timed */);
// learn_bpe_from_string (bpe.cpp:859-1293) on an attached corpus
Status learn_bpe(GpuCtx &g, int vocab_size, const std::string &model_path, const BpeConfig &cfg, BPEState *state, TrainReport *report);

struct EncoderDevice;  // HBM-resident model tables for K5
struct Config;         // yttm_config.h

class BaseEncoder {  // bpe.h:22-82
 public:
  BPEState bpe_state;
  std::unordered_map<uint32_t, uint32_t> char2id, id2char;
  std::unordered_map<uint32_t, std::vector<uint32_t>> recipe;
  std::unordered_map<std::string, uint32_t> reversed_recipe;
  int n_threads = 1;

  BaseEncoder(const std::string &model_path, int n_threads, Status *ret_status, int device = 0);
  ~BaseEncoder();

  // packed batch API (bytes + offsets[S+1]); ids/out_off are filled on the host
  Status encode_as_ids(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos, bool reverse,
                       double dropout_prob, std::vector<int32_t> *ids, std::vector<unsigned long long> *out_off) const;
  Status encode_as_ids_malloc(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos, bool reverse,
                              double dropout_prob, int32_t **ids, unsigned long long **out_off) const;
  Status encode_as_subwords(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos,
                            bool reverse, double dropout_prob, std::vector<std::string> *pieces,
                            std::vector<unsigned long long> *piece_off) const;
  // device-resident variant used by bench.py: input already in HBM, output left in HBM (ids_dev/off_dev owned by the encoder)
  Status encode_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                       unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                       unsigned long long *n_ids_out, double *kernel_ms) const;
  Status fetch_device_result(int32_t *ids, unsigned long long *out_off, unsigned long long n_sent) const;
  // device decode (host_decode.cpp, k_decode.h): ids + offsets (or a padded matrix) already in HBM, the text left in HBM in lane 0 next to the
  // encode result; ignore_ids is a host array.  replaces decode(), bpe.h:52-54, bpe.cpp:1828-1861, for a batch
  Status decode_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, const int32_t *ignore_ids,
                       unsigned long long n_ignore, unsigned long long *n_bytes, double *kernel_ms) const;
  Status decode_device_padded(const void *d_ids, unsigned long long n_sent, unsigned long long width, unsigned long long row_stride, const void *d_lengths,
                              const int32_t *ignore_ids, unsigned long long n_ignore, unsigned long long *n_bytes, double *kernel_ms) const;
  Status fetch_decode_result(char *bytes, unsigned long long *out_off, unsigned long long n_sent) const;      // device to host
  Status copy_decode_result(void *d_bytes, void *d_out_off, unsigned long long n_sent) const;                 // device to device
  // the result of the last encode_device, device to device: ragged, or as a padded matrix + lengths (k_enc_pad)
  Status copy_encode_result(void *d_ids, void *d_out_off, unsigned long long n_sent) const;
  Status copy_encode_padded(void *d_matrix, void *d_lengths, unsigned long long n_sent, unsigned long long width, int32_t pad_value,
                            unsigned long long *longest) const;
  // text that is not cut into sentences yet (host_lines.cpp, k_lines.h): its lines by std::getline's rules, found on the device.  lines_device leaves
  // uint64 offsets[n_lines + 1] (line i WITH its newline) in lane 0, beside a pending encode / decode result; take_lines copies them out.
  Status lines_device(const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines, unsigned long long *longest, double *kernel_ms) const;
  Status take_lines(void *offsets, unsigned long long n_lines, bool to_device) const;
  // split + encode_device: the result is pending as after encode_device (n_sent = *n_lines)
  Status encode_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                            unsigned long long *n_lines, unsigned long long *n_ids, double *kernel_ms) const;
  // a file of any size in pieces through both lanes; out_prefix: PREFIX.ids / PREFIX.off instead of malloc'ed arrays
  Status encode_file(const std::string &path, const char *out_prefix, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long piece_bytes,
                     int32_t **ids, unsigned long long **out_off, unsigned long long *n_lines, unsigned long long *n_ids, std::string *report) const;
  // SUBWORD output on the device (host_decode.cpp, host_lines.cpp, k_subword.h): encode_device / encode_text_device / encode_file, then the text
  // `yttm encode --output_type subword` prints -- every piece followed by a space, '\n' per sentence -- left in lane 0's text slot (taken with
  // fetch_decode_result / copy_decode_result: it replaces a pending decode result), the ids pending as after encode_device.
  // replaces encode_as_subwords, bpe.h:41-46, bpe.cpp:1757, :1597-1613, and the formatting of encode_cli, bpe.cpp:1942-2014
  Status subword_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                        unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long *n_ids,
                        unsigned long long *n_text_bytes, double *kernel_ms) const;
  Status subword_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                             unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes, double *kernel_ms) const;
  Status encode_file_subword(const std::string &path, const std::string &out_path, bool bos, bool eos, bool reverse, double dropout_prob,
                             unsigned long long piece_bytes, unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes,
                             std::string *report) const;
  // Decimal id text on the device (host_lines.cpp, host_decode.cpp, k_idtext.h), the format `yttm encode --output_type id` prints and `yttm decode`
  // reads.  ids_parse_device: split + the ids `while (ss >> x)` reads from every line (bpe.cpp:1863-1873), pending as after encode_device with
  // n_sent = *n_lines; decode_text_device: the same, then the device decode of those ids with a '\n' behind every line (decode_cli,
  // bpe.cpp:2016-2028), the text in lane 0's text slot; decode_file: a file of such text -> the file `yttm decode` prints, through both lanes;
  // idtext_device: the pending encode result -> its decimal text (utils.h:92-103) in the text slot; encode_file_idtext: encode_file_subword with
  // that printer in place of the SUBWORD formatter.
  Status ids_parse_device(const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines, unsigned long long *n_ids, double *kernel_ms) const;
  Status decode_text_device(const void *d_text, unsigned long long n_bytes, const int32_t *ignore_ids, unsigned long long n_ignore,
                            unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes, double *kernel_ms) const;
  Status decode_file(const std::string &path, const std::string &out_path, const int32_t *ignore_ids, unsigned long long n_ignore,
                     unsigned long long piece_bytes, unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes,
                     std::string *report) const;
  Status idtext_device(unsigned long long n_sent, unsigned long long *n_text_bytes, double *kernel_ms) const;
  Status encode_file_idtext(const std::string &path, const std::string &out_path, bool bos, bool eos, bool reverse, double dropout_prob,
                            unsigned long long piece_bytes, unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes,
                            std::string *report) const;
  // Byte spans on the device (host_decode.cpp, host_lines.cpp, k_spans.h): encode_device / encode_text_device, then for every id the bytes of
  // its sentence it stands for, uint32 [n_ids][2] relative to the sentence's first byte (on the text route: the line's), in lane 0's span slot; the
  // ids are pending as after encode_device.  The slot holds the spans of the ids pending beside it: any later encode on the lane empties it, and
  // taking spans that are not there is code 1.
  Status spans_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                      unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long *n_ids,
                      double *kernel_ms) const;
  Status spans_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                           unsigned long long *n_lines, unsigned long long *n_ids, double *kernel_ms) const;
  Status take_spans(void *spans, unsigned long long n_sent, bool to_device) const;  // ragged [n_ids][2]: to a host array or device to device
  Status copy_spans_padded(void *d_matrix, unsigned long long n_sent, unsigned long long width, unsigned long long *longest) const;  // [n_sent, width, 2]
  Status encode_as_ids_spans(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos, bool reverse,
                             double dropout_prob, int32_t **ids, unsigned long long **out_off, uint32_t **spans) const;  // host to host, free()
  // Token frequencies on the device (host_decode.cpp, host_lines.cpp, k_idcount.h): uint64 counts[n_bins + 1] (n_bins == 0: vocab_size()) of the
  // pending encode result or of any int32 array in HBM, in a slot of the encoder's own that only a count changes; counts[n_bins] holds the ids
  // outside [0, n_bins).  What is counted is only read: a pending result stays pending.  encode_file_counts: the pipeline of encode_file with the
  // count in place of the download; the caller's counts[vocab_size() + 1] is all that comes down.
  Status id_counts_device(unsigned long long n_sent, unsigned long long n_bins, bool accumulate, unsigned long long *n_counted, double *kernel_ms) const;
  Status id_counts_ids_device(const void *d_ids, unsigned long long n_ids, unsigned long long n_bins, bool accumulate, double *kernel_ms) const;
  Status take_id_counts(void *counts, unsigned long long n_bins, bool to_device) const;  // [n_bins + 1]: to a host array or device to device
  Status encode_file_counts(const std::string &path, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long piece_bytes,
                            unsigned long long *counts, unsigned long long *n_lines, unsigned long long *n_ids, std::string *report) const;
  // Training blocks on the device (host_decode.cpp, host_lines.cpp, k_blocks.h; the rule is in include/yttm_mi355x.h): the pending encode result, or
  // any ids + offsets in HBM, behind the encoder's open row, packed into rows of exactly seq_len ids with segment numbers, positions and the list
  // of fragments, in a slot of the encoder's own that only the next blocks call replaces.  What is packed is only read.  mode: 0 stream, 1 whole;
  // tail: 0 pad, 1 keep (the incomplete row becomes the open row), 2 drop.  blocks_open: {ids in the open row, its seq_len, its mode};
  // blocks_discard empties the open row.  take_blocks: the five arrays to host arrays or device to device, a null pointer is skipped.
  // encode_file_blocks: the pipeline of encode_file, every piece packed with tail = keep and written to PREFIX.rows / PREFIX.frags.
  Status blocks_device(unsigned long long n_sent, unsigned long long seq_len, int mode, int32_t pad_value, int tail, unsigned long long *n_rows,
                       unsigned long long *n_frags, double *kernel_ms) const;
  Status blocks_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, unsigned long long seq_len, int mode,
                           int32_t pad_value, int tail, unsigned long long *n_rows, unsigned long long *n_frags, double *kernel_ms) const;
  Status blocks_flush(int32_t pad_value, unsigned long long *n_rows, unsigned long long *n_frags, double *kernel_ms) const;
  void blocks_open(unsigned long long out[3]) const;
  void blocks_discard() const;
  Status take_blocks(void *rows, void *seg, void *pos, void *frags, void *row_frags, unsigned long long n_rows, unsigned long long n_frags,
                     bool to_device) const;
  Status encode_file_blocks(const std::string &path, const std::string &out_prefix, bool bos, bool eos, bool reverse, double dropout_prob,
                            unsigned long long piece_bytes, unsigned long long seq_len, int mode, int32_t pad_value, int tail, unsigned long long *n_rows,
                            unsigned long long *n_frags, unsigned long long *n_lines, unsigned long long *n_ids, std::string *report) const;
  // Batches by length under a token budget on the device (host_decode.cpp, k_batches.h; the rule is in include/yttm_mi355x.h): the plan (a stable
  // order of the sentences by length and its greedy cuts) from the pending encode result's offsets or from int32 lengths in HBM, and the gather of
  // the planned batches of one side (the pending result, or any ids + offsets in HBM) into padded matrices, both in a slot of the encoder's own:
  // a plan call replaces the plan and empties the gathered part, a gather replaces the gathered part.  take_batches: the five arrays to host
  // arrays or device to device, a null pointer is skipped.
  Status batches_plan_device(unsigned long long n_sent, unsigned long long max_tokens, unsigned long long max_sentences, unsigned long long min_len,
                             unsigned long long max_len, unsigned long long *n_kept, unsigned long long *n_batches, double *kernel_ms) const;
  Status batches_plan_lengths_device(const void *d_lengths, unsigned long long n_sent, unsigned long long max_tokens, unsigned long long max_sentences,
                                     unsigned long long min_len, unsigned long long max_len, unsigned long long *n_kept, unsigned long long *n_batches,
                                     double *kernel_ms) const;
  Status batches_gather_device(unsigned long long n_sent, int32_t pad_value, bool left_pad, unsigned long long *n_elems, double *kernel_ms) const;
  Status batches_gather_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, int32_t pad_value,
                                   bool left_pad, unsigned long long *n_elems, double *kernel_ms) const;
  Status take_batches(void *order, void *batch_first, void *widths, void *batch_off, void *out, unsigned long long n_sent, unsigned long long n_batches,
                      unsigned long long n_elems, bool to_device) const;
  // Encode under a restricted vocabulary (host_encoder.cpp, k_restrict.h; the rule is in include/yttm_mi355x.h): allowed[vocab_size()] (null:
  // clears it) -> the expansion tables in HBM; from then on every encode on this encoder leaves restricted ids.  info (optional): allowed ids,
  // ids that split, the longest expansion.  vocabulary_stats: restricted calls, calls where nothing split, ids in, ids out.
  // restrict_ids_device: the pass over ids + offsets in HBM that the encoder did not make; the result is pending as after encode_device.
  Status set_vocabulary(const uint8_t *allowed, unsigned long long n, unsigned long long *info) const;
  void vocabulary_stats(unsigned long long out[4]) const;
  Status restrict_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, bool reverse,
                             unsigned long long *n_out, double *kernel_ms) const;
  // Byte fallback (host_encoder.cpp, k_bytefb.h; the rule is in include/yttm_mi355x.h): a setting of the encoder.  On: every encode leaves the
  // bytes of an unknown run as the ids vocab_size() + b in place of the run's unk_id, and the decode, the names, the SUBWORD pieces and the
  // counts know the ids [vocab_size(), vocab_size() + 256).  byte_fallback_stats: calls of the pass, calls whose write pass was skipped, ids in,
  // ids out.  byte_fallback_ids_device: the pass over ids + offsets and the text they were made from, all in HBM, that the encoder did not make;
  // the result is pending as after encode_device.
  Status set_byte_fallback(bool on) const;
  bool byte_fallback() const;
  void byte_fallback_stats(unsigned long long out[4]) const;
  Status byte_fallback_ids_device(const void *d_ids, const void *d_id_offsets, const void *d_bytes, const void *d_text_offsets, unsigned long long n_sent,
                                  unsigned long long n_ids, unsigned long long total_bytes, bool reverse, unsigned long long *n_out, double *kernel_ms) const;
  // Added tokens (host_encoder.cpp, k_added.h; the rule is in include/yttm_mi355x.h): a setting of the encoder.  n byte strings as a blob plus
  // offsets[n + 1]; token k is the id vocab_size() + 256 + k, matched in every batch's text, never split.  blob == nullptr clears the setting.
  // added_tokens: a copy of the set in the caller's order.  added_tokens_stats: calls with the setting on, calls without a match, matches,
  // sub-sentences encoded.  added_split_device: the stand-alone split of a text in HBM into the encoder's own slot, taken with take_added_split.
  // id_bound / default_bins: the ids the decode, the names and the counts know under the settings as they stand.
  Status set_added_tokens(const uint8_t *blob, const unsigned long long *tok_offsets, unsigned long long n) const;
  unsigned long long n_added_tokens() const;
  std::vector<std::string> added_tokens() const;
  void added_tokens_stats(unsigned long long out[4]) const;
  Status added_split_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes, unsigned long long *n_sub,
                            unsigned long long *n_matches, double *kernel_ms) const;
  Status take_added_split(void *sub_first, void *sub_off, void *tok, unsigned long long n_sent, unsigned long long n_sub, bool to_device) const;
  unsigned long long id_bound() const;
  unsigned long long default_bins() const { return id_bound(); }
  // the YTTM_* hooks as they stood when THIS encoder was made: every entry point binds them to its thread (yttm_config.h CfgBind), so that a
  // later encoder or training never changes the paths of this one
  std::shared_ptr<const Config> config() const;
  void set_cache(int mode, unsigned long long min_bytes) const;  // word cache of the batch encoder: 0 off, 1 always, 2 from min_bytes up
  unsigned long long cache_words() const;                          // distinct words of the last encode_device batch (0: not cached)

  Status id_to_subword(int id, std::string *subword, bool replace_space = false) const;  // bpe.cpp:1774-1807
  int subword_to_id(const std::string &token) const;                                      // bpe.cpp:1809-1826
  Status decode(const std::vector<int> &ids, std::string *sentence, const std::unordered_set<int> *ignore_ids) const;  // bpe.cpp:1843
  int vocab_size() const;                                                                 // bpe.cpp:1692
  std::vector<std::string> vocabulary() const;                                            // bpe.cpp:1884
  // the streaming loops of the `yttm` command line (host_cli.cpp); the reference's read std::cin and write std::cout
  Status encode_cli(const std::string &output_type, bool stream, bool bos, bool eos, bool reverse, double dropout_prob, int in_fd = 0,
                    int out_fd = 1) const;                                                // bpe.h:66-68, bpe.cpp:1942-2014
  Status decode_cli(const std::unordered_set<int> *ignore_ids, int in_fd = 0, int out_fd = 1) const;  // bpe.h:70, bpe.cpp:2016-2028
  Status vocab_cli(bool verbose, int out_fd = 1) const;                                   // bpe.h:71, bpe.cpp:1896-1940

 private:
  void fill_from_state();  // bpe.cpp:1667-1690
  EncoderDevice *dev_ = nullptr;
  int device_ = 0;
};

std::string encode_utf8(const std::vector<uint32_t> &text);  // utf8.cpp:102-109
std::vector<uint32_t> decode_utf8(const char *begin, const char *end, bool *invalid = nullptr);  // utf8.cpp:111-128
bool is_space(uint32_t ch);  // utils.cpp:99-101

}  // namespace yttm
