// capi.cpp -- extern "C" entry points declared in include/yttm_mi355x.h (drop-in boundary) and include/yttm_gpu.h
// (kernel stages).  Thin marshalling only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/yttm_gpu.h"
#include "../../include/yttm_mi355x.h"
#include "gpu_ctx.h"
#include "host_core.h"

using namespace yttm;

static void put_err(char *err, int errlen, const std::string &m) {
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", m.c_str());
}
static int finish(const Status &s, char *err, int errlen) {
  if (!s.ok()) put_err(err, errlen, s.message);
  return s.code;
}
static BpeConfig make_cfg(double coverage, int n_threads, int pad, int unk, int bos, int eos) {
  BpeConfig c;
  c.character_coverage = coverage;
  c.n_threads = n_threads;
  c.special_tokens.pad_id = pad;
  c.special_tokens.unk_id = unk;
  c.special_tokens.bos_id = bos;
  c.special_tokens.eos_id = eos;
  return c;
}
void yttm_report_to_json(const TrainReport &r, char *buf, int len) {
  if (!buf || len <= 0) return;
  static const char *names[8] = {"char_hist", "segments", "dedup", "build", "pair_count", "merge_apply", "cand_scan", "exchange"};
  std::string s = "{";
  char tmp[1280];
  snprintf(tmp, sizeof tmp, "\"seconds_total\": %.6f, \"seconds_upload\": %.6f, \"seconds_frontend\": %.6f, \"seconds_merge\": %.6f, \"seconds_io\": %.6f, ", r.seconds_total,
           r.seconds_upload, r.seconds_frontend, r.seconds_merge, r.seconds_io);
  s += tmp;
  snprintf(tmp, sizeof tmp, "\"corpus_bytes\": %llu, \"n_unique\": %llu, \"n_tokens\": %llu, \"rounds\": %llu, \"rules\": %llu, \"cand_rescans\": %llu, \"hot_rebuilds\": %llu, \"repacks\": %llu, \"merge_sites\": %llu, ",
           r.corpus_bytes, r.n_unique, r.n_tokens, r.rounds, r.rules, r.cand_rescans, r.hot_rebuilds, r.repacks, r.merge_sites);
  s += tmp;
  snprintf(tmp, sizeof tmp, "\"fused_rounds\": %llu, \"fused_overflows\": %llu, \"exchange_retries\": %llu, \"word_table_retries\": %llu, \"front_end_overlapped\": %llu, \"top_refills\": %llu, \"index_builds\": %llu, \"index_radix_builds\": %llu, \"word_rounds\": %llu, \"word_switch_round\": %llu, \"word_all_rounds\": %llu, \"word_fused_rounds\": %llu, \"rounds_exhausted\": %llu, \"batch_extensions\": %llu, \"batch_splits\": %llu, \"replicated_merge_loop\": %llu, \"front_end_chunks\": %llu, \"peak_device_bytes\": %llu, \"classb_word_rounds\": %llu, \"k3_radix\": %llu, ",
           r.fused_rounds, r.fused_overflows, r.exchange_retries, r.word_table_retries, r.front_end_overlapped, r.top_refills, r.index_builds, r.index_radix_builds, r.word_rounds, r.word_switch_round, r.word_all_rounds, r.word_fused_rounds, r.rounds_exhausted, r.batch_extensions, r.batch_splits, r.replicated_merge_loop, r.front_end_chunks, r.peak_device_bytes, r.classb_word_rounds, r.k3_radix);
  s += tmp;
  snprintf(tmp, sizeof tmp, "\"touched_tiles\": %llu, \"touched_tile_tokens\": %llu, \"touched_words\": %llu, \"touched_word_tokens\": %llu, ",
           r.touched_tiles, r.touched_tile_tokens, r.touched_words, r.touched_word_tokens);
  s += tmp;
  snprintf(tmp, sizeof tmp, "\"split_round\": %llu, \"split_sites\": %llu, \"split_touched_words\": %llu, \"split_touched_word_tokens\": %llu, \"merge_ms_word_rounds\": %.6f, \"merge_launches_word_rounds\": %llu, ",
           r.split_round, r.split_sites, r.split_touched_words, r.split_touched_word_tokens, r.merge_ms_words, r.merge_launches_words);
  s += tmp;
  s += "\"kernels\": {";
  for (int i = 0; i < 8; i++) {
    snprintf(tmp, sizeof tmp, "%s\"%s\": {\"ms\": %.6f, \"launches\": %llu, \"bytes\": %llu}", i ? ", " : "", names[i], r.kt_ms[i], r.kt_launches[i],
             r.kt_bytes[i]);
    s += tmp;
  }
  s += "}}";
  snprintf(buf, (size_t)len, "%s", s.c_str());
}

template <class T>
static T *to_malloc(const std::vector<T> &v) {
  T *p = (T *)malloc((v.size() ? v.size() : 1) * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

extern "C" {

// ------------------------------------------------------------------------------------------------- outer ABI
int yttm_train_bpe(const char *input_path, const char *model_path, int vocab_size, double coverage, int n_threads, int pad_id, int unk_id,
                   int bos_id, int eos_id, char *err, int errlen) {
  return finish(train_bpe(input_path, model_path, vocab_size, make_cfg(coverage, n_threads, pad_id, unk_id, bos_id, eos_id)), err, errlen);
}

int yttm_train_bpe_ex(const char *input_path, const char *model_path, int vocab_size, double coverage, int n_threads, int pad_id, int unk_id,
                      int bos_id, int eos_id, int device, char *report_json, int report_len, char *err, int errlen) {
  TrainReport rep;
  Status s = train_bpe(input_path, model_path, vocab_size, make_cfg(coverage, n_threads, pad_id, unk_id, bos_id, eos_id), device, &rep);
  if (s.ok()) yttm_report_to_json(rep, report_json, report_len);
  return finish(s, err, errlen);
}

int yttm_train_bpe_from_memory(const uint8_t *text, uint64_t n, const char *model_path, int vocab_size, double coverage, int pad_id,
                               int unk_id, int bos_id, int eos_id, int device, char *report_json, int report_len, char *err, int errlen) {
  TrainReport rep;
  Status s = train_bpe_from_memory(text, n, model_path ? model_path : "", vocab_size, make_cfg(coverage, 1, pad_id, unk_id, bos_id, eos_id), device, &rep);
  if (s.ok()) yttm_report_to_json(rep, report_json, report_len);
  return finish(s, err, errlen);
}

int yttm_train_bpe_from_device(const void *d_text, uint64_t n, const char *model_path, int vocab_size, double coverage, int pad_id, int unk_id,
                               int bos_id, int eos_id, int device, int profile, char *report_json, int report_len, char *err, int errlen) {
  TrainReport rep;
  Status s = train_bpe_from_device(d_text, n, model_path ? model_path : "", vocab_size, make_cfg(coverage, 1, pad_id, unk_id, bos_id, eos_id), device,
                                   &rep, nullptr, profile);
  if (s.ok()) yttm_report_to_json(rep, report_json, report_len);
  return finish(s, err, errlen);
}

struct yttm_encoder {
  BaseEncoder *enc;
};

int yttm_encoder_create(const char *model_path, int n_threads, int device, yttm_encoder **out, char *err, int errlen) {
  Status st;
  BaseEncoder *e = new BaseEncoder(model_path, n_threads, &st, device);
  if (!st.ok()) {
    delete e;
    *out = nullptr;
    return finish(st, err, errlen);
  }
  *out = new yttm_encoder{e};
  return 0;
}
void yttm_encoder_destroy(yttm_encoder *h) {
  if (!h) return;
  delete h->enc;
  delete h;
}

int yttm_encode_as_ids(yttm_encoder *h, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos, int eos, int reverse,
                       double dropout_prob, int32_t **ids, uint64_t **out_offsets, char *err, int errlen) {
  unsigned long long *off = nullptr;
  Status s = h->enc->encode_as_ids_malloc(bytes, (const unsigned long long *)offsets, n_sent, bos, eos, reverse, dropout_prob, ids, &off);
  if (!s.ok()) return finish(s, err, errlen);
  *out_offsets = (uint64_t *)off;
  return 0;
}

static void pack_strings(const std::vector<std::string> &v, char **blob, uint64_t **off) {
  size_t total = 0;
  for (auto &s : v) total += s.size();
  char *b = (char *)malloc(total + 1);
  uint64_t *o = (uint64_t *)malloc((v.size() + 1) * sizeof(uint64_t));
  size_t p = 0;
  for (size_t i = 0; i < v.size(); i++) {
    o[i] = p;
    memcpy(b + p, v[i].data(), v[i].size());
    p += v[i].size();
  }
  o[v.size()] = p;
  b[p] = 0;
  *blob = b;
  *off = o;
}

int yttm_encode_as_subwords(yttm_encoder *h, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos, int eos, int reverse,
                            double dropout_prob, char **blob, uint64_t **piece_off, uint64_t *n_pieces, uint64_t **sent_off, char *err,
                            int errlen) {
  std::vector<std::string> pieces;
  std::vector<unsigned long long> so;
  Status s = h->enc->encode_as_subwords(bytes, (const unsigned long long *)offsets, n_sent, bos, eos, reverse, dropout_prob, &pieces, &so);
  if (!s.ok()) return finish(s, err, errlen);
  pack_strings(pieces, blob, piece_off);
  *n_pieces = pieces.size();
  *sent_off = (uint64_t *)to_malloc(so);
  return 0;
}

int yttm_encode_device(yttm_encoder *h, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes,
                       uint64_t max_sentence_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_ids, double *kernel_ms,
                       char *err, int errlen) {
  unsigned long long n = 0;
  Status s = h->enc->encode_device(d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, &n, kernel_ms);
  if (n_ids) *n_ids = n;
  return finish(s, err, errlen);
}
int yttm_encode_fetch(yttm_encoder *h, int32_t *ids, uint64_t *out_offsets, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->fetch_device_result(ids, (unsigned long long *)out_offsets, n_sent), err, errlen);
}

int yttm_encode_copy_device(yttm_encoder *h, void *d_ids, void *d_out_offsets, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->copy_encode_result(d_ids, d_out_offsets, n_sent), err, errlen);
}
int yttm_encode_copy_padded(yttm_encoder *h, void *d_matrix, void *d_lengths, uint64_t n_sent, uint64_t width, int32_t pad_value, uint64_t *longest,
                            char *err, int errlen) {
  unsigned long long need = 0;
  Status s = h->enc->copy_encode_padded(d_matrix, d_lengths, n_sent, width, pad_value, &need);
  if (longest) *longest = need;
  return finish(s, err, errlen);
}
int yttm_decode_device(yttm_encoder *h, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, const int32_t *ignore_ids,
                       uint64_t n_ignore, uint64_t *n_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long n = 0;
  Status s = h->enc->decode_device(d_ids, d_offsets, n_sent, n_ids, ignore_ids, n_ignore, &n, kernel_ms);
  if (n_bytes) *n_bytes = n;
  return finish(s, err, errlen);
}
int yttm_decode_device_padded(yttm_encoder *h, const void *d_ids, uint64_t n_sent, uint64_t width, uint64_t row_stride, const void *d_lengths,
                              const int32_t *ignore_ids, uint64_t n_ignore, uint64_t *n_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long n = 0;
  Status s = h->enc->decode_device_padded(d_ids, n_sent, width, row_stride, d_lengths, ignore_ids, n_ignore, &n, kernel_ms);
  if (n_bytes) *n_bytes = n;
  return finish(s, err, errlen);
}
int yttm_decode_fetch(yttm_encoder *h, char *bytes, uint64_t *out_offsets, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->fetch_decode_result(bytes, (unsigned long long *)out_offsets, n_sent), err, errlen);
}
int yttm_decode_copy_device(yttm_encoder *h, void *d_bytes, void *d_out_offsets, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->copy_decode_result(d_bytes, d_out_offsets, n_sent), err, errlen);
}

int yttm_lines_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, uint64_t *n_lines, uint64_t *longest, double *kernel_ms, char *err, int errlen) {
  unsigned long long n = 0, m = 0;
  Status s = h->enc->lines_device(d_text, n_bytes, &n, &m, kernel_ms);
  if (n_lines) *n_lines = n;
  if (longest) *longest = m;
  return finish(s, err, errlen);
}
int yttm_lines_copy_device(yttm_encoder *h, void *d_offsets, uint64_t n_lines, char *err, int errlen) {
  return finish(h->enc->take_lines(d_offsets, n_lines, true), err, errlen);
}
int yttm_lines_fetch(yttm_encoder *h, uint64_t *offsets, uint64_t n_lines, char *err, int errlen) {
  return finish(h->enc->take_lines(offsets, n_lines, false), err, errlen);
}
int yttm_encode_text_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_lines,
                            uint64_t *n_ids, double *kernel_ms, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0;
  Status s = h->enc->encode_text_device(d_text, n_bytes, bos, eos, reverse, dropout_prob, &nl, &ni, kernel_ms);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  return finish(s, err, errlen);
}
int yttm_encode_file(yttm_encoder *h, const char *path, const char *out_prefix, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes,
                     int32_t **ids, uint64_t **offsets, uint64_t *n_lines, uint64_t *n_ids, char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, *off = nullptr;
  int32_t *idp = nullptr;
  std::string report;
  Status s = h->enc->encode_file(path ? path : "", out_prefix, bos, eos, reverse, dropout_prob, chunk_bytes, out_prefix ? nullptr : &idp, out_prefix ? nullptr : &off,
                                 &nl, &ni, &report);
  if (ids) *ids = idp;
  else free(idp);
  if (offsets) *offsets = (uint64_t *)off;
  else free(off);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return finish(s, err, errlen);
}

int yttm_subword_device(yttm_encoder *h, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes, uint64_t max_sentence_bytes, int bos,
                        int eos, int reverse, double dropout_prob, uint64_t *n_ids, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long ni = 0, nt = 0;
  Status s = h->enc->subword_device(d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, &ni, &nt, kernel_ms);
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  return finish(s, err, errlen);
}
int yttm_subword_text_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_lines,
                             uint64_t *n_ids, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, nt = 0;
  Status s = h->enc->subword_text_device(d_text, n_bytes, bos, eos, reverse, dropout_prob, &nl, &ni, &nt, kernel_ms);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  return finish(s, err, errlen);
}
int yttm_encode_file_subword(yttm_encoder *h, const char *path, const char *out_path, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes,
                             uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, nt = 0;
  std::string report;
  Status s = h->enc->encode_file_subword(path ? path : "", out_path ? out_path : "", bos, eos, reverse, dropout_prob, chunk_bytes, &nl, &ni, &nt, &report);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return finish(s, err, errlen);
}

int yttm_ids_parse_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, uint64_t *n_lines, uint64_t *n_ids, double *kernel_ms, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0;
  Status s = h->enc->ids_parse_device(d_text, n_bytes, &nl, &ni, kernel_ms);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  return finish(s, err, errlen);
}
int yttm_decode_text_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, const int32_t *ignore_ids, uint64_t n_ignore, uint64_t *n_lines,
                            uint64_t *n_ids, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, nt = 0;
  Status s = h->enc->decode_text_device(d_text, n_bytes, ignore_ids, n_ignore, &nl, &ni, &nt, kernel_ms);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  return finish(s, err, errlen);
}
int yttm_decode_file(yttm_encoder *h, const char *path, const char *out_path, const int32_t *ignore_ids, uint64_t n_ignore, uint64_t chunk_bytes,
                     uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, nt = 0;
  std::string report;
  Status s = h->enc->decode_file(path ? path : "", out_path ? out_path : "", ignore_ids, n_ignore, chunk_bytes, &nl, &ni, &nt, &report);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return finish(s, err, errlen);
}
int yttm_idtext_device(yttm_encoder *h, uint64_t n_sent, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen) {
  unsigned long long nt = 0;
  Status s = h->enc->idtext_device(n_sent, &nt, kernel_ms);
  if (n_text_bytes) *n_text_bytes = nt;
  return finish(s, err, errlen);
}
int yttm_encode_file_idtext(yttm_encoder *h, const char *path, const char *out_path, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes,
                            uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0, nt = 0;
  std::string report;
  Status s = h->enc->encode_file_idtext(path ? path : "", out_path ? out_path : "", bos, eos, reverse, dropout_prob, chunk_bytes, &nl, &ni, &nt, &report);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (n_text_bytes) *n_text_bytes = nt;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return finish(s, err, errlen);
}

int yttm_spans_device(yttm_encoder *h, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes, uint64_t max_sentence_bytes, int bos,
                      int eos, int reverse, double dropout_prob, uint64_t *n_ids, double *kernel_ms, char *err, int errlen) {
  unsigned long long ni = 0;
  Status s = h->enc->spans_device(d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, &ni, kernel_ms);
  if (n_ids) *n_ids = ni;
  return finish(s, err, errlen);
}
int yttm_spans_text_device(yttm_encoder *h, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_lines,
                           uint64_t *n_ids, double *kernel_ms, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0;
  Status s = h->enc->spans_text_device(d_text, n_bytes, bos, eos, reverse, dropout_prob, &nl, &ni, kernel_ms);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  return finish(s, err, errlen);
}
int yttm_spans_fetch(yttm_encoder *h, uint32_t *spans, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->take_spans(spans, n_sent, false), err, errlen);
}
int yttm_spans_copy_device(yttm_encoder *h, void *d_spans, uint64_t n_sent, char *err, int errlen) {
  return finish(h->enc->take_spans(d_spans, n_sent, true), err, errlen);
}
int yttm_spans_copy_padded(yttm_encoder *h, void *d_matrix, uint64_t n_sent, uint64_t width, uint64_t *longest, char *err, int errlen) {
  unsigned long long need = 0;
  Status s = h->enc->copy_spans_padded(d_matrix, n_sent, width, &need);
  if (longest) *longest = need;
  return finish(s, err, errlen);
}
int yttm_encode_as_ids_spans(yttm_encoder *h, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos, int eos, int reverse,
                             double dropout_prob, int32_t **ids, uint64_t **out_offsets, uint32_t **spans, char *err, int errlen) {
  unsigned long long *off = nullptr;
  Status s = h->enc->encode_as_ids_spans(bytes, (const unsigned long long *)offsets, n_sent, bos, eos, reverse, dropout_prob, ids, &off, spans);
  if (!s.ok()) return finish(s, err, errlen);
  *out_offsets = (uint64_t *)off;
  return 0;
}

int yttm_id_counts_device(yttm_encoder *h, uint64_t n_sent, uint64_t n_bins, int accumulate, uint64_t *n_counted, double *kernel_ms, char *err, int errlen) {
  unsigned long long nc = 0;
  Status s = h->enc->id_counts_device(n_sent, n_bins, accumulate != 0, &nc, kernel_ms);
  if (n_counted) *n_counted = nc;
  return finish(s, err, errlen);
}
int yttm_id_counts_ids_device(yttm_encoder *h, const void *d_ids, uint64_t n_ids, uint64_t n_bins, int accumulate, double *kernel_ms, char *err, int errlen) {
  return finish(h->enc->id_counts_ids_device(d_ids, n_ids, n_bins, accumulate != 0, kernel_ms), err, errlen);
}
int yttm_id_counts_fetch(yttm_encoder *h, uint64_t *counts, uint64_t n_bins, char *err, int errlen) {
  return finish(h->enc->take_id_counts(counts, n_bins, false), err, errlen);
}
int yttm_id_counts_copy_device(yttm_encoder *h, void *d_counts, uint64_t n_bins, char *err, int errlen) {
  return finish(h->enc->take_id_counts(d_counts, n_bins, true), err, errlen);
}
int yttm_encode_file_counts(yttm_encoder *h, const char *path, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes, uint64_t *counts,
                            uint64_t *n_lines, uint64_t *n_ids, char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nl = 0, ni = 0;
  std::string report;
  Status s = h->enc->encode_file_counts(path ? path : "", bos, eos, reverse, dropout_prob, chunk_bytes, (unsigned long long *)counts, &nl, &ni, &report);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return finish(s, err, errlen);
}

static int blocks_done(const Status &s, unsigned long long nr, unsigned long long nf, uint64_t *n_rows, uint64_t *n_frags, char *err, int errlen) {
  if (n_rows) *n_rows = nr;
  if (n_frags) *n_frags = nf;
  return finish(s, err, errlen);
}
int yttm_blocks_device(yttm_encoder *h, uint64_t n_sent, uint64_t seq_len, int mode, int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags,
                       double *kernel_ms, char *err, int errlen) {
  unsigned long long nr = 0, nf = 0;
  const Status s = h->enc->blocks_device(n_sent, seq_len, mode, pad_value, tail, &nr, &nf, kernel_ms);
  return blocks_done(s, nr, nf, n_rows, n_frags, err, errlen);
}
int yttm_blocks_ids_device(yttm_encoder *h, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, uint64_t seq_len, int mode,
                           int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags, double *kernel_ms, char *err, int errlen) {
  unsigned long long nr = 0, nf = 0;
  const Status s = h->enc->blocks_ids_device(d_ids, d_offsets, n_sent, n_ids, seq_len, mode, pad_value, tail, &nr, &nf, kernel_ms);
  return blocks_done(s, nr, nf, n_rows, n_frags, err, errlen);
}
int yttm_blocks_flush(yttm_encoder *h, int32_t pad_value, uint64_t *n_rows, uint64_t *n_frags, double *kernel_ms, char *err, int errlen) {
  unsigned long long nr = 0, nf = 0;
  const Status s = h->enc->blocks_flush(pad_value, &nr, &nf, kernel_ms);
  return blocks_done(s, nr, nf, n_rows, n_frags, err, errlen);
}
int yttm_blocks_open(yttm_encoder *h, uint64_t out[3]) {
  unsigned long long o3[3] = {0, 0, 0};
  h->enc->blocks_open(o3);
  for (int i = 0; i < 3; i++) out[i] = o3[i];
  return 0;
}
int yttm_blocks_discard(yttm_encoder *h) {
  h->enc->blocks_discard();
  return 0;
}
int yttm_blocks_fetch(yttm_encoder *h, int32_t *rows, int32_t *seg, int32_t *pos, int32_t *frags, uint64_t *row_frags, uint64_t n_rows, uint64_t n_frags,
                      char *err, int errlen) {
  return finish(h->enc->take_blocks(rows, seg, pos, frags, row_frags, n_rows, n_frags, false), err, errlen);
}
int yttm_blocks_copy_device(yttm_encoder *h, void *d_rows, void *d_seg, void *d_pos, void *d_frags, void *d_row_frags, uint64_t n_rows, uint64_t n_frags,
                            char *err, int errlen) {
  return finish(h->enc->take_blocks(d_rows, d_seg, d_pos, d_frags, d_row_frags, n_rows, n_frags, true), err, errlen);
}
int yttm_encode_file_blocks(yttm_encoder *h, const char *path, const char *out_prefix, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes,
                            uint64_t seq_len, int mode, int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags, uint64_t *n_lines, uint64_t *n_ids,
                            char *report_json, int report_len, char *err, int errlen) {
  unsigned long long nr = 0, nf = 0, nl = 0, ni = 0;
  std::string report;
  const Status s = h->enc->encode_file_blocks(path ? path : "", out_prefix ? out_prefix : "", bos, eos, reverse, dropout_prob, chunk_bytes, seq_len, mode, pad_value,
                                              tail, &nr, &nf, &nl, &ni, &report);
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  if (s.ok() && report_json && report_len > 0) snprintf(report_json, (size_t)report_len, "%s", report.c_str());
  return blocks_done(s, nr, nf, n_rows, n_frags, err, errlen);
}

static int batches_planned(const Status &s, unsigned long long nk, unsigned long long nb, uint64_t *n_kept, uint64_t *n_batches, char *err, int errlen) {
  if (n_kept) *n_kept = nk;
  if (n_batches) *n_batches = nb;
  return finish(s, err, errlen);
}
int yttm_batches_plan_device(yttm_encoder *h, uint64_t n_sent, uint64_t max_tokens, uint64_t max_sentences, uint64_t min_len, uint64_t max_len, uint64_t *n_kept,
                             uint64_t *n_batches, double *kernel_ms, char *err, int errlen) {
  unsigned long long nk = 0, nb = 0;
  const Status s = h->enc->batches_plan_device(n_sent, max_tokens, max_sentences, min_len, max_len, &nk, &nb, kernel_ms);
  return batches_planned(s, nk, nb, n_kept, n_batches, err, errlen);
}
int yttm_batches_plan_lengths_device(yttm_encoder *h, const void *d_lengths, uint64_t n_sent, uint64_t max_tokens, uint64_t max_sentences, uint64_t min_len,
                                     uint64_t max_len, uint64_t *n_kept, uint64_t *n_batches, double *kernel_ms, char *err, int errlen) {
  unsigned long long nk = 0, nb = 0;
  const Status s = h->enc->batches_plan_lengths_device(d_lengths, n_sent, max_tokens, max_sentences, min_len, max_len, &nk, &nb, kernel_ms);
  return batches_planned(s, nk, nb, n_kept, n_batches, err, errlen);
}
int yttm_batches_gather_device(yttm_encoder *h, uint64_t n_sent, int32_t pad_value, int left_pad, uint64_t *n_elems, double *kernel_ms, char *err, int errlen) {
  unsigned long long ne = 0;
  const Status s = h->enc->batches_gather_device(n_sent, pad_value, left_pad != 0, &ne, kernel_ms);
  if (n_elems) *n_elems = ne;
  return finish(s, err, errlen);
}
int yttm_batches_gather_ids_device(yttm_encoder *h, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, int32_t pad_value, int left_pad,
                                   uint64_t *n_elems, double *kernel_ms, char *err, int errlen) {
  unsigned long long ne = 0;
  const Status s = h->enc->batches_gather_ids_device(d_ids, d_offsets, n_sent, n_ids, pad_value, left_pad != 0, &ne, kernel_ms);
  if (n_elems) *n_elems = ne;
  return finish(s, err, errlen);
}
int yttm_batches_fetch(yttm_encoder *h, uint32_t *order, uint64_t *batch_first, uint32_t *widths, uint64_t *batch_off, int32_t *out, uint64_t n_sent,
                       uint64_t n_batches, uint64_t n_elems, char *err, int errlen) {
  return finish(h->enc->take_batches(order, batch_first, widths, batch_off, out, n_sent, n_batches, n_elems, false), err, errlen);
}
int yttm_batches_copy_device(yttm_encoder *h, void *d_order, void *d_batch_first, void *d_widths, void *d_batch_off, void *d_out, uint64_t n_sent,
                             uint64_t n_batches, uint64_t n_elems, char *err, int errlen) {
  return finish(h->enc->take_batches(d_order, d_batch_first, d_widths, d_batch_off, d_out, n_sent, n_batches, n_elems, true), err, errlen);
}

int yttm_encoder_set_vocabulary(yttm_encoder *h, const uint8_t *allowed, uint64_t n, uint64_t *info, char *err, int errlen) {
  unsigned long long i3[3] = {0, 0, 0};
  Status s = h->enc->set_vocabulary(allowed, n, i3);
  if (info) for (int i = 0; i < 3; i++) info[i] = i3[i];
  return finish(s, err, errlen);
}
int yttm_encoder_vocabulary_stats(yttm_encoder *h, uint64_t out[4]) {
  unsigned long long o4[4] = {0, 0, 0, 0};
  h->enc->vocabulary_stats(o4);
  for (int i = 0; i < 4; i++) out[i] = o4[i];
  return 0;
}
int yttm_restrict_ids_device(yttm_encoder *h, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, int reverse, uint64_t *n_out,
                             double *kernel_ms, char *err, int errlen) {
  unsigned long long no = 0;
  Status s = h->enc->restrict_ids_device(d_ids, d_offsets, n_sent, n_ids, reverse != 0, &no, kernel_ms);
  if (n_out) *n_out = no;
  return finish(s, err, errlen);
}

int yttm_encoder_set_byte_fallback(yttm_encoder *h, int on, char *err, int errlen) { return finish(h->enc->set_byte_fallback(on != 0), err, errlen); }
int yttm_encoder_byte_fallback(yttm_encoder *h) { return h->enc->byte_fallback() ? 1 : 0; }
int yttm_encoder_byte_fallback_stats(yttm_encoder *h, uint64_t out[4]) {
  unsigned long long o4[4] = {0, 0, 0, 0};
  h->enc->byte_fallback_stats(o4);
  for (int i = 0; i < 4; i++) out[i] = o4[i];
  return 0;
}
int yttm_byte_fallback_ids_device(yttm_encoder *h, const void *d_ids, const void *d_id_offsets, const void *d_bytes, const void *d_text_offsets,
                                  uint64_t n_sent, uint64_t n_ids, uint64_t total_bytes, int reverse, uint64_t *n_out, double *kernel_ms, char *err,
                                  int errlen) {
  unsigned long long no = 0;
  Status s = h->enc->byte_fallback_ids_device(d_ids, d_id_offsets, d_bytes, d_text_offsets, n_sent, n_ids, total_bytes, reverse != 0, &no, kernel_ms);
  if (n_out) *n_out = no;
  return finish(s, err, errlen);
}

int yttm_encoder_set_added_tokens(yttm_encoder *h, const uint8_t *blob, const uint64_t *tok_offsets, uint64_t n, char *err, int errlen) {
  return finish(h->enc->set_added_tokens(blob, (const unsigned long long *)tok_offsets, n), err, errlen);
}
int yttm_encoder_added_tokens(yttm_encoder *h, char **blob, uint64_t **tok_offsets, uint64_t *n) {
  const std::vector<std::string> toks = h->enc->added_tokens();
  pack_strings(toks, blob, tok_offsets);
  if (n) *n = toks.size();
  return 0;
}
int yttm_encoder_added_tokens_stats(yttm_encoder *h, uint64_t out[4]) {
  unsigned long long o4[4] = {0, 0, 0, 0};
  h->enc->added_tokens_stats(o4);
  for (int i = 0; i < 4; i++) out[i] = o4[i];
  return 0;
}
int yttm_added_split_device(yttm_encoder *h, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes, uint64_t *n_sub,
                            uint64_t *n_matches, double *kernel_ms, char *err, int errlen) {
  unsigned long long ns = 0, nm = 0;
  Status s = h->enc->added_split_device(d_bytes, d_offsets, n_sent, total_bytes, &ns, &nm, kernel_ms);
  if (n_sub) *n_sub = ns;
  if (n_matches) *n_matches = nm;
  return finish(s, err, errlen);
}
int yttm_added_split_fetch(yttm_encoder *h, uint64_t *sub_first, uint64_t *sub_offsets, int32_t *tok, uint64_t n_sent, uint64_t n_sub, char *err, int errlen) {
  return finish(h->enc->take_added_split(sub_first, sub_offsets, tok, n_sent, n_sub, false), err, errlen);
}
int yttm_added_split_copy_device(yttm_encoder *h, void *d_sub_first, void *d_sub_offsets, void *d_tok, uint64_t n_sent, uint64_t n_sub, char *err,
                                 int errlen) {
  return finish(h->enc->take_added_split(d_sub_first, d_sub_offsets, d_tok, n_sent, n_sub, true), err, errlen);
}

int yttm_encoder_set_cache(yttm_encoder *h, int mode, uint64_t min_bytes) {
  h->enc->set_cache(mode, min_bytes);
  return 0;
}
uint64_t yttm_encode_cache_words(yttm_encoder *h) { return h->enc->cache_words(); }

int yttm_id_to_subword(yttm_encoder *h, int id, char **subword, char *err, int errlen) {
  std::string s;
  Status st = h->enc->id_to_subword(id, &s);
  if (!st.ok()) return finish(st, err, errlen);
  *subword = (char *)malloc(s.size() + 1);
  memcpy(*subword, s.c_str(), s.size() + 1);
  return 0;
}
int yttm_subword_to_id(yttm_encoder *h, const char *token) { return h->enc->subword_to_id(token); }

int yttm_decode(yttm_encoder *h, const int32_t *ids, const uint64_t *offsets, uint64_t n_sent, const int32_t *ignore_ids, uint64_t n_ignore,
                char **blob, uint64_t **out_offsets, char *err, int errlen) {
  std::unordered_set<int> ign(ignore_ids, ignore_ids + n_ignore);
  std::vector<std::string> out;
  for (uint64_t i = 0; i < n_sent; i++) {
    std::vector<int> v(ids + offsets[i], ids + offsets[i + 1]);
    std::string s;
    Status st = h->enc->decode(v, &s, &ign);
    if (!st.ok()) return finish(st, err, errlen);
    out.push_back(std::move(s));
  }
  pack_strings(out, blob, out_offsets);
  return 0;
}
int yttm_vocab_size(yttm_encoder *h) { return h->enc->vocab_size(); }
int yttm_vocabulary(yttm_encoder *h, char **blob, uint64_t **offsets, uint64_t *n) {
  std::vector<std::string> v = h->enc->vocabulary();
  pack_strings(v, blob, offsets);
  *n = v.size();
  return 0;
}
int yttm_encode_cli(yttm_encoder *h, const char *output_type, int stream, int bos, int eos, int reverse, double dropout_prob, int in_fd, int out_fd,
                    char *err, int errlen) {
  return finish(h->enc->encode_cli(output_type, stream != 0, bos != 0, eos != 0, reverse != 0, dropout_prob, in_fd, out_fd), err, errlen);
}
int yttm_decode_cli(yttm_encoder *h, const int32_t *ignore_ids, uint64_t n_ignore, int in_fd, int out_fd, char *err, int errlen) {
  std::unordered_set<int> ign;
  for (uint64_t i = 0; i < n_ignore; i++) ign.insert(ignore_ids[i]);
  return finish(h->enc->decode_cli(&ign, in_fd, out_fd), err, errlen);
}
int yttm_vocab_cli(yttm_encoder *h, int verbose, int out_fd, char *err, int errlen) {
  return finish(h->enc->vocab_cli(verbose != 0, out_fd), err, errlen);
}

unsigned long long yttm_ids_fnv1a64(const int32_t *ids, const uint64_t *offsets, uint64_t n_sent) {
  unsigned long long h = 1469598103934665603ull;
  auto mix4 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) { h ^= (v >> (8 * k)) & 0xffu; h *= 1099511628211ull; }
  };
  for (uint64_t i = 0; i < n_sent; i++) {
    mix4((uint32_t)(offsets[i + 1] - offsets[i]));
    for (uint64_t k = offsets[i]; k < offsets[i + 1]; k++) mix4((uint32_t)ids[k]);
  }
  return h;
}

void yttm_free(void *p) { free(p); }

int yttm_device_info(int device, char *buf, int buflen) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= device) {
    snprintf(buf, (size_t)buflen, "no HIP device %d visible (%s)", device, e != hipSuccess ? hipGetErrorString(e) : "device count too small");
    return 1;
  }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) { snprintf(buf, (size_t)buflen, "hipGetDeviceProperties failed"); return 1; }
  snprintf(buf, (size_t)buflen, "%s %s CUs=%d HBM=%.1fGB", p.gcnArchName, p.name, p.multiProcessorCount, (double)p.totalGlobalMem / 1e9);
  return 0;
}

// ------------------------------------------------------------------------------------------------- inner ABI
static thread_local std::string g_last_error;
const char *yttm_gpu_last_error(void) { return g_last_error.c_str(); }

struct yttm_ctx {
  GpuCtx *g;
};

#define GUARD(...)                                   \
  try {                                              \
    __VA_ARGS__;                                     \
    return 0;                                        \
  } catch (const GpuError &e) {                      \
    g_last_error = e.msg;                            \
    return 2;                                        \
  } catch (const std::exception &e) {                \
    g_last_error = e.what();                         \
    return 2;                                        \
  }

// the same with the context's own snapshot of the YTTM_* hooks bound to the calling thread (yttm_config.h CfgBind)
#define GUARD_CTX(...) GUARD({ const CfgBind _bind(c && c->g ? c->g->config_ptr() : nullptr); __VA_ARGS__; })

int yttm_gpu_ctx_create(int device, yttm_ctx **out) {
  *out = nullptr;
  GUARD({ *out = new yttm_ctx{new GpuCtx(device)}; })
}
void yttm_gpu_ctx_destroy(yttm_ctx *c) {
  if (!c) return;
  delete c->g;
  delete c;
}
int yttm_gpu_ctx_set_comm(yttm_ctx *c, void *comm) { GUARD_CTX(c->g->set_comm((Comm *)comm)) }
int yttm_gpu_upload_corpus(yttm_ctx *c, const uint8_t *utf8, uint64_t n) { GUARD_CTX(c->g->upload_corpus(utf8, n)) }
int yttm_gpu_attach_corpus(yttm_ctx *c, const void *p, uint64_t n) { GUARD_CTX(c->g->attach_corpus(p, n)) }

int yttm_gpu_char_hist(yttm_ctx *c, uint32_t *cps, uint64_t *cnts, uint32_t *n_inout, uint64_t *n_codepoints) {
  GUARD_CTX({
    std::vector<uint32_t> a;
    std::vector<unsigned long long> b;
    unsigned long long steps = 0;
    c->g->char_hist(a, b, steps);
    if (a.size() > *n_inout) throw GpuError{"char_hist: output capacity too small"};
    for (size_t i = 0; i < a.size(); i++) { cps[i] = a[i]; cnts[i] = b[i]; }
    *n_inout = (uint32_t)a.size();
    *n_codepoints = steps;
  })
}
int yttm_gpu_build_word_table(yttm_ctx *c, const uint32_t *cp, const uint32_t *id, uint32_t n_alpha, uint32_t space_id, uint32_t n_ids_cap,
                              uint64_t *n_unique, uint64_t *n_tokens) {
  GUARD_CTX({
    c->g->build_word_table(cp, id, n_alpha, space_id, n_ids_cap);
    *n_unique = c->g->n_unique;
    *n_tokens = c->g->n_tokens0;
  })
}
int yttm_gpu_download_word_table(yttm_ctx *c, uint32_t *tok, uint64_t *off, uint32_t *cnt, uint64_t *n_tokens_now) {
  GUARD_CTX({
    std::vector<uint32_t> t, w;
    std::vector<unsigned long long> o;
    c->g->download_word_table(t, o, w);
    memcpy(tok, t.data(), t.size() * 4);
    for (size_t i = 0; i < o.size(); i++) off[i] = o[i];
    memcpy(cnt, w.data(), w.size() * 4);
    *n_tokens_now = t.size();
  })
}
int yttm_gpu_pair_count(yttm_ctx *c, uint64_t *n_pairs) {
  GUARD_CTX({
    c->g->pair_count();
    *n_pairs = c->g->n_keys_host;
  })
}
int yttm_gpu_download_pairs(yttm_ctx *c, uint64_t *pairs, uint64_t *counts, uint64_t *n_inout) {
  GUARD_CTX({
    std::vector<unsigned long long> k, v;
    c->g->download_pairs(k, v);
    if (k.size() > *n_inout) throw GpuError{"download_pairs: output capacity too small"};
    for (size_t i = 0; i < k.size(); i++) { pairs[i] = k[i]; counts[i] = v[i]; }
    *n_inout = k.size();
  })
}
int yttm_gpu_download_index(yttm_ctx *c, uint64_t *pairs, uint64_t *run_lo, uint64_t *run_hi, uint64_t *n_keys_inout, uint32_t *post, uint64_t *n_post_inout) {
  GUARD_CTX({
    std::vector<unsigned long long> k, lo, hi;
    std::vector<uint32_t> p;
    c->g->download_index(k, lo, hi, p);
    const bool fits = k.size() <= *n_keys_inout && p.size() <= *n_post_inout;
    *n_keys_inout = k.size();
    *n_post_inout = p.size();
    if (!fits) throw GpuError{"download_index: output capacity too small"};
    for (size_t i = 0; i < k.size(); i++) { pairs[i] = k[i]; run_lo[i] = lo[i]; run_hi[i] = hi[i]; }
    if (!p.empty()) memcpy(post, p.data(), p.size() * 4);
  })
}
int yttm_gpu_merge_apply(yttm_ctx *c, const uint32_t *xyz, uint32_t k) { GUARD_CTX(c->g->merge_apply(xyz, k, nullptr)) }
int yttm_gpu_merge_apply_scan(yttm_ctx *c, const uint32_t *xyz, uint32_t k, const uint64_t *rule_counts, uint64_t next_tau_cnt, uint32_t next_tau_mx,
                              uint32_t next_want) {
  GUARD_CTX({
    const unsigned long long tau = next_tau_cnt;
    c->g->merge_apply(xyz, k, (const unsigned long long *)rule_counts, &tau, next_tau_mx, next_want);
  })
}
int yttm_gpu_round_stats(yttm_ctx *c, uint64_t *out, uint32_t n) {
  GUARD_CTX({
    const GpuCtx &g = *c->g;
    const unsigned long long v[YTTM_ROUND_STATS] = {g.merge_rounds, g.word_rounds, g.word_all_rounds, g.word_fused_rounds, g.index_builds, g.classb_word_rounds,
                                                    g.fused_rounds, g.fused_overflows, g.hot_rebuilds, g.top_refills, g.word_switch_round, g.exchange_retries, g.k3_radix,
                                                    g.index_radix_builds};
    for (uint32_t i = 0; i < std::min<uint32_t>(n, YTTM_ROUND_STATS); i++) out[i] = v[i];
  })
}
int yttm_gpu_pair_query(yttm_ctx *c, const uint64_t *pairs, uint32_t n, uint64_t *counts) {
  GUARD_CTX(c->g->pair_query((const unsigned long long *)pairs, n, (unsigned long long *)counts))
}
int yttm_gpu_candidates(yttm_ctx *c, uint64_t tau_cnt, uint32_t tau_mx, uint64_t *pairs, uint64_t *counts, uint32_t *n_inout) {
  GUARD_CTX({
    std::vector<CandRec> out;
    uint32_t n = c->g->candidates(tau_cnt, tau_mx, out, nullptr);
    uint32_t take = std::min<uint32_t>((uint32_t)out.size(), *n_inout);
    for (uint32_t i = 0; i < take; i++) { pairs[i] = out[i].key; counts[i] = out[i].cnt; }
    *n_inout = n;
  })
}

int yttm_gpu_k4_measure(yttm_ctx *c, int on, uint64_t out[6]) {
  GUARD_CTX({
    c->g->instrument = on != 0;
    if (out) {
      c->g->resolve_timers();
      out[0] = c->g->merge_sites; out[1] = c->g->touched_tiles; out[2] = c->g->touched_tile_tokens;
      out[3] = c->g->touched_words; out[4] = c->g->touched_word_tokens; out[5] = c->g->merge_rounds;
    }
  })
}

void yttm_release_device_memory(void) { yttm::release_device_memory(); }
void yttm_gpu_pool_stats(uint64_t out[4]) {
  unsigned long long v[4];
  yttm::pool_stats(v);
  for (int i = 0; i < 4; i++) out[i] = v[i];
}
const char *yttm_config_table(void) { return yttm::config_table_markdown(); }

}  // extern "C"
