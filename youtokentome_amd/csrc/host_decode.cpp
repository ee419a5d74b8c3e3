// host_decode.cpp -- host side of the device decode (k_decode.h), of the SUBWORD formatter (k_subword.h) and the id printer (k_idtext.h), which
// leave their text in the decode's slot, and the device-to-device exits of the encoder's and the decoder's results, on the encoder's lanes
// (enc_lanes.h).
//
// Results live in lane 0 like those of encode_device, in buffers of their own: a decode leaves a pending encode result alone and the other way
// round.  Every call locks the lane and returns after the lane's stream has synchronised; a pair (decode_device, fetch) is not atomic.
#include <algorithm>

#include "enc_lanes.h"
#include "idcount_plan.h"

namespace yttm {

// A piece table, once per encoder (under dec_mu; `ready` is the table's own flag): build(blob, off, per_id) fills the text of every id back to
// back, off[V + 256 + 1] (the byte ids' entries are always there; the bound handed to the kernels says whether they count) and -- where the table has a third array, dst_per_id -- a word per id, by the table's own per-id rules.  All are allocated,
// then copied, and handed to the encoder together once every copy is there: a failure on the way leaves the encoder as it was.
template <class Build>
static void table_once(const BaseEncoder &enc, EncoderDevice &D, bool &ready, DevBuf<uint8_t> &dst_blob, DevBuf<uint32_t> &dst_off,
                       DevBuf<uint32_t> *dst_per_id, Build &&build) {
  std::lock_guard<std::mutex> lk(D.dec_mu);
  if (ready) return;
  std::string blob;
  std::vector<uint32_t> off(added_table_offsets((uint32_t)enc.vocab_size(), D.add.n.load()), 0), per_id(dst_per_id ? (size_t)enc.vocab_size() : 0, 0);
  build(blob, off, per_id);
  DevBuf<uint8_t> d_blob;
  DevBuf<uint32_t> d_off, d_per_id;
  d_blob.alloc(blob.size() + 1);
  d_off.alloc(off.size());
  if (dst_per_id) d_per_id.alloc(per_id.size());
  if (!blob.empty()) HIP_CHECK(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  if (!per_id.empty()) HIP_CHECK(hipMemcpy(d_per_id, per_id.data(), per_id.size() * 4, hipMemcpyHostToDevice));
  dst_blob = std::move(d_blob);
  dst_off = std::move(d_off);
  if (dst_per_id) *dst_per_id = std::move(d_per_id);
  ready = true;
}

// The text of every id: from the host's id_to_subword(id, replace_space = true), so that the device path cannot drift from the host path.  An
// id the host function refuses is marked (DEC_INVALID) and reported by the device path the same way.
static void decode_table(const BaseEncoder &enc, EncoderDevice &D) {
  table_once(enc, D, D.dec_ready, D.piece_blob, D.piece_off, nullptr, [&](std::string &blob, std::vector<uint32_t> &off, std::vector<uint32_t> &) {
    const int V = enc.vocab_size();
    std::string piece;
    for (int id = 0; id < V; id++) {
      if (blob.size() >= (size_t)DEC_INVALID) throw GpuError{"decode: the vocabulary's text does not fit 2 GB"};
      off[(size_t)id] = (uint32_t)blob.size();
      piece.clear();
      bool ok = false;
      try {
        ok = enc.id_to_subword(id, &piece, true).ok();
      } catch (const std::exception &) {
      }
      if (ok) blob += piece;
      else off[(size_t)id] |= DEC_INVALID;
    }
    if (blob.size() + BYTE_IDS >= (size_t)DEC_INVALID) throw GpuError{"decode: the vocabulary's text does not fit 2 GB"};
    for (uint32_t b = 0; b <= BYTE_IDS; b++) off[(size_t)V + b] = (uint32_t)blob.size() + b;  // a byte id's piece is the raw byte
    for (uint32_t b = 0; b < BYTE_IDS; b++) blob += (char)b;
    // an added id's piece is the token verbatim.  With added tokens the bound lies behind the byte ids whether the byte fallback is on or not:
    // while it is off they are marked as ids the host refuses (set_byte_fallback and set_added_tokens have this table made again)
    const uint32_t n_added = D.add.n.load();
    if (n_added && !D.bfb.on.load())
      for (uint32_t b = 0; b < BYTE_IDS; b++) off[(size_t)V + b] |= DEC_INVALID;
    for (uint32_t k = 0; k < n_added; k++) {
      blob += D.add.toks[k];
      off[(size_t)V + BYTE_IDS + k + 1] = (uint32_t)blob.size();
    }
    if (blob.size() >= (size_t)DEC_INVALID) throw GpuError{"decode: the vocabulary's text does not fit 2 GB"};
    D.dec_vocab = (uint32_t)V;
  });
}

// A text for n_sent sentences into the lane's text slot (dec; the lane locked by the caller): the slot is invalid from the first step on and
// valid again only with the new text in it.  No sentence: an empty text, nothing is launched.  Else prepare() (tables, inputs), then the two
// passes over dec.len / dec.off (two_pass_on_lane: launch, check) into dec.bytes, which has 16 bytes more than the text -- the writer's last
// 16-byte store may reach past the end -- and must be 16-byte aligned.  `who` names the route in that message.
template <class Prepare, class Launch, class Check>
static Status text_on_lane(EncodeLane &d, int device, const char *who, unsigned long long n_sent, unsigned long long *n_bytes, double *kernel_ms,
                           Prepare &&prepare, Launch &&launch, Check &&check) {
  return on_device(device, [&]() -> Status {
    d.dec.valid = false;
    if (n_bytes) *n_bytes = 0;
    if (kernel_ms) *kernel_ms = 0;
    unsigned long long total = 0;
    if (n_sent) {
      prepare();
      const Status s = two_pass_on_lane(d, n_sent, d.dec.len, d.dec.off, kernel_ms, &total, launch, check, [&](unsigned long long need) {
        d.dec.bytes.grow((size_t)need + 16);
        if (((uintptr_t)d.dec.bytes.p & 15u) != 0) throw GpuError{std::string(who) + ": the output blob is not 16-byte aligned"};
      });
      if (!s.ok()) return s;
    }
    d.dec.n_sent = n_sent;
    d.dec.n_bytes = total;
    d.dec.valid = true;
    if (n_bytes) *n_bytes = total;
    return Status();
  });
}
static Status no_check() { return Status(); }

// measure -> scan -> write on the lane (locked by the caller).  n_flat: the ids the kernels walk (ragged: n_ids; padded: n_sent * stride).
// newline (ragged input only): a '\n' behind every sentence, as decode_cli writes its lines.
Status decode_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, DecInput in, unsigned long long n_flat,
                      const int32_t *ignore_ids, unsigned long long n_ignore, unsigned long long *n_bytes, double *kernel_ms, bool newline) {
  DecTable tb{};
  DecIgnore ig{nullptr, nullptr, 0, 0};
  unsigned long long bad = ~0ull;  // the measure pass's smallest flat index of an invalid id
  return text_on_lane(
      d, device, "decode", in.n_sent, n_bytes, kernel_ms,
      [&] {
        decode_table(enc, D);
        const uint32_t bound = D.id_bound(D.dec_vocab);
        tb = DecTable{D.piece_blob, D.piece_off, bound};
        if (!n_ignore) return;
        const size_t words = bytefb_bitmap_words(bound);
        std::vector<uint32_t> host(words, 0);
        std::vector<int32_t> extra;
        for (unsigned long long i = 0; i < n_ignore; i++) {
          const int32_t id = ignore_ids[i];
          if ((uint32_t)id < bound) host[(uint32_t)id >> 5] |= 1u << ((uint32_t)id & 31u);
          else extra.push_back(id);
        }
        std::sort(extra.begin(), extra.end());
        extra.erase(std::unique(extra.begin(), extra.end()), extra.end());
        for (int32_t id : extra) host.push_back((uint32_t)id);
        d.dec.ign.grow(host.size());
        HIP_CHECK(hipMemcpy(d.dec.ign, host.data(), host.size() * 4, hipMemcpyHostToDevice));  // (the lane's stream is idle; the vector ends with this call)
        ig = DecIgnore{d.dec.ign, (const int32_t *)(d.dec.ign + words), (uint32_t)extra.size(), 1u};
      },
      [&](bool write) {
        if (!write) HIP_CHECK(hipMemsetAsync(d.dec.misc, 0xff, 8, d.st));
        launch_decode(write, newline, in, tb, ig, n_flat, d.dec.len, d.dec.misc, d.dec.off, d.dec.bytes, d.st);
        if (!write) HIP_CHECK(hipMemcpyAsync(&bad, d.dec.misc, 8, hipMemcpyDeviceToHost, d.st));  // (here once the scan has synchronised)
      },
      [&]() -> Status {
        if (bad == ~0ull) return Status();
        // the first id, in sentence order then position order, that is neither ignored nor valid: the host path's message
        int32_t id = 0;
        HIP_CHECK(hipMemcpyAsync(&id, in.ids + bad, 4, hipMemcpyDeviceToHost, d.st));
        HIP_CHECK(hipStreamSynchronize(d.st));
        std::string piece;
        const Status st = enc.id_to_subword(id, &piece, true);
        return st.ok() ? Status(1, "decode: no text for id " + std::to_string(id)) : st;
      });
}

Status BaseEncoder::decode_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, const int32_t *ignore_ids,
                                  unsigned long long n_ignore, unsigned long long *n_bytes, double *kernel_ms) const {
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && !d_offsets) return Status(2, "decode_device: no offsets");
  const Lane0 l(*dev_);
  const DecInput in{(const int32_t *)d_ids, (const unsigned long long *)d_offsets, nullptr, 0, 0, n_sent};
  return decode_on_lane(*this, *dev_, l.d, device_, in, n_ids, ignore_ids, n_ignore, n_bytes, kernel_ms, false);
}

Status BaseEncoder::decode_device_padded(const void *d_ids, unsigned long long n_sent, unsigned long long width, unsigned long long row_stride,
                                         const void *d_lengths, const int32_t *ignore_ids, unsigned long long n_ignore, unsigned long long *n_bytes,
                                         double *kernel_ms) const {
  if (!dev_) return Status(2, "encoder has no device state");
  if (row_stride < width) return Status(2, "decode_device_padded: row_stride is smaller than width");
  if (row_stride == 0) row_stride = 1;  // (width 0: rows without ids)
  if (n_sent > (~0ull >> 1) / row_stride) return Status(2, "decode_device_padded: the matrix is too large");
  const Lane0 l(*dev_);
  const DecInput in{(const int32_t *)d_ids, nullptr, (const int32_t *)d_lengths, width, row_stride, n_sent};
  return decode_on_lane(*this, *dev_, l.d, device_, in, n_sent * row_stride, ignore_ids, n_ignore, n_bytes, kernel_ms, false);
}

Status BaseEncoder::fetch_decode_result(char *bytes, unsigned long long *out_off, unsigned long long n_sent) const {
  if (!dev_) return Status(2, "fetch_decode_result: no matching result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.dec.valid || n_sent != d.dec.n_sent) return Status(2, "fetch_decode_result: no matching result");
  return on_device(device_, [&]() -> Status {
    if (n_sent == 0) { if (out_off) out_off[0] = 0; return Status(); }
    if (bytes && d.dec.n_bytes) copy_down(device_, bytes, d.dec.bytes, (size_t)d.dec.n_bytes, d.st);
    if (out_off) copy_down(device_, out_off, d.dec.off, (size_t)(n_sent + 1) * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

Status BaseEncoder::copy_decode_result(void *d_bytes, void *d_out_off, unsigned long long n_sent) const {
  if (!dev_) return Status(2, "copy_decode_result: no matching result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.dec.valid || n_sent != d.dec.n_sent) return Status(2, "copy_decode_result: no matching result");
  return copy_out_device(device_, d, d_bytes, d.dec.bytes, (size_t)d.dec.n_bytes, d_out_off, d.dec.off, n_sent);
}

Status BaseEncoder::copy_encode_result(void *d_ids, void *d_out_off, unsigned long long n_sent) const {
  if (!dev_) return Status(2, "copy_encode_result: no matching result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (n_sent != d.res.n_sent) return Status(2, "copy_encode_result: no matching result");
  return copy_out_device(device_, d, d_ids, d.res.ids, (size_t)d.res.n_ids * 4, d_out_off, d.res.off, n_sent);
}

// The longest row of the encode result pending on the lane (k_enc_longest; synchronises), checked against the width of a padded copy: a row
// that does not fit is the reference's message, code 1 -- nothing is truncated, and nothing was written.
static Status longest_row_fits(EncodeLane &d, unsigned long long n_sent, unsigned long long width, unsigned long long *need, unsigned long long *longest) {
  HIP_CHECK(hipMemsetAsync(d.res.misc, 0, 8, d.st));
  launch_enc_longest(d.res.off, n_sent, (unsigned int *)d.res.misc.p, d.st);
  HIP_CHECK(hipMemcpyAsync(need, d.res.misc, 8, hipMemcpyDeviceToHost, d.st));
  HIP_CHECK(hipStreamSynchronize(d.st));
  if (longest) *longest = *need;
  if (*need > width)
    return Status(1, "width is smaller than the longest row. Current value: width = " + std::to_string(width) + "; longest = " + std::to_string(*need) + ";");
  return Status();
}

Status BaseEncoder::copy_encode_padded(void *d_matrix, void *d_lengths, unsigned long long n_sent, unsigned long long width, int32_t pad_value,
                                       unsigned long long *longest) const {
  if (longest) *longest = 0;
  if (!dev_) return Status(2, "copy_encode_padded: no matching result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (n_sent != d.res.n_sent) return Status(2, "copy_encode_padded: no matching result");
  if (n_sent == 0) return Status();
  return on_device(device_, [&]() -> Status {
    unsigned long long need = 0;
    const Status fit = longest_row_fits(d, n_sent, width, &need, longest);
    if (!fit.ok()) return fit;
    if (need > 0x7fffffffull) return Status(2, "copy_encode_padded: a row is too long for int32 lengths");
    if (!d_matrix || !d_lengths) return Status(2, "copy_encode_padded: no output");
    if (((uintptr_t)d_matrix & 3u) != 0) return Status(2, "copy_encode_padded: the matrix must be 4-byte aligned");
    launch_enc_pad(d.res.ids, d.res.off, n_sent, width, pad_value, (int32_t *)d_matrix, (int32_t *)d_lengths, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// ---- SUBWORD output (k_subword.h) ----------------------------------------------------------------------------------------------------------
// The text `yttm encode --output_type subword` prints for a batch, made on the device from the ids K5 left and the batch's own text.  It lands
// in the lane's text slot, the one a device decode uses: it is taken with fetch_decode_result / copy_decode_result and replaces a pending
// decode result; the ids stay pending as after encode_device.
// The text of every id, once per encoder: from the host's id_to_subword(id, replace_space = false), so that the device path cannot drift from
// the host path ("▁" stays, the special ids give their names, a hole of the id space is "").
static void subword_table(const BaseEncoder &enc, EncoderDevice &D) {
  // units: the units an id covers (k_spans.h), counted beside the pieces
  table_once(enc, D, D.sub_ready, D.sub_blob, D.sub_off, &D.sub_units, [&](std::string &blob, std::vector<uint32_t> &off, std::vector<uint32_t> &units) {
    const int V = enc.vocab_size();
    std::string piece;
    const SpecialTokens &sp = enc.bpe_state.special_tokens;
    for (int id = 0; id < V; id++) {
      off[(size_t)id] = (uint32_t)blob.size();
      piece.clear();
      if (enc.id_to_subword(id, &piece, false).ok()) blob += piece;
      if (blob.size() >= (size_t)DEC_INVALID) throw GpuError{"subword: the vocabulary's text does not fit 2 GB"};
      // an unknown run is one unit; a special token none; else the piece's code points other than U+2581
      if (id == sp.unk_id) {
        units[(size_t)id] = 1;
      } else if (id != sp.pad_id && id != sp.bos_id && id != sp.eos_id) {
        uint32_t n = 0;
        for (size_t i = 0; i < piece.size(); i++) {
          if (((uint8_t)piece[i] & 0xC0u) == 0x80u) continue;
          if (piece.compare(i, 3, "\xe2\x96\x81") != 0) n++;
        }
        units[(size_t)id] = n;
      }
    }
    for (uint32_t b = 0; b < BYTE_IDS; b++) {  // a byte id prints as its name, <0xNN>
      off[(size_t)V + b] = (uint32_t)blob.size();
      blob += bytefb_name(b);
    }
    off[(size_t)V + BYTE_IDS] = (uint32_t)blob.size();
    for (uint32_t k = 0; k < D.add.n.load(); k++) {  // an added id prints as the token
      blob += D.add.toks[k];
      off[(size_t)V + BYTE_IDS + k + 1] = (uint32_t)blob.size();
    }
  });
}

static SubInput pending_input(const BaseEncoder &enc, const EncodeLane &d, const void *d_text, const void *d_soff, bool reverse) {
  return SubInput{(const uint8_t *)d_text, (const unsigned long long *)d_soff, d.res.ids, d.res.off, d.res.n_sent, (int32_t)enc.bpe_state.special_tokens.unk_id,
                  reverse ? 1 : 0};
}

Status format_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, const void *d_soff, bool reverse,
                      unsigned long long *n_text_bytes, double *kernel_ms) {
  const SubInput in = pending_input(enc, d, d_text, d_soff, reverse);
  return text_on_lane(
      d, device, "subword", in.n_sent, n_text_bytes, kernel_ms, [&] { subword_table(enc, D); },
      [&](bool write) {
        launch_subword(write, D.m, in, DecTable{D.sub_blob, D.sub_off, D.id_bound((uint32_t)enc.vocab_size())}, d.res.n_ids, d.dec.len, d.dec.off, d.dec.bytes, d.st);
      },
      no_check);
}

// ---- id text (k_idtext.h) ------------------------------------------------------------------------------------------------------------------
// The text `yttm encode --output_type id` prints for the encode result pending on the lane (utils.h:92-103: every id and a space, a newline per
// sentence), left in the lane's text slot like the SUBWORD text; the ids stay pending.  Needs no input text and no table.
Status idtext_on_lane(EncodeLane &d, int device, unsigned long long *n_text_bytes, double *kernel_ms) {
  return text_on_lane(
      d, device, "idtext", d.res.n_sent, n_text_bytes, kernel_ms, [] {},
      [&](bool write) { launch_idprint(write, d.res.ids, d.res.off, d.res.n_sent, d.res.n_ids, d.dec.len, d.dec.off, d.dec.bytes, d.st); }, no_check);
}

Status BaseEncoder::idtext_device(unsigned long long n_sent, unsigned long long *n_text_bytes, double *kernel_ms) const {
  if (n_text_bytes) *n_text_bytes = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(1, "idtext_device: no matching encode result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (n_sent != d.res.n_sent) return Status(1, "idtext_device: no matching encode result");  // (before any work: a pending text stays)
  return idtext_on_lane(d, device_, n_text_bytes, ms.next());
}

// ---- token frequencies (k_idcount.h) -------------------------------------------------------------------------------------------------------
// uint64 counts[n_bins + 1] of an id array in HBM, in the encoder's own slot (EncoderDevice::idc): counts[v] the ids equal to v, the last one the
// ids outside [0, n_bins).  One pass that writes nothing per id; what it counts is only read.
Status count_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *d_ids, unsigned long long n_ids, unsigned long long n_bins, bool accumulate,
                     double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (n_bins == 0 || n_bins > IDC_BINS_MAX) return Status(1, "id_counts: n_bins must be within 1 .. 2^31");
  const bool fresh = !accumulate || !D.idc.valid;
  if (!fresh && D.idc.n_bins != n_bins)
    return Status(1, "id_counts: accumulate needs the n_bins of the counts so far (" + std::to_string(D.idc.n_bins) + ", not " + std::to_string(n_bins) + ")");
  if (n_ids && !d_ids) return Status(2, "id_counts: no ids");
  return on_device(device, [&]() -> Status {
    EventPair ev(d.st, kernel_ms != nullptr);
    if (fresh) {
      D.idc.valid = false;
      D.idc.counts.grow((size_t)n_bins + 1);
      D.idc.n_bins = n_bins;
    }
    ev.start();
    if (fresh) HIP_CHECK(hipMemsetAsync(D.idc.counts, 0, ((size_t)n_bins + 1) * 8, d.st));
    launch_idcount(d_ids, n_ids, n_bins, D.idc.counts, d.st);
    ev.stop();
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
    D.idc.valid = true;
    return Status();
  });
}

Status BaseEncoder::id_counts_device(unsigned long long n_sent, unsigned long long n_bins, bool accumulate, unsigned long long *n_counted,
                                     double *kernel_ms) const {
  if (n_counted) *n_counted = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(1, "id_counts_device: no matching encode result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.res.made || n_sent != d.res.n_sent) return Status(1, "id_counts_device: no matching encode result");  // (before any work: the counts stay)
  const Status s = count_on_lane(*dev_, d, device_, d.res.ids, d.res.n_ids, n_bins ? n_bins : default_bins(), accumulate, ms.next());
  if (s.ok() && n_counted) *n_counted = d.res.n_ids;
  return s;
}

Status BaseEncoder::id_counts_ids_device(const void *d_ids, unsigned long long n_ids, unsigned long long n_bins, bool accumulate, double *kernel_ms) const {
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (((uintptr_t)d_ids & 3u) != 0) return Status(2, "id_counts_ids_device: the ids must be 4-byte aligned");
  const Lane0 l(*dev_);
  return count_on_lane(*dev_, l.d, device_, (const int32_t *)d_ids, n_ids, n_bins ? n_bins : default_bins(), accumulate, ms.next());
}

Status BaseEncoder::take_id_counts(void *counts, unsigned long long n_bins, bool to_device) const {
  const char *who = to_device ? "copy_id_counts: no matching counts" : "fetch_id_counts: no matching counts";
  if (!dev_) return Status(1, who);
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!dev_->idc.valid || (n_bins ? n_bins : default_bins()) != dev_->idc.n_bins) return Status(1, who);
  if (!counts) return Status(2, "id_counts: no output");
  const size_t bytes = ((size_t)dev_->idc.n_bins + 1) * 8;
  return on_device(device_, [&]() -> Status {
    if (to_device) HIP_CHECK(hipMemcpyAsync(counts, dev_->idc.counts, bytes, hipMemcpyDeviceToDevice, d.st));
    else copy_down(device_, counts, dev_->idc.counts, bytes, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// ---- training blocks (k_blocks.h) ----------------------------------------------------------------------------------------------------------
// Rows of exactly L ids from the encoder's open row followed by the call's sentences, in the encoder's own slot (EncoderDevice::blk).  seg and pos
// are kept in the slot beside the rows: the write pass has them in registers when it stores the ids, and the exits stay plain copies.
// Order: everything that can refuse the call (the parameters, the open row's binding, a sentence longer than L, the size limit) is known before
// the slot or the open row is touched -- the passes up to there write working arrays only.
Status blocks_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                      unsigned long long n_ids, const BlkParams &p, const char *what, unsigned long long first_index, unsigned long long *n_rows_out,
                      unsigned long long *n_frags_out, double *kernel_ms) {
  if (n_rows_out) *n_rows_out = 0;
  if (n_frags_out) *n_frags_out = 0;
  if (kernel_ms) *kernel_ms = 0;
  auto &B = D.blk;
  const unsigned long long L = p.L;
  if (L < 1 || L > (1ull << 24)) return Status(1, "blocks: seq_len must be within 1 .. 2^24 (" + std::to_string(L) + ")");
  if (p.mode != 0 && p.mode != 1) return Status(1, "blocks: mode must be 0 (stream) or 1 (whole)");
  if (p.tail < 0 || p.tail > 2) return Status(1, "blocks: tail must be 0 (pad), 1 (keep) or 2 (drop)");
  if (B.open_f && (B.open_L != L || B.open_mode != p.mode))
    return Status(1, "blocks: the open row holds " + std::to_string(B.open_f) + " ids for seq_len " + std::to_string(B.open_L) + ", mode " +
                         std::to_string(B.open_mode) + "; flush or discard it before packing with seq_len " + std::to_string(L) + ", mode " + std::to_string(p.mode));
  if (n_sent && !off) return Status(2, "blocks: no offsets");
  if (n_ids && !ids) return Status(2, "blocks: no ids");
  const unsigned long long m = B.open_f ? B.open_m : 0, f = B.open_f, n = m + n_sent, total = f + n_ids;
  if (n >= 0xfffffffeull) return Status(1, "blocks: too many sentences for one call");
  return on_device(device, [&]() -> Status {
    const BlkIn in{B.open_ids[B.gen], B.open_off[B.gen], m, f, ids, off, n_sent, total};
    EventPair ev(d.st, kernel_ms != nullptr);
    ev.start();
    unsigned long long rows = 0, rest = 0;  // complete rows; the ids of the incomplete row behind them
    const uint32_t *rowsent = nullptr;
    if (total) {
      B.cnt.grow((size_t)n);
      B.ne.grow((size_t)n + 1);
      B.info.grow(4);
      launch_blk_flags(in, B.cnt, d.st);
      (void)scan_counts(d, B.cnt, n, B.ne);  // (syncs)
      if (p.mode == 1) {
        const size_t nb = (size_t)((n + BLK_ORBIT - 1) / BLK_ORBIT);
        B.nxt.grow((size_t)n);
        B.hop.grow((size_t)n);
        B.entry.grow(nb);
        B.rowbase.grow(nb);
        B.rowsent.grow((size_t)n + 1);
        HIP_CHECK(hipMemsetAsync(B.entry, 0xff, nb * 4, d.st));
        HIP_CHECK(hipMemsetAsync(B.info, 0, 24, d.st));
        HIP_CHECK(hipMemsetAsync(B.info + 3, 0xff, 8, d.st));
        launch_blk_orbit(in, L, B.nxt, B.hop, B.entry, B.rowbase, B.rowsent, B.info + 3, B.info, d.st);
        unsigned long long info[4] = {0, 0, 0, 0};
        HIP_CHECK(hipMemcpyAsync(info, B.info, 32, hipMemcpyDeviceToHost, d.st));
        HIP_CHECK(hipStreamSynchronize(d.st));
        if (info[3] != ~0ull) {  // (a sentence of the call: what the open row holds fitted a row of this L before)
          const unsigned long long s = info[3] - m;
          unsigned long long o2[2] = {0, 0};
          HIP_CHECK(hipMemcpyAsync(o2, off + s, 16, hipMemcpyDeviceToHost, d.st));
          HIP_CHECK(hipStreamSynchronize(d.st));
          return Status(1, "seq_len is smaller than " + std::string(what) + " " + std::to_string(first_index + s) + ": whole mode places every sentence whole. Current value: seq_len = " +
                               std::to_string(L) + "; length = " + std::to_string(o2[1] - o2[0]) + ";");
        }
        rows = info[0];
        if (info[1] != L && info[1] != 0) {
          rows--;
          rest = info[1];
        }
        rowsent = B.rowsent;
      } else {
        rows = total / L;
        rest = total % L;
      }
    }
    const unsigned long long n_rows = rows + (rest && p.tail == 0 ? 1 : 0);
    if (n_rows > 0x7fffffffull / L)
      return Status(1, "blocks: " + std::to_string(n_rows) + " rows of " + std::to_string(L) + " ids exceed 2^31 - 1 elements: pack fewer sentences per call");
    // ---- from here on the call succeeds
    B.valid = false;
    const size_t n_out = (size_t)(n_rows * L);
    unsigned long long n_frags = 0;
    if (n_rows) {
      B.rows.grow(n_out + 4);
      B.seg.grow(n_out + 4);
      B.pos.grow(n_out + 4);
      B.rowsrc.grow((size_t)n_rows + 1);
      const Status s = two_pass_on_lane(
          d, n_rows, B.rowcnt, B.row_frags, nullptr, &n_frags,
          [&](bool write) {
            if (!write) launch_blk_measure(in, B.ne, L, n_rows, rowsent, B.rowcnt, B.rowsrc, d.st);
            else launch_blk_write(in, B.ne, L, n_rows, B.rowsrc, B.row_frags, p.pad, B.rows, B.seg, B.pos, B.frags, d.st);
          },
          no_check, [&](unsigned long long need) { B.frags.grow((size_t)need * 2 + 2); });
      if (!s.ok()) return s;
    } else {
      B.row_frags.grow(1);
      HIP_CHECK(hipMemsetAsync(B.row_frags, 0, 8, d.st));
    }
    if (rest && p.tail == 1) {  // the incomplete row into the other generation, which then is the open row
      const int g = B.gen ^ 1;
      B.open_ids[g].grow((size_t)rest);
      B.open_off[g].grow((size_t)rest + 1);
      launch_blk_keep(in, B.ne, total - rest, B.open_ids[g], B.open_off[g], B.info, d.st);
      unsigned long long m_new = 0;
      HIP_CHECK(hipMemcpyAsync(&m_new, B.info + 2, 8, hipMemcpyDeviceToHost, d.st));
      HIP_CHECK(hipStreamSynchronize(d.st));
      B.gen = g;
      B.open_f = rest;
      B.open_m = m_new;
      B.open_L = L;
      B.open_mode = p.mode;
    } else {
      B.open_f = B.open_m = 0;
    }
    ev.stop();
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
    B.n_rows = n_rows;
    B.n_frags = n_frags;
    B.L = L;
    B.valid = true;
    if (n_rows_out) *n_rows_out = n_rows;
    if (n_frags_out) *n_frags_out = n_frags;
    return Status();
  });
}

Status BaseEncoder::blocks_device(unsigned long long n_sent, unsigned long long seq_len, int mode, int32_t pad_value, int tail, unsigned long long *n_rows,
                                  unsigned long long *n_frags, double *kernel_ms) const {
  if (n_rows) *n_rows = 0;
  if (n_frags) *n_frags = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(1, "blocks_device: no matching encode result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.res.made || n_sent != d.res.n_sent) return Status(1, "blocks_device: no matching encode result");  // (before any work: the slot stays)
  return blocks_on_lane(*dev_, d, device_, d.res.ids, d.res.off, n_sent, n_sent ? d.res.n_ids : 0, BlkParams{seq_len, mode, pad_value, tail}, "sentence", 0,
                        n_rows, n_frags, kernel_ms);
}

Status BaseEncoder::blocks_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, unsigned long long seq_len,
                                      int mode, int32_t pad_value, int tail, unsigned long long *n_rows, unsigned long long *n_frags, double *kernel_ms) const {
  if (n_rows) *n_rows = 0;
  if (n_frags) *n_frags = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  if (((uintptr_t)d_ids & 3u) != 0) return Status(2, "blocks_ids_device: the ids must be 4-byte aligned");
  if (((uintptr_t)d_offsets & 7u) != 0) return Status(2, "blocks_ids_device: the offsets must be 8-byte aligned");
  const Lane0 l(*dev_);
  return blocks_on_lane(*dev_, l.d, device_, (const int32_t *)d_ids, (const unsigned long long *)d_offsets, n_sent, n_sent ? n_ids : 0,
                        BlkParams{seq_len, mode, pad_value, tail}, "sentence", 0, n_rows, n_frags, kernel_ms);
}

// the open row as a result of 0 or 1 rows: a call without sentences under the open row's own (L, mode), its tail padded
Status BaseEncoder::blocks_flush(int32_t pad_value, unsigned long long *n_rows, unsigned long long *n_frags, double *kernel_ms) const {
  if (n_rows) *n_rows = 0;
  if (n_frags) *n_frags = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  const Lane0 l(*dev_);
  const auto &B = dev_->blk;
  const BlkParams p{B.open_f ? B.open_L : (B.valid && B.L ? B.L : 1), B.open_f ? B.open_mode : 0, pad_value, 0};
  return blocks_on_lane(*dev_, l.d, device_, nullptr, nullptr, 0, 0, p, "sentence", 0, n_rows, n_frags, kernel_ms);
}

void BaseEncoder::blocks_open(unsigned long long out[3]) const {
  out[0] = out[1] = out[2] = 0;
  if (!dev_) return;
  const Lane0 l(*dev_);
  const auto &B = dev_->blk;
  if (!B.open_f) return;
  out[0] = B.open_f;
  out[1] = B.open_L;
  out[2] = (unsigned long long)B.open_mode;
}

void BaseEncoder::blocks_discard() const {
  if (!dev_) return;
  const Lane0 l(*dev_);
  dev_->blk.open_f = dev_->blk.open_m = 0;
}

Status BaseEncoder::take_blocks(void *rows, void *seg, void *pos, void *frags, void *row_frags, unsigned long long n_rows, unsigned long long n_frags,
                                bool to_device) const {
  const char *who = to_device ? "copy_blocks: no matching blocks" : "fetch_blocks: no matching blocks";
  if (!dev_) return Status(1, who);
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  const auto &B = dev_->blk;
  if (!B.valid || n_rows != B.n_rows || n_frags != B.n_frags) return Status(1, who);
  return on_device(device_, [&]() -> Status {
    const size_t mat = (size_t)(B.n_rows * B.L) * 4;
    auto take = [&](void *dst, const void *src, size_t bytes) {
      if (!dst || !bytes) return;
      if (to_device) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, d.st));
      else copy_down(device_, dst, src, bytes, d.st);
    };
    take(rows, B.rows, mat);
    take(seg, B.seg, mat);
    take(pos, B.pos, mat);
    take(frags, B.frags, (size_t)B.n_frags * 8);
    take(row_frags, B.row_frags, ((size_t)B.n_rows + 1) * 8);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// ---- batches by length under a token budget (k_batches.h) ------------------------------------------------------------------------------------
// The plan: keys -> the passes of the sort -> the cuts.  What can refuse the call (the parameters, a negative length, a kept sentence longer than
// max_tokens) is known after the key pass, which writes a working array only; from there on the call succeeds and the slot is rewritten.
Status plan_on_lane(EncoderDevice &D, EncodeLane &d, int device, const BatIn &in, const BatParams &p, unsigned long long *n_kept_out,
                    unsigned long long *n_batches_out, double *kernel_ms) {
  if (n_kept_out) *n_kept_out = 0;
  if (n_batches_out) *n_batches_out = 0;
  if (kernel_ms) *kernel_ms = 0;
  auto &B = D.bat;
  const unsigned long long n = in.n, lim = 0x7fffffffull;
  if (p.T < 1 || p.T > lim) return Status(1, "batches: max_tokens must be within 1 .. 2^31 - 1 (" + std::to_string(p.T) + ")");
  if (p.M > lim) return Status(1, "batches: max_sentences must be 0 (no limit) or within 1 .. 2^31 - 1 (" + std::to_string(p.M) + ")");
  if (n >= 0xfffffffeull) return Status(1, "batches: too many sentences for one call");
  if (n && !in.off && !in.len) return Status(2, "batches: no lengths");
  const BatRule r{p.T, p.M, p.min_len, p.max_len, p.max_len && p.max_len < p.T ? p.max_len : p.T};
  return on_device(device, [&]() -> Status {
    EventPair ev(d.st, kernel_ms != nullptr);
    ev.start();
    unsigned long long info[3] = {~0ull, 0, 0};
    if (n) {
      B.key.grow((size_t)n);
      B.info.grow(4);
      HIP_CHECK(hipMemsetAsync(B.info, 0xff, 8, d.st));
      HIP_CHECK(hipMemsetAsync(B.info + 1, 0, 24, d.st));
      launch_bat_keys(in, r, B.key, B.info, d.st);
      HIP_CHECK(hipMemcpyAsync(info, B.info, 16, hipMemcpyDeviceToHost, d.st));
      HIP_CHECK(hipStreamSynchronize(d.st));
      if (info[0] != ~0ull) {
        const unsigned long long i = info[0];
        if (in.off) {
          unsigned long long o2[2] = {0, 0};
          HIP_CHECK(hipMemcpyAsync(o2, in.off + i, 16, hipMemcpyDeviceToHost, d.st));
          HIP_CHECK(hipStreamSynchronize(d.st));
          info[2] = o2[1] - o2[0];
        } else {
          int32_t l = 0;
          HIP_CHECK(hipMemcpyAsync(&l, in.len + i, 4, hipMemcpyDeviceToHost, d.st));
          HIP_CHECK(hipStreamSynchronize(d.st));
          if (l < 0) return Status(1, "batches: sentence " + std::to_string(i) + " has a negative length (" + std::to_string(l) + ")");
          info[2] = (unsigned long long)l;
        }
        return Status(1, "max_tokens is smaller than sentence " + std::to_string(i) + ": no batch holds it. Current value: max_tokens = " + std::to_string(p.T) +
                             "; length = " + std::to_string(info[2]) + ";");
      }
    }
    // ---- from here on the call succeeds
    const unsigned long long n_kept = info[1];
    unsigned long long n_batches = 0;
    B.planned = B.gathered = false;
    B.order.grow((size_t)n);
    if (n) {
      const unsigned int passes = bat_passes(r.cap);
      const size_t nh = (size_t)(256 * bat_tiles(n));
      B.hist.grow(nh);
      B.hist_off.grow(nh);
      d.k5.scan_tmp.grow((size_t)scan_scratch_blocks(nh));
      if (passes > 1) {
        B.key1.grow((size_t)n);
        B.idx1.grow((size_t)n);
      }
      if (passes > 2) {
        B.key2.grow((size_t)n);
        B.idx2.grow((size_t)n);
      }
      const uint32_t *key_in = B.key, *idx_in = nullptr;  // (the keys of the key pass stay: the cuts read them through the order)
      for (unsigned int k = 0; k < passes; k++) {
        const bool last = k + 1 == passes;
        uint32_t *key_out = last ? nullptr : (k & 1) ? B.key2.p : B.key1.p, *idx_out = last ? B.order.p : (k & 1) ? B.idx2.p : B.idx1.p;
        launch_bat_sort_pass(key_in, idx_in, n, 8 * k, B.hist, B.hist_off, d.k5.scan_tmp, d.k5.total, key_out, idx_out, d.st);
        key_in = key_out;
        idx_in = idx_out;
      }
    }
    if (n_kept) {
      const unsigned int orbit = bat_orbit_positions();
      const size_t nb = (size_t)((n_kept + orbit - 1) / orbit);
      B.skey.grow((size_t)n_kept);
      B.nxt.grow((size_t)n_kept);
      B.hop.grow((size_t)n_kept);
      B.entry.grow(nb);
      B.base.grow(nb);
      B.batch_first.grow((size_t)n_kept + 1);
      HIP_CHECK(hipMemsetAsync(B.entry, 0xff, nb * 4, d.st));
      launch_bat_cuts(B.key, B.order, n_kept, r, orbit, B.skey, B.nxt, B.hop, B.entry, B.base, B.batch_first, B.info, d.st);
      HIP_CHECK(hipMemcpyAsync(&n_batches, B.info + 2, 8, hipMemcpyDeviceToHost, d.st));
    } else {
      B.batch_first.grow(1);
      HIP_CHECK(hipMemsetAsync(B.batch_first, 0, 8, d.st));
    }
    ev.stop();
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
    B.n = n;
    B.n_kept = n_kept;
    B.n_batches = n_batches;
    B.n_elems = 0;
    B.planned = true;
    if (n_kept_out) *n_kept_out = n_kept;
    if (n_batches_out) *n_batches_out = n_batches;
    return Status();
  });
}

// The gather: measure -> scan -> write.  The measure pass writes working arrays; they become the gathered part once the size limit has passed.
Status gather_on_lane(EncoderDevice &D, EncodeLane &d, int device, const int32_t *ids, const unsigned long long *off, unsigned long long n_sent,
                      int32_t pad, bool left_pad, unsigned long long *n_elems_out, double *kernel_ms) {
  if (n_elems_out) *n_elems_out = 0;
  if (kernel_ms) *kernel_ms = 0;
  auto &B = D.bat;
  if (!B.planned) return Status(1, "batches: no plan (call yttm_batches_plan_device or yttm_batches_plan_lengths_device first)");
  if (n_sent != B.n) return Status(1, "batches: the plan is of " + std::to_string(B.n) + " sentences, not of " + std::to_string(n_sent));
  if (B.n_kept && !off) return Status(2, "batches: no offsets");
  return on_device(device, [&]() -> Status {
    const BatPlan plan{B.order, B.batch_first, B.n_batches};
    unsigned long long total = 0;
    if (B.n_batches) {
      B.info.grow(4);
      B.w_widths.grow((size_t)B.n_batches);
      HIP_CHECK(hipMemsetAsync(B.info + 3, 0, 8, d.st));
      const Status s = two_pass_on_lane(
          d, B.n_batches, B.cnt, B.w_off, kernel_ms, &total,
          [&](bool write) {
            if (!write) launch_bat_measure(plan, off, B.w_widths, B.cnt, B.info + 3, d.st);
            else if (total) launch_bat_write(plan, ids, off, B.w_widths, B.w_off, total, pad, left_pad, B.out, d.st);
          },
          [&]() -> Status {
            HIP_CHECK(hipMemcpyAsync(&total, B.info + 3, 8, hipMemcpyDeviceToHost, d.st));  // (exact; the scan's counts saturate)
            HIP_CHECK(hipStreamSynchronize(d.st));
            if (total > 0x7fffffffull)
              return Status(1, "batches: the gathered batches exceed 2^31 - 1 elements (" + std::to_string(total) + "): plan fewer sentences per call");
            B.gathered = false;  // ---- from here on the call succeeds
            return Status();
          },
          [&](unsigned long long need) { B.out.grow((size_t)need + 4); });
      if (!s.ok()) return s;
      std::swap(B.widths, B.w_widths);
      std::swap(B.batch_off, B.w_off);
    } else {
      B.gathered = false;
      B.batch_off.grow(1);
      HIP_CHECK(hipMemsetAsync(B.batch_off, 0, 8, d.st));
      HIP_CHECK(hipStreamSynchronize(d.st));
    }
    B.n_elems = total;
    B.gathered = true;
    if (n_elems_out) *n_elems_out = total;
    return Status();
  });
}

Status BaseEncoder::batches_plan_device(unsigned long long n_sent, unsigned long long max_tokens, unsigned long long max_sentences, unsigned long long min_len,
                                        unsigned long long max_len, unsigned long long *n_kept, unsigned long long *n_batches, double *kernel_ms) const {
  if (n_kept) *n_kept = 0;
  if (n_batches) *n_batches = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(1, "batches_plan_device: no matching encode result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.res.made || n_sent != d.res.n_sent) return Status(1, "batches_plan_device: no matching encode result");
  return plan_on_lane(*dev_, d, device_, BatIn{n_sent ? d.res.off.p : nullptr, nullptr, n_sent}, BatParams{max_tokens, max_sentences, min_len, max_len}, n_kept,
                      n_batches, kernel_ms);
}

Status BaseEncoder::batches_plan_lengths_device(const void *d_lengths, unsigned long long n_sent, unsigned long long max_tokens, unsigned long long max_sentences,
                                                unsigned long long min_len, unsigned long long max_len, unsigned long long *n_kept,
                                                unsigned long long *n_batches, double *kernel_ms) const {
  if (n_kept) *n_kept = 0;
  if (n_batches) *n_batches = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  if (((uintptr_t)d_lengths & 3u) != 0) return Status(2, "batches_plan_lengths_device: the lengths must be 4-byte aligned");
  const Lane0 l(*dev_);
  return plan_on_lane(*dev_, l.d, device_, BatIn{nullptr, (const int32_t *)d_lengths, n_sent}, BatParams{max_tokens, max_sentences, min_len, max_len}, n_kept,
                      n_batches, kernel_ms);
}

Status BaseEncoder::batches_gather_device(unsigned long long n_sent, int32_t pad_value, bool left_pad, unsigned long long *n_elems, double *kernel_ms) const {
  if (n_elems) *n_elems = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(1, "batches_gather_device: no matching encode result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.res.made || n_sent != d.res.n_sent) return Status(1, "batches_gather_device: no matching encode result");
  return gather_on_lane(*dev_, d, device_, d.res.ids, n_sent ? d.res.off.p : nullptr, n_sent, pad_value, left_pad, n_elems, kernel_ms);
}

Status BaseEncoder::batches_gather_ids_device(const void *d_ids, const void *d_offsets, unsigned long long n_sent, unsigned long long n_ids, int32_t pad_value,
                                              bool left_pad, unsigned long long *n_elems, double *kernel_ms) const {
  if (n_elems) *n_elems = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  if (((uintptr_t)d_ids & 3u) != 0) return Status(2, "batches_gather_ids_device: the ids must be 4-byte aligned");
  if (((uintptr_t)d_offsets & 7u) != 0) return Status(2, "batches_gather_ids_device: the offsets must be 8-byte aligned");
  if (n_ids && !d_ids) return Status(2, "batches: no ids");
  const Lane0 l(*dev_);
  return gather_on_lane(*dev_, l.d, device_, (const int32_t *)d_ids, (const unsigned long long *)d_offsets, n_sent, pad_value, left_pad, n_elems, kernel_ms);
}

Status BaseEncoder::take_batches(void *order, void *batch_first, void *widths, void *batch_off, void *out, unsigned long long n_sent, unsigned long long n_batches,
                                 unsigned long long n_elems, bool to_device) const {
  const char *who = to_device ? "copy_batches: no matching batches" : "fetch_batches: no matching batches";
  if (!dev_) return Status(1, who);
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  const auto &B = dev_->bat;
  if (!B.planned || n_sent != B.n || n_batches != B.n_batches || n_elems != B.n_elems) return Status(1, who);
  if (!B.gathered && (widths || batch_off || out)) return Status(1, who);
  return on_device(device_, [&]() -> Status {
    auto take = [&](void *dst, const void *src, size_t bytes) {
      if (!dst || !bytes) return;
      if (to_device) HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, d.st));
      else copy_down(device_, dst, src, bytes, d.st);
    };
    take(order, B.order, (size_t)B.n * 4);
    take(batch_first, B.batch_first, ((size_t)B.n_batches + 1) * 8);
    take(widths, B.widths, (size_t)B.n_batches * 4);
    take(batch_off, B.batch_off, ((size_t)B.n_batches + 1) * 8);
    take(out, B.out, (size_t)B.n_elems * 4);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

Status BaseEncoder::subword_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                                   unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                                   unsigned long long *n_ids, unsigned long long *n_text_bytes, double *kernel_ms) const {
  if (n_ids) *n_ids = 0;
  if (n_text_bytes) *n_text_bytes = 0;
  StageClock ms(kernel_ms);
  if (n_added_tokens() && !byte_fallback()) return Status(1, SUBWORD_UNDER_ADDED_TOKENS);
  const Status tokens = check_bos_eos(*this, bos, eos);  // (before any work, and before the device check: nothing that was pending is touched)
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && !d_offsets) return Status(2, "subword_device: no offsets");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  Status s = encode_on_lane(*this, *dev_, d, device_, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, n_ids,
                            ms.next());
  if (s.ok()) s = format_on_lane(*this, *dev_, d, device_, d_bytes, d_offsets, reverse, n_text_bytes, ms.next());
  return s;
}

// ---- byte spans (k_spans.h) ----------------------------------------------------------------------------------------------------------------
// For every id K5 left the bytes of its sentence it stands for, made on the device from the ids and the batch's own text in one pass: uint32
// [n_ids][2] in the lane's span slot, beside the ids they belong to.
Status spans_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, const void *d_soff, bool reverse,
                     double *kernel_ms) {
  return on_device(device, [&]() -> Status {
    d.sp.valid = false;
    if (kernel_ms) *kernel_ms = 0;
    const unsigned long long n_sent = d.res.n_sent;
    if (n_sent == 0) {
      d.sp.n_sent = d.sp.n_ids = 0;
      d.sp.valid = true;
      return Status();
    }
    subword_table(enc, D);
    const SubInput in = pending_input(enc, d, d_text, d_soff, reverse);
    d.sp.spans.grow((size_t)d.res.n_ids * 2 + 2);
    EventPair ev(d.st, kernel_ms != nullptr);
    ev.start();
    HIP_CHECK(hipMemsetAsync(d.sp.misc, 0, 4, d.st));
    launch_spans(D.m, in, D.sub_units, (uint32_t)enc.vocab_size(), d.res.n_ids, d.sp.spans, d.sp.misc, d.st);
    ev.stop();
    uint32_t bad = 0;
    HIP_CHECK(hipMemcpyAsync(&bad, d.sp.misc, 4, hipMemcpyDeviceToHost, d.st));
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
    if (bad) return Status(2, "spans: the ids of a sentence do not fit the units of its text");
    d.sp.n_sent = n_sent;
    d.sp.n_ids = d.res.n_ids;
    d.sp.valid = true;
    return Status();
  });
}

Status BaseEncoder::spans_device(const void *d_bytes, const void *d_offsets, unsigned long long n_sent, unsigned long long total_bytes,
                                 unsigned long long max_sentence_bytes, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long *n_ids,
                                 double *kernel_ms) const {
  if (n_ids) *n_ids = 0;
  StageClock ms(kernel_ms);
  if (byte_fallback()) return Status(1, SPANS_UNDER_BYTE_FALLBACK);
  if (n_added_tokens()) return Status(1, SPANS_UNDER_ADDED_TOKENS);
  const Status tokens = check_bos_eos(*this, bos, eos);  // (before any work, and before the device check: nothing that was pending is touched)
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_sent && !d_offsets) return Status(2, "spans_device: no offsets");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  Status s = encode_on_lane(*this, *dev_, d, device_, d_bytes, d_offsets, n_sent, total_bytes, max_sentence_bytes, bos, eos, reverse, dropout_prob, n_ids,
                            ms.next());
  if (s.ok()) s = spans_on_lane(*this, *dev_, d, device_, d_bytes, d_offsets, reverse, ms.next());
  return s;
}

Status BaseEncoder::take_spans(void *spans, unsigned long long n_sent, bool to_device) const {
  const char *who = to_device ? "copy_spans: no matching result" : "fetch_spans: no matching result";
  if (!dev_) return Status(1, who);
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.sp.valid || n_sent != d.sp.n_sent || n_sent != d.res.n_sent || d.sp.n_ids != d.res.n_ids) return Status(1, who);
  if (!spans || !d.sp.n_ids) return Status();
  if (to_device) return copy_out_device(device_, d, spans, d.sp.spans, (size_t)d.sp.n_ids * 8, nullptr, nullptr, n_sent);
  return on_device(device_, [&]() -> Status {
    copy_down(device_, spans, d.sp.spans, (size_t)d.sp.n_ids * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

Status BaseEncoder::copy_spans_padded(void *d_matrix, unsigned long long n_sent, unsigned long long width, unsigned long long *longest) const {
  if (longest) *longest = 0;
  if (!dev_) return Status(1, "copy_spans_padded: no matching result");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.sp.valid || n_sent != d.sp.n_sent || n_sent != d.res.n_sent || d.sp.n_ids != d.res.n_ids) return Status(1, "copy_spans_padded: no matching result");
  if (n_sent == 0) return Status();
  return on_device(device_, [&]() -> Status {
    unsigned long long need = 0;
    const Status fit = longest_row_fits(d, n_sent, width, &need, longest);
    if (!fit.ok()) return fit;
    if (n_sent > (~0ull >> 4) / (width ? width : 1)) return Status(2, "copy_spans_padded: the matrix is too large");
    if (!width) return Status();
    if (!d_matrix) return Status(2, "copy_spans_padded: no output");
    if (((uintptr_t)d_matrix & 7u) != 0) return Status(2, "copy_spans_padded: the matrix must be 8-byte aligned");
    launch_spans_pad(d.sp.spans, d.res.off, n_sent, width, (uint32_t *)d_matrix, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// host to host on one lane: upload -> K5 -> spans -> download, into arrays the caller releases with free()
Status BaseEncoder::encode_as_ids_spans(const uint8_t *bytes, const unsigned long long *offsets, unsigned long long n_sent, bool bos, bool eos, bool reverse,
                                        double dropout_prob, int32_t **ids, unsigned long long **out_off, uint32_t **spans) const {
  *ids = nullptr;
  *out_off = nullptr;
  *spans = nullptr;
  const CfgBind bind(config());
  if (byte_fallback()) return Status(1, SPANS_UNDER_BYTE_FALLBACK);
  if (n_added_tokens()) return Status(1, SPANS_UNDER_ADDED_TOKENS);
  Status s = check_bos_eos(*this, bos, eos);
  if (!s.ok()) return s;
  if (n_sent && !dev_) return Status(2, "encoder has no device state");
  unsigned long long *off = (unsigned long long *)result_alloc((size_t)(n_sent + 1) * 8);
  if (!off) return Status(2, "out of memory");
  off[0] = 0;
  unsigned long long n_ids = 0;
  int32_t *idp = nullptr;
  uint32_t *spp = nullptr;
  if (n_sent) {
    const unsigned long long b0 = offsets[0], total_bytes = offsets[n_sent] - b0;
    unsigned long long max_len = 0;
    std::vector<unsigned long long> rel((size_t)n_sent + 1);  // offsets are rebased to the first byte of the batch
    for (unsigned long long i = 0; i <= n_sent; i++) rel[i] = offsets[i] - b0;
    for (unsigned long long i = 0; i < n_sent; i++) max_len = std::max(max_len, rel[i + 1] - rel[i]);
    std::unique_lock<std::mutex> lk;
    EncodeLane &d = dev_->acquire(lk);  // held until the results are back on the host
    s = on_device(device_, [&]() -> Status {
      d.in.bytes.grow((size_t)total_bytes + 16);
      d.in.off.grow((size_t)n_sent + 1);
      copy_up(device_, d.in.bytes, bytes + b0, (size_t)total_bytes, d.st);
      copy_up(device_, d.in.off, rel.data(), ((size_t)n_sent + 1) * 8, d.st);
      HIP_CHECK(hipStreamSynchronize(d.st));
      return Status();
    });
    if (s.ok()) s = encode_on_lane(*this, *dev_, d, device_, d.in.bytes, d.in.off, n_sent, total_bytes, max_len, bos, eos, reverse, dropout_prob, &n_ids, nullptr);
    if (s.ok()) s = spans_on_lane(*this, *dev_, d, device_, d.in.bytes, d.in.off, reverse, nullptr);
    if (s.ok()) {
      idp = (int32_t *)result_alloc((size_t)(n_ids ? n_ids : 1) * 4);
      spp = (uint32_t *)result_alloc((size_t)(n_ids ? n_ids : 1) * 8);
      if (!idp || !spp) s = Status(2, "out of memory");
    }
    if (s.ok())
      s = on_device(device_, [&]() -> Status {
        if (n_ids) copy_down(device_, idp, d.res.ids, (size_t)n_ids * 4, d.st);
        if (n_ids) copy_down(device_, spp, d.sp.spans, (size_t)n_ids * 8, d.st);
        copy_down(device_, off, d.res.off, (size_t)(n_sent + 1) * 8, d.st);
        HIP_CHECK(hipStreamSynchronize(d.st));
        return Status();
      });
  } else {
    idp = (int32_t *)result_alloc(4);
    spp = (uint32_t *)result_alloc(8);
    if (!idp || !spp) s = Status(2, "out of memory");
  }
  if (!s.ok()) {
    free(idp);
    free(spp);
    free(off);
    return s;
  }
  *ids = idp;
  *out_off = off;
  *spans = spp;
  return Status();
}

}  // namespace yttm
