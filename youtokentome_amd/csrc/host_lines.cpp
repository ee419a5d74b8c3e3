// host_lines.cpp -- host side of the line split (k_lines.h) and the encoder's entries for text that is not yet cut into sentences: a buffer in HBM
// (lines_device, encode_text_device, subword_text_device; decimal id text: ids_parse_device, decode_text_device) and a file of any size
// (encode_file; text to text: encode_file_subword, encode_file_idtext, decode_file), on the encoder's lanes (enc_lanes.h).
//
// The offsets of a split live in the lane like the results of encode_device and decode_device, in buffers of their own: a split leaves a pending
// encode or decode result alone.  Every call locks the lane and returns after the lane's stream has synchronised.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>

#include "enc_lanes.h"

namespace yttm {

// count -> scan -> write -> longest on the lane (locked by the caller).  Throws GpuError.
static void split_on_lane(EncodeLane &d, const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines_out, unsigned long long *longest_out,
                          double *kernel_ms) {
  d.ln.valid = false;
  if (kernel_ms) *kernel_ms = 0;
  unsigned long long n_lines = 0, longest = 0;
  if (n_bytes) {
    const uint8_t *text = (const uint8_t *)d_text;
    EventPair ev(d.st, kernel_ms != nullptr);
    ev.start();
    const unsigned long long n_tiles = lines_tiles(d_text, n_bytes);
    unsigned long long inner = 0;  // newlines in front of the last byte: each one starts a line
    if (n_tiles) {
      d.ln.cnt.grow((size_t)n_tiles);
      d.ln.rank.grow((size_t)n_tiles + 1);
      launch_lines_count(text, n_bytes, d.ln.cnt, d.st);
      inner = scan_counts(d, d.ln.cnt, n_tiles, d.ln.rank);  // (syncs)
    }
    n_lines = inner + 1;
    d.ln.off.grow((size_t)n_lines + 1);
    HIP_CHECK(hipMemsetAsync(d.ln.misc, 0, 8, d.st));
    launch_lines_write(text, n_bytes, d.ln.rank, d.ln.off, n_lines, d.st);
    launch_lines_longest(d.ln.off, n_lines, d.ln.misc, d.st);
    ev.stop();
    HIP_CHECK(hipMemcpyAsync(&longest, d.ln.misc, 8, hipMemcpyDeviceToHost, d.st));
    HIP_CHECK(hipStreamSynchronize(d.st));
    if (kernel_ms) *kernel_ms = ev.elapsed_ms();
  }
  d.ln.n_lines = n_lines;
  d.ln.n_bytes = n_bytes;
  d.ln.longest = longest;
  d.ln.valid = true;
  if (n_lines_out) *n_lines_out = n_lines;
  if (longest_out) *longest_out = longest;
}

Status BaseEncoder::lines_device(const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines, unsigned long long *longest,
                                 double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (longest) *longest = 0;
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_bytes && !d_text) return Status(2, "lines_device: no text");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  return on_device(device_, [&]() -> Status {
    split_on_lane(d, d_text, n_bytes, n_lines, longest, kernel_ms);
    return Status();
  });
}

// the offsets of the last lines_device / encode_text_device: to a host array (to_device == false) or to device memory the caller owns
Status BaseEncoder::take_lines(void *offsets, unsigned long long n_lines, bool to_device) const {
  const char *who = to_device ? "copy_lines: no matching result" : "fetch_lines: no matching result";
  if (!dev_) return Status(2, who);
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  if (!d.ln.valid || n_lines != d.ln.n_lines) return Status(2, who);
  if (!offsets) return Status();
  if (to_device) return copy_out_device(device_, d, nullptr, nullptr, 0, offsets, d.ln.off, n_lines);
  return on_device(device_, [&]() -> Status {
    if (n_lines == 0) *(unsigned long long *)offsets = 0;  // (nothing was launched: the one offset is 0)
    else copy_down(device_, offsets, d.ln.off, (size_t)(n_lines + 1) * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
}

// split, then the batch encoder on the lane's own offsets: the lines keep their newline, which is white space to the encoder
static Status encode_text_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, unsigned long long n_bytes, bool bos,
                                  bool eos, bool reverse, double dropout_prob, unsigned long long *n_lines, unsigned long long *n_ids, double *split_ms,
                                  double *encode_ms) {
  Status s = check_bos_eos(enc, bos, eos);  // (before any work, as every encode entry does)
  if (!s.ok()) return s;
  unsigned long long nl = 0, longest = 0;
  s = on_device(device, [&]() -> Status {
    split_on_lane(d, d_text, n_bytes, &nl, &longest, split_ms);
    return Status();
  });
  if (!s.ok()) return s;
  if (n_lines) *n_lines = nl;
  return encode_on_lane(enc, D, d, device, d_text, d.ln.off, nl, n_bytes, longest, bos, eos, reverse, dropout_prob, n_ids, encode_ms);
}

Status BaseEncoder::encode_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                                       unsigned long long *n_lines, unsigned long long *n_ids, double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (n_ids) *n_ids = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");  // (this entry alone asks for the device first: bos / eos are checked on the lane)
  if (n_bytes && !d_text) return Status(2, "encode_text_device: no text");
  const Lane0 l(*dev_);
  double *const ms_split = ms.next(), *const ms_enc = ms.next();
  return encode_text_on_lane(*this, *dev_, l.d, device_, d_text, n_bytes, bos, eos, reverse, dropout_prob, n_lines, n_ids, ms_split, ms_enc);
}

// split, encode, then the SUBWORD text of those ids (host_decode.cpp): the lines' offsets are the formatter's sentence offsets
static Status subword_text_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, unsigned long long n_bytes, bool bos,
                                   bool eos, bool reverse, double dropout_prob, unsigned long long *n_lines, unsigned long long *n_ids,
                                   unsigned long long *n_text_bytes, double *split_ms, double *encode_ms, double *format_ms) {
  const Status s = encode_text_on_lane(enc, D, d, device, d_text, n_bytes, bos, eos, reverse, dropout_prob, n_lines, n_ids, split_ms, encode_ms);
  if (!s.ok()) return s;
  return format_on_lane(enc, D, d, device, d_text, d.ln.off, reverse, n_text_bytes, format_ms);
}

Status BaseEncoder::subword_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                                        unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes, double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (n_ids) *n_ids = 0;
  if (n_text_bytes) *n_text_bytes = 0;
  StageClock ms(kernel_ms);
  if (n_added_tokens() && !byte_fallback()) return Status(1, SUBWORD_UNDER_ADDED_TOKENS);
  const Status tokens = check_bos_eos(*this, bos, eos);  // (before any work, and before the device check: nothing that was pending is touched)
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_bytes && !d_text) return Status(2, "subword_text_device: no text");
  const Lane0 l(*dev_);
  double *const ms_split = ms.next(), *const ms_enc = ms.next(), *const ms_fmt = ms.next();
  return subword_text_on_lane(*this, *dev_, l.d, device_, d_text, n_bytes, bos, eos, reverse, dropout_prob, n_lines, n_ids, n_text_bytes, ms_split, ms_enc,
                              ms_fmt);
}

// split, encode, then the byte spans of those ids (host_decode.cpp): a sentence is a line with its newline, the spans count from the line's start
Status BaseEncoder::spans_text_device(const void *d_text, unsigned long long n_bytes, bool bos, bool eos, bool reverse, double dropout_prob,
                                      unsigned long long *n_lines, unsigned long long *n_ids, double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (n_ids) *n_ids = 0;
  StageClock ms(kernel_ms);
  if (byte_fallback()) return Status(1, SPANS_UNDER_BYTE_FALLBACK);
  if (n_added_tokens()) return Status(1, SPANS_UNDER_ADDED_TOKENS);
  const Status tokens = check_bos_eos(*this, bos, eos);  // (before any work, and before the device check: nothing that was pending is touched)
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_bytes && !d_text) return Status(2, "spans_text_device: no text");
  const Lane0 l(*dev_);
  EncodeLane &d = l.d;
  double *const ms_split = ms.next(), *const ms_enc = ms.next();
  Status s = encode_text_on_lane(*this, *dev_, d, device_, d_text, n_bytes, bos, eos, reverse, dropout_prob, n_lines, n_ids, ms_split, ms_enc);
  if (s.ok()) s = spans_on_lane(*this, *dev_, d, device_, d_text, d.ln.off, reverse, ms.next());
  return s;
}

// ---- decimal id text (k_idtext.h) ----------------------------------------------------------------------------------------------------------
// The ids `while (ss >> x) ids.push_back(x)` reads from every line of the split pending on the lane (bpe.cpp:1863-1873), left in the lane's
// encode-result buffers exactly as encode_on_lane leaves its ids, n_sent = the lines: measure -> scan -> write.
static Status parse_on_lane(EncodeLane &d, int device, const void *d_text, unsigned long long n_bytes, unsigned long long *n_ids_out, double *kernel_ms) {
  return on_device(device, [&]() -> Status {
    const unsigned long long n_lines = d.ln.n_lines;
    d.res.n_sent = n_lines;
    d.res.n_ids = 0;
    d.res.made = true;
    d.sp.valid = false;  // (spans belong to the ids they were made from)
    if (n_ids_out) *n_ids_out = 0;
    if (kernel_ms) *kernel_ms = 0;
    if (n_lines == 0) return Status();
    unsigned long long total = 0;
    const Status s = two_pass_on_lane(
        d, n_lines, d.k5.counts, d.res.off, kernel_ms, &total,
        [&](bool write) { launch_idparse(write, (const uint8_t *)d_text, d.ln.off, n_lines, n_bytes, d.k5.counts, d.res.off, d.res.ids, d.st); },
        [] { return Status(); }, [&](unsigned long long need) { d.res.ids.grow((size_t)need + 1); });
    if (!s.ok()) return s;
    d.res.n_ids = total;
    if (n_ids_out) *n_ids_out = total;
    return Status();
  });
}

// split, then the parse of those lines
static Status parse_text_on_lane(EncodeLane &d, int device, const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines,
                                 unsigned long long *n_ids, double *split_ms, double *parse_ms) {
  unsigned long long nl = 0;
  const Status s = on_device(device, [&]() -> Status {
    split_on_lane(d, d_text, n_bytes, &nl, nullptr, split_ms);
    return Status();
  });
  if (!s.ok()) return s;
  if (n_lines) *n_lines = nl;
  return parse_on_lane(d, device, d_text, n_bytes, n_ids, parse_ms);
}

// split, parse, then the device decode of those ids with a newline behind every line: what decode_cli writes for the text (bpe.cpp:2016-2028)
static Status decode_text_on_lane(const BaseEncoder &enc, EncoderDevice &D, EncodeLane &d, int device, const void *d_text, unsigned long long n_bytes,
                                  const int32_t *ignore_ids, unsigned long long n_ignore, unsigned long long *n_lines, unsigned long long *n_ids,
                                  unsigned long long *n_text_bytes, double *split_ms, double *parse_ms, double *decode_ms) {
  unsigned long long nl = 0, ni = 0;
  const Status s = parse_text_on_lane(d, device, d_text, n_bytes, &nl, &ni, split_ms, parse_ms);
  if (!s.ok()) return s;
  if (n_lines) *n_lines = nl;
  if (n_ids) *n_ids = ni;
  const DecInput in{d.res.ids, d.res.off, nullptr, 0, 0, nl};
  return decode_on_lane(enc, D, d, device, in, ni, ignore_ids, n_ignore, n_text_bytes, decode_ms, true);
}

Status BaseEncoder::ids_parse_device(const void *d_text, unsigned long long n_bytes, unsigned long long *n_lines, unsigned long long *n_ids,
                                     double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (n_ids) *n_ids = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_bytes && !d_text) return Status(2, "ids_parse_device: no text");
  const Lane0 l(*dev_);
  double *const ms_split = ms.next(), *const ms_parse = ms.next();
  return parse_text_on_lane(l.d, device_, d_text, n_bytes, n_lines, n_ids, ms_split, ms_parse);
}

Status BaseEncoder::decode_text_device(const void *d_text, unsigned long long n_bytes, const int32_t *ignore_ids, unsigned long long n_ignore,
                                       unsigned long long *n_lines, unsigned long long *n_ids, unsigned long long *n_text_bytes, double *kernel_ms) const {
  if (n_lines) *n_lines = 0;
  if (n_ids) *n_ids = 0;
  if (n_text_bytes) *n_text_bytes = 0;
  StageClock ms(kernel_ms);
  if (!dev_) return Status(2, "encoder has no device state");
  if (n_bytes && !d_text) return Status(2, "decode_text_device: no text");
  if (n_ignore && !ignore_ids) return Status(2, "decode_text_device: no ignore_ids");
  const Lane0 l(*dev_);
  double *const ms_split = ms.next(), *const ms_parse = ms.next(), *const ms_dec = ms.next();
  return decode_text_on_lane(*this, *dev_, l.d, device_, d_text, n_bytes, ignore_ids, n_ignore, n_lines, n_ids, n_text_bytes, ms_split, ms_parse, ms_dec);
}

// ---- a file of any size ------------------------------------------------------------------------------------------------------------------
// The file crosses in pieces of about piece_bytes, each cut behind the last newline inside it (a line longer than a piece extends the piece
// to that line's end), through both lanes: while piece k is split and encoded, piece k + 1 is read (pread into the pinned chunks of
// staged_transfer) and uploaded and the ids of piece k - 1 come down (run_two_lanes).  The result is appended in file
// order, the pieces' offsets moved behind the ids so far; it does not depend on the cuts (no word and no line crosses one).
constexpr unsigned long long FILE_PIECE_DEFAULT = 256ull << 20;

namespace {
struct Fd {
  int fd = -1;
  ~Fd() { if (fd >= 0) close(fd); }
};
// end of the piece that starts at pos: behind the last newline of [pos, pos + want), else behind the first one after it, else the file's end
bool piece_end(int fd, unsigned long long pos, unsigned long long want, unsigned long long size, unsigned long long *end) {
  if (size - pos <= want) { *end = size; return true; }
  std::vector<char> buf(1u << 16);
  auto read_at = [&](unsigned long long at, size_t len) {
    size_t got = 0;
    while (got < len) {
      const ssize_t r = pread(fd, buf.data() + got, len - got, (off_t)(at + got));
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) return false;
      got += (size_t)r;
    }
    return true;
  };
  for (unsigned long long hi = pos + want; hi > pos;) {  // backwards
    const size_t len = (size_t)std::min<unsigned long long>(buf.size(), hi - pos);
    if (!read_at(hi - len, len)) return false;
    if (const void *p = memrchr(buf.data(), '\n', len)) { *end = hi - len + (unsigned long long)((const char *)p - buf.data()) + 1; return true; }
    hi -= len;
  }
  for (unsigned long long lo = pos + want; lo < size;) {  // the line is longer than the piece: forwards
    const size_t len = (size_t)std::min<unsigned long long>(buf.size(), size - lo);
    if (!read_at(lo, len)) return false;
    if (const void *p = memchr(buf.data(), '\n', len)) { *end = lo + (unsigned long long)((const char *)p - buf.data()) + 1; return true; }
    lo += len;
  }
  *end = size;
  return true;
}
bool pwrite_all(int fd, const void *p, size_t n, unsigned long long at) {
  const char *c = (const char *)p;
  while (n) {
    const ssize_t w = pwrite(fd, c, n, (off_t)at);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    c += w;
    n -= (size_t)w;
    at += (unsigned long long)w;
  }
  return true;
}
// The piece that starts at pos (piece_end) from the file into the lane's input buffer: pread into the pinned chunks of staged_transfer.
Status upload_piece(int fd, const std::string &path, int device, EncodeLane &d, unsigned long long pos, unsigned long long piece_bytes,
                    unsigned long long size, unsigned long long *end_out) {
  unsigned long long end = size;
  if (!piece_end(fd, pos, piece_bytes, size, &end)) return Status(1, "Failed to read file: " + path);
  const unsigned long long nb = end - pos;
  d.in.bytes.grow((size_t)nb + 16);
  std::atomic<bool> read_ok{true};
  try {
    staged_transfer(device, d.in.bytes, nb, true, [&](void *chunk, unsigned long long o, size_t len) {
      size_t got = 0;
      while (got < len) {
        const ssize_t r = pread(fd, (char *)chunk + got, len - got, (off_t)(pos + o + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { read_ok.store(false); return false; }  // (an error, or the file shrank)
        got += (size_t)r;
      }
      return true;
    });
  } catch (const GpuError &) {
    if (!read_ok.load()) return Status(1, "Failed to read file: " + path);
    throw;
  }
  *end_out = end;
  return Status();
}
// A result array that is filled as the pieces arrive.  Its size is not known before the last piece; `hint` is the caller's estimate of the
// whole from the pieces so far, so that a file of even lines is one allocation (result_alloc: huge pages for a large one, the first touch of
// 4 KB pages costs more than the copy that does the touching) and only a misjudged one is moved.
template <class T>
struct Growing {
  T *p = nullptr;
  size_t cap = 0, used = 0;
  bool need(size_t n, size_t hint) {
    if (n <= cap) return true;
    const size_t c = std::max(std::max(n, hint), cap + cap / 2);  // (geometric at least: a file whose lines grow is not copied once per piece)
    T *q = (T *)result_alloc(c * sizeof(T));
    if (!q) return false;
    if (used) memcpy(q, p, used * sizeof(T));
    free(p);
    p = q;
    cap = c;
    return true;
  }
  ~Growing() { free(p); }
};

double secs_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); }

// What the file entries share: the input, the upload leg of run_two_lanes and the record of the piece in flight on each lane -- upload(i) fills
// it, the entry's work(i) adds the counts (and kernel times in milliseconds: the split, two more named by the route), its download(i) reads it.
struct FilePieces {
  struct Piece {
    unsigned long long pos = 0, bytes = 0, n_lines = 0, n_ids = 0, n_text = 0;
    double ms_split = 0, ms_a = 0, ms_b = 0;
  } piece[2];
  const std::string &path;
  EncoderDevice *const dev;
  const int device;
  const unsigned long long piece_bytes;
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  Fd in;
  struct stat sb;
  unsigned long long size = 0, next_pos = 0;
  double s_up = 0;
  FilePieces(const std::string &input, EncoderDevice *D, int dev_id, unsigned long long want)
      : path(input), dev(D), device(dev_id), piece_bytes(want ? want : FILE_PIECE_DEFAULT) {}
  Status open_input() {
    in.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (in.fd < 0 || fstat(in.fd, &sb) != 0) return Status(1, "Failed to open file: " + path + " (" + strerror(errno) + ")");
    if (!S_ISREG(sb.st_mode)) return Status(1, "Failed to read file: " + path + " is not a regular file");
    size = (unsigned long long)sb.st_size;
    return Status();
  }
  Status upload(size_t i, bool *exhausted) {
    const unsigned long long pos = next_pos;
    if (pos >= size) { *exhausted = true; return Status(); }
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long end = size;
    const Status st = upload_piece(in.fd, path, device, dev->lane[i & 1], pos, piece_bytes, size, &end);
    if (!st.ok()) return st;
    s_up += secs_since(t0);
    piece[i & 1] = Piece{};
    piece[i & 1].pos = pos;
    piece[i & 1].bytes = end - pos;
    next_pos = end;
    return Status();
  }
  // the report of a finished call: text_bytes only for the text routes, `stages` the route's own kernel seconds behind the encode's
  std::string report(size_t n_pieces, unsigned long long lines, unsigned long long ids, const unsigned long long *text_bytes, double s_split, double s_enc,
                     std::initializer_list<std::pair<const char *, double>> stages, double s_down) const {
    char tmp[512];
    snprintf(tmp, sizeof tmp, "{\"pieces\": %zu, \"piece_bytes\": %llu, \"bytes\": %llu, \"lines\": %llu, \"ids\": %llu, ", n_pieces, piece_bytes, size, lines, ids);
    std::string r = tmp;
    if (text_bytes) {
      snprintf(tmp, sizeof tmp, "\"text_bytes\": %llu, ", *text_bytes);
      r += tmp;
    }
    snprintf(tmp, sizeof tmp, "\"seconds_total\": %.6f, \"seconds_read_upload\": %.6f, \"seconds_split\": %.6f, \"seconds_encode\": %.6f", secs_since(t_begin), s_up,
             s_split, s_enc);
    r += tmp;
    for (const auto &st : stages) {
      if (!st.first) continue;
      snprintf(tmp, sizeof tmp, ", \"%s\": %.6f", st.first, st.second);
      r += tmp;
    }
    snprintf(tmp, sizeof tmp, ", \"seconds_download_write\": %.6f}", s_down);
    return r + tmp;
  }
};
}  // namespace

Status BaseEncoder::encode_file(const std::string &path, const char *out_prefix, bool bos, bool eos, bool reverse, double dropout_prob,
                                unsigned long long piece_bytes, int32_t **ids_out, unsigned long long **off_out, unsigned long long *n_lines_out,
                                unsigned long long *n_ids_out, std::string *report) const {
  if (ids_out) *ids_out = nullptr;
  if (off_out) *off_out = nullptr;
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  const Status tokens = check_bos_eos(*this, bos, eos);
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (!out_prefix && (!ids_out || !off_out)) return Status(2, "encode_file: no output");
  FilePieces fp(path, dev_, device_, piece_bytes);
  const Status opened = fp.open_input();
  if (!opened.ok()) return opened;
  const unsigned long long size = fp.size;
  Fd out_ids, out_off;
  std::string ids_path, off_path;
  if (out_prefix) {
    ids_path = std::string(out_prefix) + ".ids";
    off_path = std::string(out_prefix) + ".off";
    out_ids.fd = open(ids_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (out_ids.fd < 0) return Status(1, "Failed to open file for writing: " + ids_path + " (" + strerror(errno) + ")");
    out_off.fd = open(off_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (out_off.fd < 0) return Status(1, "Failed to open file for writing: " + off_path + " (" + strerror(errno) + ")");
  }
  const std::shared_ptr<const Config> C = dev_->cfg;
  const CfgBind bind(C);
  const int device = device_;
  EncoderDevice *dev = dev_;
  std::lock_guard<std::mutex> lk0(dev->lane[0].mu), lk1(dev->lane[1].mu);  // (lane 0 first, always: nobody else waits for two lanes)

  double s_split = 0, s_enc = 0, s_down = 0;
  Growing<int32_t> ids;
  Growing<unsigned long long> off;
  unsigned long long lines_total = 0, ids_total = 0;  // (the download leg's)

  auto upload = [&](size_t i, bool *exhausted) { return fp.upload(i, exhausted); };
  auto work = [&](size_t i) {
    FilePieces::Piece &p = fp.piece[i & 1];
    EncodeLane &d = dev->lane[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    const Status st = encode_text_on_lane(*this, *dev, d, device, d.in.bytes, p.bytes, bos, eos, reverse, dropout_prob, &p.n_lines, &p.n_ids, &p.ms_split, nullptr);
    s_split += p.ms_split * 1e-3;
    s_enc += secs_since(t0) - p.ms_split * 1e-3;
    return st;
  };
  auto download = [&](size_t i) {
    const FilePieces::Piece p = fp.piece[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    EncodeLane &d = dev->lane[i & 1];
    const unsigned long long ids_base = ids_total, lines_base = lines_total;
    std::atomic<bool> write_ok{true};
    if (!out_prefix) {  // room for this piece, asked for at what the pieces so far say about the whole file
      const double whole = (double)size / (double)(p.pos + p.bytes) * 1.03;
      ids.used = (size_t)ids_base;
      off.used = (size_t)lines_base + (lines_base ? 1 : 0);
      if (!ids.need((size_t)(ids_base + p.n_ids) + 1, (size_t)((double)(ids_base + p.n_ids) * whole) + 1024) ||
          !off.need((size_t)(lines_base + p.n_lines) + 1, (size_t)((double)(lines_base + p.n_lines) * whole) + 1024))
        return Status(2, "out of memory");
    }
    try {
      if (p.n_ids)
        staged_transfer(device, (uint8_t *)d.res.ids.p, p.n_ids * 4, false, [&](void *chunk, unsigned long long o, size_t len) {
          if (!out_prefix) { memcpy((uint8_t *)(ids.p + ids_base) + o, chunk, len); return true; }
          if (!pwrite_all(out_ids.fd, chunk, len, ids_base * 4 + o)) { write_ok.store(false); return false; }
          return true;
        }, nullptr, ENC_CHUNK);
      // (the piece's offsets start at 0: moved behind the ids so far; its last entry is the next piece's first, written twice, the same)
      if (p.n_lines)
        staged_transfer(device, (uint8_t *)d.res.off.p, (p.n_lines + 1) * 8, false, [&](void *chunk, unsigned long long o, size_t len) {
          unsigned long long *v = (unsigned long long *)chunk;
          if (!out_prefix) {
            unsigned long long *dst = off.p + lines_base + o / 8;
            for (size_t j = 0; j < len / 8; j++) dst[j] = v[j] + ids_base;
            return true;
          }
          for (size_t j = 0; j < len / 8; j++) v[j] += ids_base;
          if (!pwrite_all(out_off.fd, chunk, len, lines_base * 8 + o)) { write_ok.store(false); return false; }
          return true;
        }, nullptr, ENC_CHUNK);
    } catch (const GpuError &) {
      if (!write_ok.load()) return Status(1, "Failed to write file: " + (ids_path.empty() ? std::string("?") : std::string(out_prefix) + ".ids / .off"));
      throw;
    }
    ids_total += p.n_ids;
    lines_total += p.n_lines;
    s_down += secs_since(t0);
    return Status();
  };
  size_t n_pieces = 0;
  const Status piped = run_two_lanes("encode_file", C, device, PIPE_UNTIL_EXHAUSTED, upload, work, download, &n_pieces);
  if (!piped.ok()) return piped;
  if (out_prefix) {
    if (size == 0 || lines_total == 0) {  // (no piece wrote the offsets' first entry)
      const unsigned long long zero = 0;
      if (!pwrite_all(out_off.fd, &zero, 8, 0)) return Status(1, "Failed to write file: " + off_path);
    }
    const int fd_a = out_ids.fd, fd_b = out_off.fd;
    out_ids.fd = out_off.fd = -1;
    const bool ok_a = close(fd_a) == 0, ok_b = close(fd_b) == 0;
    if (!ok_a || !ok_b) return Status(1, "Failed to write file: " + (ok_a ? off_path : ids_path));
  } else {
    if (!ids.need(1, 1) || !off.need(1, 1)) return Status(2, "out of memory");
    if (lines_total == 0) off.p[0] = 0;
    // (what the caller keeps until its yttm_free is the result itself, not the room it grew in)
    if (void *small = realloc(ids.p, std::max<size_t>((size_t)ids_total, 1) * sizeof(int32_t))) ids.p = (int32_t *)small;
    if (void *small = realloc(off.p, ((size_t)lines_total + 1) * sizeof(unsigned long long))) off.p = (unsigned long long *)small;
    *ids_out = ids.p;
    *off_out = off.p;
    ids.p = nullptr;
    off.p = nullptr;
  }
  if (n_lines_out) *n_lines_out = lines_total;
  if (n_ids_out) *n_ids_out = ids_total;
  if (report) *report = fp.report(n_pieces, lines_total, ids_total, nullptr, s_split, s_enc, {}, s_down);
  return Status();
}

// ---- a text file to its token frequencies ------------------------------------------------------------------------------------------------
// The same pipeline with no download leg: piece k is split, encoded and counted (k_idcount.h) into the encoder's counts slot while piece k + 1 is
// read and uploaded; the slot is zeroed first and every piece adds to it -- `work` runs on one thread and ends synchronised, so the lanes never
// add at once --, and counts[vocab_size + 1] is all that comes down.
Status BaseEncoder::encode_file_counts(const std::string &path, bool bos, bool eos, bool reverse, double dropout_prob, unsigned long long piece_bytes,
                                       unsigned long long *counts, unsigned long long *n_lines_out, unsigned long long *n_ids_out, std::string *report) const {
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  const Status tokens = check_bos_eos(*this, bos, eos);
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (!counts) return Status(2, "encode_file_counts: no output");
  FilePieces fp(path, dev_, device_, piece_bytes);
  const Status opened = fp.open_input();
  if (!opened.ok()) return opened;
  const std::shared_ptr<const Config> C = dev_->cfg;
  const CfgBind bind(C);
  const int device = device_;
  EncoderDevice *dev = dev_;
  const unsigned long long n_bins = default_bins();  // (the caller's counts hold that many and one more)
  std::lock_guard<std::mutex> lk0(dev->lane[0].mu), lk1(dev->lane[1].mu);  // (lane 0 first, always: nobody else waits for two lanes)

  const Status zeroed = count_on_lane(*dev, dev->lane[0], device, nullptr, 0, n_bins, false, nullptr);  // (an empty file counts nothing into zeroes)
  if (!zeroed.ok()) return zeroed;
  double s_split = 0, s_enc = 0, s_count = 0;
  unsigned long long lines_total = 0, ids_total = 0;
  auto upload = [&](size_t i, bool *exhausted) { return fp.upload(i, exhausted); };
  auto work = [&](size_t i) {
    FilePieces::Piece &p = fp.piece[i & 1];
    EncodeLane &d = dev->lane[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    Status st = encode_text_on_lane(*this, *dev, d, device, d.in.bytes, p.bytes, bos, eos, reverse, dropout_prob, &p.n_lines, &p.n_ids, &p.ms_split, nullptr);
    if (st.ok()) st = count_on_lane(*dev, d, device, d.res.ids, p.n_ids, n_bins, true, &p.ms_a);
    s_split += p.ms_split * 1e-3;
    s_count += p.ms_a * 1e-3;
    s_enc += secs_since(t0) - (p.ms_split + p.ms_a) * 1e-3;
    return st;
  };
  auto download = [&](size_t i) {  // (nothing comes down: the piece's totals, in file order)
    lines_total += fp.piece[i & 1].n_lines;
    ids_total += fp.piece[i & 1].n_ids;
    return Status();
  };
  size_t n_pieces = 0;
  const Status piped = run_two_lanes("encode_file_counts", C, device, PIPE_UNTIL_EXHAUSTED, upload, work, download, &n_pieces);
  if (!piped.ok()) return piped;
  const auto t_down = std::chrono::steady_clock::now();
  const Status down = on_device(device, [&]() -> Status {
    EncodeLane &d = dev->lane[0];
    copy_down(device, counts, dev->idc.counts, ((size_t)n_bins + 1) * 8, d.st);
    HIP_CHECK(hipStreamSynchronize(d.st));
    return Status();
  });
  if (!down.ok()) return down;
  if (n_lines_out) *n_lines_out = lines_total;
  if (n_ids_out) *n_ids_out = ids_total;
  if (report) *report = fp.report(n_pieces, lines_total, ids_total, nullptr, s_split, s_enc, {{"seconds_count", s_count}}, secs_since(t_down));
  return Status();
}

// ---- a text file to a text file ---------------------------------------------------------------------------------------------------------
// The same pipeline with text as the only thing that comes down: piece k's text, left in the lane's text slot by `work`, is written to out_path
// behind the text of the pieces before it.  Three routes share it: the SUBWORD formatter and the id printer behind the encode, and the decode
// of a file of decimal ids.
namespace {
struct TextRoute {
  const char *who;           // for run_two_lanes' messages
  const char *key_a, *key_b;  // report keys of a piece's ms_a, ms_b ("seconds_..."; key_b may be null)
  bool has_encode;            // the wall time of `work` beyond the three kernel times is the encode's ("seconds_encode"; else it is 0)
};
using PieceWork = FilePieces::Piece;
using PieceFn = std::function<Status(EncodeLane &d, unsigned long long bytes, PieceWork *w)>;

Status file_to_text(EncoderDevice *dev, int device, const TextRoute &route, const std::string &path, const std::string &out_path, unsigned long long piece_bytes,
                    const PieceFn &work_piece, unsigned long long *n_lines_out, unsigned long long *n_ids_out, unsigned long long *n_text_out,
                    std::string *report) {
  if (!dev) return Status(2, "encoder has no device state");
  if (out_path.empty()) return Status(1, "Failed to open file for writing: no output path");
  FilePieces fp(path, dev, device, piece_bytes);
  const Status opened = fp.open_input();
  if (!opened.ok()) return opened;
  const struct stat &sb = fp.sb;
  Fd out;
  // (opened without O_TRUNC, emptied only once it is known not to be the input itself: the output may be longer than the input it would overwrite)
  out.fd = open(out_path.c_str(), O_WRONLY | O_CREAT | O_CLOEXEC, 0644);
  struct stat ob;
  if (out.fd < 0 || fstat(out.fd, &ob) != 0) return Status(1, "Failed to open file for writing: " + out_path + " (" + strerror(errno) + ")");
  if (ob.st_dev == sb.st_dev && ob.st_ino == sb.st_ino) return Status(1, "Failed to open file for writing: " + out_path + " is the input file");
  if (S_ISREG(ob.st_mode) && ftruncate(out.fd, 0) != 0) return Status(1, "Failed to open file for writing: " + out_path + " (" + strerror(errno) + ")");
  const std::shared_ptr<const Config> C = dev->cfg;
  const CfgBind bind(C);
  std::lock_guard<std::mutex> lk0(dev->lane[0].mu), lk1(dev->lane[1].mu);  // (lane 0 first, always: nobody else waits for two lanes)

  double s_split = 0, s_enc = 0, s_a = 0, s_b = 0, s_down = 0;
  unsigned long long lines_total = 0, ids_total = 0, text_total = 0;  // (the download leg's)

  auto upload = [&](size_t i, bool *exhausted) { return fp.upload(i, exhausted); };
  auto work = [&](size_t i) {
    PieceWork &p = fp.piece[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    const Status st = work_piece(dev->lane[i & 1], p.bytes, &p);
    s_split += p.ms_split * 1e-3;
    s_a += p.ms_a * 1e-3;
    s_b += p.ms_b * 1e-3;
    if (route.has_encode) s_enc += secs_since(t0) - (p.ms_split + p.ms_a + p.ms_b) * 1e-3;
    return st;
  };
  auto download = [&](size_t i) {
    const PieceWork p = fp.piece[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    EncodeLane &d = dev->lane[i & 1];
    const unsigned long long text_base = text_total;
    std::atomic<bool> write_ok{true};
    try {
      if (p.n_text)
        staged_transfer(device, d.dec.bytes.p, p.n_text, false, [&](void *chunk, unsigned long long o, size_t len) {
          if (!pwrite_all(out.fd, chunk, len, text_base + o)) { write_ok.store(false); return false; }
          return true;
        }, nullptr, ENC_CHUNK);
    } catch (const GpuError &) {
      if (!write_ok.load()) return Status(1, "Failed to write file: " + out_path);
      throw;
    }
    text_total += p.n_text;
    ids_total += p.n_ids;
    lines_total += p.n_lines;
    s_down += secs_since(t0);
    return Status();
  };
  size_t n_pieces = 0;
  const Status piped = run_two_lanes(route.who, C, device, PIPE_UNTIL_EXHAUSTED, upload, work, download, &n_pieces);
  if (!piped.ok()) return piped;
  const int fd = out.fd;
  out.fd = -1;
  if (close(fd) != 0) return Status(1, "Failed to write file: " + out_path);
  if (n_lines_out) *n_lines_out = lines_total;
  if (n_ids_out) *n_ids_out = ids_total;
  if (n_text_out) *n_text_out = text_total;
  if (report) *report = fp.report(n_pieces, lines_total, ids_total, &text_total, s_split, s_enc, {{route.key_a, s_a}, {route.key_b, s_b}}, s_down);
  return Status();
}
}  // namespace

Status BaseEncoder::encode_file_subword(const std::string &path, const std::string &out_path, bool bos, bool eos, bool reverse, double dropout_prob,
                                        unsigned long long piece_bytes, unsigned long long *n_lines_out, unsigned long long *n_ids_out,
                                        unsigned long long *n_text_out, std::string *report) const {
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  if (n_text_out) *n_text_out = 0;
  if (n_added_tokens() && !byte_fallback()) return Status(1, SUBWORD_UNDER_ADDED_TOKENS);
  const Status tokens = check_bos_eos(*this, bos, eos);
  if (!tokens.ok()) return tokens;
  const int device = device_;
  EncoderDevice *dev = dev_;
  const PieceFn work = [&](EncodeLane &d, unsigned long long bytes, PieceWork *w) {
    return subword_text_on_lane(*this, *dev, d, device, d.in.bytes, bytes, bos, eos, reverse, dropout_prob, &w->n_lines, &w->n_ids, &w->n_text, &w->ms_split,
                                nullptr, &w->ms_a);
  };
  return file_to_text(dev, device, TextRoute{"encode_file_subword", "seconds_format", nullptr, true}, path, out_path, piece_bytes, work, n_lines_out, n_ids_out,
                      n_text_out, report);
}

// ... with the id printer in place of the SUBWORD formatter: the file `yttm encode --output_type id < path` prints
Status BaseEncoder::encode_file_idtext(const std::string &path, const std::string &out_path, bool bos, bool eos, bool reverse, double dropout_prob,
                                       unsigned long long piece_bytes, unsigned long long *n_lines_out, unsigned long long *n_ids_out,
                                       unsigned long long *n_text_out, std::string *report) const {
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  if (n_text_out) *n_text_out = 0;
  const Status tokens = check_bos_eos(*this, bos, eos);
  if (!tokens.ok()) return tokens;
  const int device = device_;
  EncoderDevice *dev = dev_;
  const PieceFn work = [&](EncodeLane &d, unsigned long long bytes, PieceWork *w) {
    const Status s = encode_text_on_lane(*this, *dev, d, device, d.in.bytes, bytes, bos, eos, reverse, dropout_prob, &w->n_lines, &w->n_ids, &w->ms_split, nullptr);
    if (!s.ok()) return s;
    return idtext_on_lane(d, device, &w->n_text, &w->ms_a);
  };
  return file_to_text(dev, device, TextRoute{"encode_file_idtext", "seconds_format", nullptr, true}, path, out_path, piece_bytes, work, n_lines_out, n_ids_out,
                      n_text_out, report);
}

// A file of decimal ids, one sentence per line -> the file `yttm decode < path` prints: split + parse + decode in place of split + encode + format.
// An id that is neither ignored nor valid ends the call at its piece -- the pieces are worked on in file order, so it is the first such id of the
// file --, with the text of the pieces before it written.
Status BaseEncoder::decode_file(const std::string &path, const std::string &out_path, const int32_t *ignore_ids, unsigned long long n_ignore,
                                unsigned long long piece_bytes, unsigned long long *n_lines_out, unsigned long long *n_ids_out, unsigned long long *n_text_out,
                                std::string *report) const {
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  if (n_text_out) *n_text_out = 0;
  if (n_ignore && !ignore_ids) return Status(2, "decode_file: no ignore_ids");
  const int device = device_;
  EncoderDevice *dev = dev_;
  const PieceFn work = [&](EncodeLane &d, unsigned long long bytes, PieceWork *w) {
    return decode_text_on_lane(*this, *dev, d, device, d.in.bytes, bytes, ignore_ids, n_ignore, &w->n_lines, &w->n_ids, &w->n_text, &w->ms_split, &w->ms_a,
                               &w->ms_b);
  };
  return file_to_text(dev, device, TextRoute{"decode_file", "seconds_parse", "seconds_decode", false}, path, out_path, piece_bytes, work, n_lines_out, n_ids_out,
                      n_text_out, report);
}

// ---- a text file to training blocks --------------------------------------------------------------------------------------------------------
// The pipeline of encode_file_counts: piece k is split, encoded and packed (k_blocks.h) with tail = keep while piece k + 1 is read and uploaded, so
// the rows do not depend on the cuts; behind the last piece the open row is flushed (tail = pad) or discarded (drop).  The blocks slot is the
// encoder's one, not a lane's, so a piece's rows and fragments are written to PREFIX.rows / PREFIX.frags inside `work`, before the next piece
// replaces them; there is no download leg.  PREFIX.frags holds uint64 (start, length) pairs, the starts flat over the whole file.
Status BaseEncoder::encode_file_blocks(const std::string &path, const std::string &out_prefix, bool bos, bool eos, bool reverse, double dropout_prob,
                                       unsigned long long piece_bytes, unsigned long long seq_len, int mode, int32_t pad_value, int tail,
                                       unsigned long long *n_rows_out, unsigned long long *n_frags_out, unsigned long long *n_lines_out,
                                       unsigned long long *n_ids_out, std::string *report) const {
  if (n_rows_out) *n_rows_out = 0;
  if (n_frags_out) *n_frags_out = 0;
  if (n_lines_out) *n_lines_out = 0;
  if (n_ids_out) *n_ids_out = 0;
  const Status tokens = check_bos_eos(*this, bos, eos);
  if (!tokens.ok()) return tokens;
  if (!dev_) return Status(2, "encoder has no device state");
  if (seq_len < 1 || seq_len > (1ull << 24)) return Status(1, "blocks: seq_len must be within 1 .. 2^24 (" + std::to_string(seq_len) + ")");
  if (mode != 0 && mode != 1) return Status(1, "blocks: mode must be 0 (stream) or 1 (whole)");
  if (tail != 0 && tail != 2) return Status(1, "encode_file_blocks: tail must be 0 (pad) or 2 (drop)");
  if (out_prefix.empty()) return Status(1, "Failed to open file for writing: no output prefix");
  FilePieces fp(path, dev_, device_, piece_bytes);
  const Status opened = fp.open_input();
  if (!opened.ok()) return opened;
  const std::string rows_path = out_prefix + ".rows", frags_path = out_prefix + ".frags";
  Fd out_rows, out_frags;
  out_rows.fd = open(rows_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (out_rows.fd < 0) return Status(1, "Failed to open file for writing: " + rows_path + " (" + strerror(errno) + ")");
  out_frags.fd = open(frags_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (out_frags.fd < 0) return Status(1, "Failed to open file for writing: " + frags_path + " (" + strerror(errno) + ")");
  const std::shared_ptr<const Config> C = dev_->cfg;
  const CfgBind bind(C);
  const int device = device_;
  EncoderDevice *dev = dev_;
  std::lock_guard<std::mutex> lk0(dev->lane[0].mu), lk1(dev->lane[1].mu);  // (lane 0 first, always: nobody else waits for two lanes)
  dev->blk.open_f = dev->blk.open_m = 0;  // the file starts from an empty open row

  double s_split = 0, s_enc = 0, s_blocks = 0, s_down = 0;
  unsigned long long lines_total = 0, ids_total = 0, rows_total = 0, frags_total = 0;
  // the slot's rows and fragments behind what the file holds so far
  auto write_slot = [&](unsigned long long nr, unsigned long long nf) -> Status {
    const auto t0 = std::chrono::steady_clock::now();
    const unsigned long long flat_base = rows_total * seq_len;
    std::atomic<bool> write_ok{true};
    try {
      if (nr)
        staged_transfer(device, (uint8_t *)dev->blk.rows.p, nr * seq_len * 4, false, [&](void *chunk, unsigned long long o, size_t len) {
          if (!pwrite_all(out_rows.fd, chunk, len, flat_base * 4 + o)) { write_ok.store(false); return false; }
          return true;
        }, nullptr, ENC_CHUNK);
      if (nf)
        staged_transfer(device, (uint8_t *)dev->blk.frags.p, nf * 8, false, [&](void *chunk, unsigned long long o, size_t len) {
          const int32_t *v = (const int32_t *)chunk;
          std::vector<unsigned long long> wide(len / 4);
          for (size_t j = 0; j < len / 8; j++) {
            wide[2 * j] = flat_base + (unsigned long long)(uint32_t)v[2 * j];
            wide[2 * j + 1] = (unsigned long long)(uint32_t)v[2 * j + 1];
          }
          if (!pwrite_all(out_frags.fd, wide.data(), wide.size() * 8, frags_total * 16 + o * 2)) { write_ok.store(false); return false; }
          return true;
        }, nullptr, ENC_CHUNK);
    } catch (const GpuError &) {
      if (!write_ok.load()) return Status(1, "Failed to write file: " + out_prefix + ".rows / .frags");
      throw;
    }
    rows_total += nr;
    frags_total += nf;
    s_down += secs_since(t0);
    return Status();
  };
  auto upload = [&](size_t i, bool *exhausted) { return fp.upload(i, exhausted); };
  auto work = [&](size_t i) {
    FilePieces::Piece &p = fp.piece[i & 1];
    EncodeLane &d = dev->lane[i & 1];
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long nr = 0, nf = 0;
    Status st = encode_text_on_lane(*this, *dev, d, device, d.in.bytes, p.bytes, bos, eos, reverse, dropout_prob, &p.n_lines, &p.n_ids, &p.ms_split, nullptr);
    if (st.ok())
      st = blocks_on_lane(*dev, d, device, d.res.ids, d.res.off, p.n_lines, p.n_lines ? p.n_ids : 0, BlkParams{seq_len, mode, pad_value, 1}, "line", lines_total + 1,
                          &nr, &nf, &p.ms_a);
    s_split += p.ms_split * 1e-3;
    s_blocks += p.ms_a * 1e-3;
    s_enc += secs_since(t0) - (p.ms_split + p.ms_a) * 1e-3;
    if (st.ok()) st = on_device(device, [&]() -> Status { return write_slot(nr, nf); });
    lines_total += p.n_lines;
    ids_total += p.n_ids;
    return st;
  };
  auto download = [&](size_t) { return Status(); };
  size_t n_pieces = 0;
  Status piped = run_two_lanes("encode_file_blocks", C, device, PIPE_UNTIL_EXHAUSTED, upload, work, download, &n_pieces);
  if (piped.ok() && tail == 0) {
    unsigned long long nr = 0, nf = 0;
    double ms = 0;
    const BlkParams flush{dev->blk.open_f ? dev->blk.open_L : seq_len, dev->blk.open_f ? dev->blk.open_mode : mode, pad_value, 0};
    piped = blocks_on_lane(*dev, dev->lane[0], device, nullptr, nullptr, 0, 0, flush, "line", 0, &nr, &nf, &ms);
    s_blocks += ms * 1e-3;
    if (piped.ok()) piped = on_device(device, [&]() -> Status { return write_slot(nr, nf); });
  }
  dev->blk.open_f = dev->blk.open_m = 0;  // (drop, or a call that failed on its way: the open row is empty afterwards)
  if (!piped.ok()) return piped;
  const int fd_a = out_rows.fd, fd_b = out_frags.fd;
  out_rows.fd = out_frags.fd = -1;
  const bool ok_a = close(fd_a) == 0, ok_b = close(fd_b) == 0;
  if (!ok_a || !ok_b) return Status(1, "Failed to write file: " + (ok_a ? frags_path : rows_path));
  if (n_rows_out) *n_rows_out = rows_total;
  if (n_frags_out) *n_frags_out = frags_total;
  if (n_lines_out) *n_lines_out = lines_total;
  if (n_ids_out) *n_ids_out = ids_total;
  if (report) {
    const std::string r = fp.report(n_pieces, lines_total, ids_total, nullptr, s_split, s_enc, {{"seconds_blocks", s_blocks}}, s_down);
    *report = "{\"rows\": " + std::to_string(rows_total) + ", \"frags\": " + std::to_string(frags_total) + ", " + r.substr(1);
  }
  return Status();
}

}  // namespace yttm
