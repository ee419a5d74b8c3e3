/* yttm_mi355x.h -- the drop-in boundary: C ABI of libyttm_mi355x.so.
 *
 * These entry points are what a binding of the reference (youtokentome/cpp/yttm.pyx) binds instead of the C++
 * surface of youtokentome/cpp/bpe.h.  Each one cites the reference interface it replaces (file:line in
 * /root/reference).  Plain pointers and sizes only; no C++/torch types.  Errors follow the reference's
 * Status{code,message} (utils.h:56-64): return value 0 = ok, otherwise the message is copied to `err`
 * (user-visible wording kept verbatim); the binding raises ValueError(message) like yttm.pyx:61-62,:84-85.
 *
 * Sentences cross the boundary packed: UTF-8 bytes + offsets[n_sent+1] (sentence i = bytes[offsets[i]..offsets[i+1])).
 * Output arrays are malloc'ed by the library and released with yttm_free().
 * Threading: one host thread per encoder/ctx at a time; n_threads is accepted for API compatibility and ignored
 * (the hot path runs on the GPU).  The library needs a visible MI355X (gfx950) and fails loudly without one.
 */
#ifndef YTTM_MI355X_H
#define YTTM_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* replaces: vkcom::Status train_bpe(const std::string& input_path, const std::string& model_path, int vocab_size,
 *           BpeConfig config)                                       bpe.h:19, bpe.cpp:1368; yttm.pyx:64-85 */
int yttm_train_bpe(const char *input_path, const char *model_path, int vocab_size, double coverage, int n_threads,
                   int pad_id, int unk_id, int bos_id, int eos_id, char *err, int errlen);

/* The same call with the device ordinal chosen by the caller and the report of the *_from_device variant below
 * (adds "seconds_upload": file -> pinned chunks -> HBM, which replaces fast_read_file_utf8, bpe.cpp:67-84). */
int yttm_train_bpe_ex(const char *input_path, const char *model_path, int vocab_size, double coverage, int n_threads,
                      int pad_id, int unk_id, int bos_id, int eos_id, int device, char *report_json, int report_len,
                      char *err, int errlen);

/* Same training on a corpus that is already in host memory (no file read), or already resident in HBM
 * (`d_text` = device pointer, 16-byte aligned).  `device` = HIP device ordinal.  `report_json` (optional, may be
 * NULL) receives a JSON object with wall-time phases and per-kernel GPU time / algorithmic bytes
 * (profile != 0 times every kernel with HIP events on the launch stream), and counters of the merge loop: "rounds",
 * "rules", "rounds_exhausted", "batch_extensions", "batch_splits" (word-mode batches of 129 .. 256 rules cut to their first
 * 128), "word_switch_round" / "word_rounds" / "word_fused_rounds" (rounds in K4's word mode; of those, one launch each) /
 * "word_all_rounds" (rounds that had to visit every word), "index_builds", "index_radix_builds" (of those: filled by radix partition of the postings), "hot_rebuilds", "top_refills", "repacks", "front_end_overlapped" (1: the char histogram, the segment
 * starts and the word dedup ran on the parts of the text while the rest was still being uploaded, and that word table was taken). */
int yttm_train_bpe_from_memory(const uint8_t *text, uint64_t n, const char *model_path, int vocab_size, double coverage,
                               int pad_id, int unk_id, int bos_id, int eos_id, int device, char *report_json,
                               int report_len, char *err, int errlen);
int yttm_train_bpe_from_device(const void *d_text, uint64_t n, const char *model_path, int vocab_size, double coverage,
                               int pad_id, int unk_id, int bos_id, int eos_id, int device, int profile,
                               char *report_json, int report_len, char *err, int errlen);

/* replaces: class vkcom::BaseEncoder                                 bpe.h:22-82 */
typedef struct yttm_encoder yttm_encoder;

/* BaseEncoder(const std::string& model_path, int n_threads, Status*) bpe.h:33, bpe.cpp:1643; yttm.pyx:58-62 */
int yttm_encoder_create(const char *model_path, int n_threads, int device, yttm_encoder **out, char *err, int errlen);
/* yttm.pyx:55-56 __dealloc__ */
void yttm_encoder_destroy(yttm_encoder *enc);

/* Status encode_as_ids(const vector<string>&, vector<vector<int>>*, bool bos, bool eos, bool reverse,
 *                      double dropout_prob) const                    bpe.h:37-39, bpe.cpp:1740; yttm.pyx:87-109 */
int yttm_encode_as_ids(yttm_encoder *enc, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos,
                       int eos, int reverse, double dropout_prob, int32_t **ids, uint64_t **out_offsets, char *err,
                       int errlen);

/* Status encode_as_subwords(...)                                      bpe.h:41-46, bpe.cpp:1757; yttm.pyx:110-124
 * pieces come back as one blob + piece_off[n_pieces+1] + sent_off[n_sent+1] (piece index ranges per sentence). */
int yttm_encode_as_subwords(yttm_encoder *enc, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos,
                            int eos, int reverse, double dropout_prob, char **blob, uint64_t **piece_off,
                            uint64_t *n_pieces, uint64_t **sent_off, char *err, int errlen);

/* Device-resident batch encode (what bench.py times): input bytes/offsets already in HBM, ids stay in HBM inside
 * the encoder until yttm_encode_fetch copies them out.  kernel_ms (optional) = HIP-event time of the K5 launch. */
int yttm_encode_device(yttm_encoder *enc, const void *d_bytes, const void *d_offsets, uint64_t n_sent,
                       uint64_t total_bytes, uint64_t max_sentence_bytes, int bos, int eos, int reverse,
                       double dropout_prob, uint64_t *n_ids, double *kernel_ms, char *err, int errlen);
int yttm_encode_fetch(yttm_encoder *enc, int32_t *ids, uint64_t *out_offsets, uint64_t n_sent, char *err, int errlen);
/* The result of the last yttm_encode_device, device to device into memory the caller owns (a framework's tensors): ragged
 * (int32 ids[n_ids], uint64 out_offsets[n_sent+1]), or as a row-major int32 matrix [n_sent, width] whose row tails hold pad_value, plus
 * int32 lengths[n_sent] (k_enc_pad).  *longest = the longest row; width < longest is an error (code 1) and writes nothing: no row is
 * truncated.  The reference has no counterpart: its encode_as_ids fills vector<vector<int>>, bpe.h:36-39, bpe.cpp:1736-1755. */
int yttm_encode_copy_device(yttm_encoder *enc, void *d_ids, void *d_out_offsets, uint64_t n_sent, char *err, int errlen);
int yttm_encode_copy_padded(yttm_encoder *enc, void *d_matrix, void *d_lengths, uint64_t n_sent, uint64_t width, int32_t pad_value,
                            uint64_t *longest, char *err, int errlen);

/* Text that is not cut into sentences yet: its lines are found on the device, by the rules of std::getline as the command line applies them
 * (bpe.cpp:1942-2014 reads std::cin with std::getline, utils.cpp:103-111): a line ends at the byte 0x0A; a last line without one counts; nothing
 * follows a final newline; empty text has 0 lines; "\r" is no separator; an empty line is a sentence.  The lines come as the packed convention
 * of this header: uint64 offsets[n_lines + 1], offsets[0] = 0, line i = text[offsets[i] .. offsets[i+1]) INCLUDING its newline (white space
 * to the encoder: the ids of a line equal those of the line without it), offsets[n_lines] = n_bytes.
 * yttm_lines_device: d_text = any device address.  The offsets stay in HBM inside the encoder, beside a pending encode or decode result, until
 * yttm_lines_copy_device (to device memory the caller owns) / yttm_lines_fetch (to a host array) takes them.  *longest = the longest line in
 * bytes, its newline included; kernel_ms (optional) = HIP-event time of count + scan + write + longest.  One thread at a time, as the other
 * device pairs. */
int yttm_lines_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, uint64_t *n_lines, uint64_t *longest, double *kernel_ms, char *err,
                      int errlen);
int yttm_lines_copy_device(yttm_encoder *enc, void *d_offsets, uint64_t n_lines, char *err, int errlen);
int yttm_lines_fetch(yttm_encoder *enc, uint64_t *offsets, uint64_t n_lines, char *err, int errlen);
/* yttm_lines_device, then yttm_encode_device on those lines: the result is pending exactly as after yttm_encode_device with n_sent = *n_lines
 * (yttm_encode_fetch, yttm_encode_copy_device, yttm_encode_copy_padded, yttm_encode_cache_words), and the lines' offsets as after
 * yttm_lines_device.  kernel_ms (optional) = split + encode.  bpe.cpp:1942-2014 (the batch loop of encode_cli) without the text formatting */
int yttm_encode_text_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob,
                            uint64_t *n_lines, uint64_t *n_ids, double *kernel_ms, char *err, int errlen);
/* A text file of any size -> ids.  The file is read with pread into pinned chunks and crosses in pieces of about chunk_bytes (0: the default),
 * each cut behind the last newline inside it -- a longer line extends its piece, it is never split --, through both encoder lanes: the upload of
 * one piece runs beside the split and encode of the one before and the download of the one before that.  With dropout_prob == 0 the result
 * does not depend on chunk_bytes.  out_prefix == NULL: *ids (int32[*n_ids]) and *offsets (uint64[*n_lines + 1], into ids) are malloc'ed, to be
 * released with yttm_free, as yttm_encode_as_ids returns them.  Otherwise two raw little-endian files are written, PREFIX.ids (int32) and
 * PREFIX.off (uint64, *n_lines + 1), and ids / offsets may be NULL.  report_json (optional): {"pieces", "piece_bytes", "bytes", "lines", "ids",
 * "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_download_write"} (the four legs overlap).  A file that
 * cannot be read or written is code 1 with a plain message.  Uses both lanes: a pending device result does not survive the call.
 * replaces: encode_cli (bpe.h:66-68, bpe.cpp:1942-2014) with output_type "id", without the decimal formatting */
int yttm_encode_file(yttm_encoder *enc, const char *path, const char *out_prefix, int bos, int eos, int reverse, double dropout_prob,
                     uint64_t chunk_bytes, int32_t **ids, uint64_t **offsets, uint64_t *n_lines, uint64_t *n_ids, char *report_json, int report_len,
                     char *err, int errlen);

/* SUBWORD output on the device: the text `yttm encode --output_type subword` prints for the batch -- per sentence every piece followed by one
 * space, then '\n' (utils.h:92-103); an empty sentence is "\n".  The ids are exactly those of yttm_encode_device with the same arguments, in
 * the order it stores them; the piece of an id is id_to_subword(id, replace_space = false), and the k-th unk_id of a sentence in forward order is
 * the text of its k-th run of unknown chars (its valid code points; invalid bytes are dropped and do not end a run).
 * yttm_subword_device encodes exactly as yttm_encode_device, then formats: afterwards the ids are pending as after yttm_encode_device, and the
 * text is pending in the encoder's text slot, THE SAME ONE a decode result uses -- a pending yttm_decode_device[_padded] result is replaced, and
 * the text is taken with yttm_decode_fetch / yttm_decode_copy_device: char bytes[*n_text_bytes], uint64 out_offsets[n_sent + 1],
 * out_offsets[0] = 0, line i = bytes[out_offsets[i] .. out_offsets[i+1]) including its '\n'.  kernel_ms (optional) = HIP-event time of encode +
 * measure + scan + write.  bos / eos on a model trained without them: the message and code (1) of yttm_encode_as_subwords, nothing is written
 * and nothing that was pending is replaced.
 * replaces: encode_as_subwords, bpe.h:41-46, bpe.cpp:1757 (the pieces: bpe.cpp:1597-1613), and the text formatting of encode_cli,
 * bpe.cpp:1942-2014 */
int yttm_subword_device(yttm_encoder *enc, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes,
                        uint64_t max_sentence_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_ids, uint64_t *n_text_bytes,
                        double *kernel_ms, char *err, int errlen);
/* yttm_encode_text_device, then the format: lines, ids and the lines' offsets are pending as after yttm_encode_text_device (n_sent = *n_lines), the
 * text as after yttm_subword_device.  kernel_ms (optional) = split + encode + format.  bpe.h:41-46, bpe.cpp:1757, :1597-1613, :1942-2014 */
int yttm_subword_text_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob,
                             uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen);
/* A text file of any size -> the text file `yttm encode --output_type subword < path` prints, byte for byte, written to out_path.  The pipeline
 * of yttm_encode_file: upload of one piece beside split + encode + format of the one before and the download and write of the text of the one
 * before that.  With dropout_prob == 0 the file does not depend on chunk_bytes.  report_json (optional): the keys of yttm_encode_file plus
 * "seconds_format" and "text_bytes".  A file that cannot be read or written is code 1 with a plain message; so are an empty out_path and an
 * out_path that names the input file itself (same device and inode: refused before anything is truncated).  out_path is emptied when the call
 * begins; a call that fails later leaves a partial file there, as yttm_encode_file leaves partial PREFIX.ids / PREFIX.off.  Uses both lanes: a pending device
 * result does not survive the call.  bpe.h:41-46, bpe.cpp:1757, :1597-1613, :1942-2014 */
int yttm_encode_file_subword(yttm_encoder *enc, const char *path, const char *out_path, int bos, int eos, int reverse, double dropout_prob,
                             uint64_t chunk_bytes, uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len,
                             char *err, int errlen);

/* Decimal id text on the device: the format `yttm encode --output_type id` prints and `yttm decode` reads, one sentence per line.
 * yttm_ids_parse_device = yttm_lines_device, then the ids `while (ss >> x) ids.push_back(x)` reads from every line in the C locale
 * (bpe.cpp:1863-1873): white space is 0x20 and 0x09 .. 0x0D; a number is a maximal run of digits, negated iff the byte just before it is '-'
 * (so "12-3" is 12, -3); a line ends at its first fail point -- a byte that is neither white space, a digit nor a sign, a sign whose next byte in
 * the line is not a digit, or a number outside int32, which is itself dropped -- and nothing carries over to the next line.  The lines' offsets
 * are pending as after yttm_lines_device, the ids exactly as after yttm_encode_device with n_sent = *n_lines (yttm_encode_fetch,
 * yttm_encode_copy_device, yttm_encode_copy_padded).  kernel_ms (optional) = split + measure + scan + write.  d_text: any address. */
int yttm_ids_parse_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, uint64_t *n_lines, uint64_t *n_ids, double *kernel_ms, char *err,
                          int errlen);
/* yttm_ids_parse_device, then the device decode of those ids with a '\n' behind every line: lines and ids are pending as after the parse, the text
 * in the encoder's text slot (yttm_decode_fetch / yttm_decode_copy_device: out_offsets[*n_lines + 1], line i = bytes[out_offsets[i] ..
 * out_offsets[i+1]) including its '\n') -- concatenated, byte for byte what yttm_decode_cli writes for the same input.  A kept id outside
 * [0, vocab_size) that is not ignored fails the call with the message and code (1) of yttm_decode, naming the first such id in line order, then
 * position order (ids behind a line's fail point are not ids); then the parse's results are pending and no text is.  kernel_ms (optional) =
 * split + parse + decode.  replaces: decode_cli, bpe.h:70, bpe.cpp:2016-2028, on decode(const vector<string>&, ...) bpe.cpp:1863-1882 */
int yttm_decode_text_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, const int32_t *ignore_ids, uint64_t n_ignore, uint64_t *n_lines,
                            uint64_t *n_ids, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen);
/* A file of decimal ids of any size -> the file `yttm decode < path` prints, byte for byte, written to out_path.  The pipeline of
 * yttm_encode_file_subword: upload of one piece beside split + parse + decode of the one before and the download and write of the text of the one
 * before that; the same file errors and messages, the same refusal to write over the input; the file does not depend on chunk_bytes.
 * report_json (optional): the keys of yttm_encode_file ("seconds_encode" is 0) plus "seconds_parse", "seconds_decode" and "text_bytes".  An id
 * that is neither ignored nor valid ends the call with the decode's message for the first such id in file order and leaves a partial file.
 * Uses both lanes: a pending device result does not survive the call.  bpe.h:70, bpe.cpp:2016-2028, :1863-1882 */
int yttm_decode_file(yttm_encoder *enc, const char *path, const char *out_path, const int32_t *ignore_ids, uint64_t n_ignore, uint64_t chunk_bytes,
                     uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len, char *err, int errlen);
/* The pending encode result (of yttm_encode_device, yttm_encode_text_device, yttm_ids_parse_device, ...; n_sent must be its) as the text `yttm encode
 * --output_type id` prints: every id in decimal, '-' for a negative one, followed by one space, then '\n' per sentence (utils.h:92-103); an empty
 * sentence is "\n".  The text is pending in the encoder's text slot as after yttm_subword_device, the ids stay pending.  No pending result of
 * n_sent sentences: code 1, and nothing that was pending is replaced.  kernel_ms (optional) = measure + scan + write.
 * replaces: the id formatting of encode_cli, bpe.cpp:1942-2014 */
int yttm_idtext_device(yttm_encoder *enc, uint64_t n_sent, uint64_t *n_text_bytes, double *kernel_ms, char *err, int errlen);
/* A text file of any size -> the file `yttm encode --output_type id < path` prints, byte for byte: yttm_encode_file_subword with the id printer in
 * place of the SUBWORD formatter (same pipeline, errors, report keys).  bpe.h:66-68, bpe.cpp:1942-2014 */
int yttm_encode_file_idtext(yttm_encoder *enc, const char *path, const char *out_path, int bos, int eos, int reverse, double dropout_prob,
                            uint64_t chunk_bytes, uint64_t *n_lines, uint64_t *n_ids, uint64_t *n_text_bytes, char *report_json, int report_len,
                            char *err, int errlen);

/* Byte spans on the device: for every id the bytes of its sentence it stands for, uint32 spans[n_ids][2] = (start, end), end exclusive, in bytes
 * from the sentence's first byte, in the order of the ids.  Read as the encoder reads it (invalid bytes dropped, white space = isspace() in the C
 * locale or U+2581), a sentence is a sequence of units: a valid non-space char of the alphabet, or a maximal run of valid chars outside the
 * alphabet that no space and no alphabet char interrupts (invalid bytes do not end it); a unit starts at the first byte of its first char and ends
 * behind the last byte of its last valid char.  An id covers u units: 1 for unk_id, else the code points of id_to_subword(id) other than U+2581
 * (0 for "\u2581" alone, <PAD>, <BOS>, <EOS>).  In forward order, with a the units of the ids before it, an id with u > 0 has the span
 * [start(unit a), end(unit a + u - 1)) -- beside its chars only invalid bytes lie inside --, one with u == 0 the empty span (p, p), p =
 * start(unit a), or the end of the sentence's last unit where there is none (0 in a sentence without units).  With reverse the ids are stored back
 * to front, and span k belongs to stored id k.  A sentence is below 4 GB.
 * yttm_spans_device encodes exactly as yttm_encode_device, then computes the spans in one pass: afterwards the ids are pending as after
 * yttm_encode_device and the spans in a slot of their own, which any later encode on the encoder empties.  kernel_ms (optional) = encode + spans.
 * bos / eos on a model trained without them: the message and code (1) of yttm_encode_as_ids, and nothing that was pending is replaced. */
int yttm_spans_device(yttm_encoder *enc, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes,
                      uint64_t max_sentence_bytes, int bos, int eos, int reverse, double dropout_prob, uint64_t *n_ids, double *kernel_ms, char *err,
                      int errlen);
/* yttm_encode_text_device, then the spans: a sentence is a line including its newline, the spans count from the line's first byte.  Lines, ids and
 * the lines' offsets are pending as after yttm_encode_text_device.  kernel_ms (optional) = split + encode + spans. */
int yttm_spans_text_device(yttm_encoder *enc, const void *d_text, uint64_t n_bytes, int bos, int eos, int reverse, double dropout_prob,
                           uint64_t *n_lines, uint64_t *n_ids, double *kernel_ms, char *err, int errlen);
/* The pending spans (n_sent must be theirs): to a host array, to device memory the caller owns (ragged, uint32 [n_ids][2]), or as a padded
 * matrix uint32 [n_sent, width, 2] whose row tails are (0, 0) (8-byte aligned; width < the longest row: the message and code (1) of
 * yttm_encode_copy_padded, *longest says what is needed, nothing is written).  No pending spans -- none were made, or an encode came after them:
 * code 1. */
int yttm_spans_fetch(yttm_encoder *enc, uint32_t *spans, uint64_t n_sent, char *err, int errlen);
int yttm_spans_copy_device(yttm_encoder *enc, void *d_spans, uint64_t n_sent, char *err, int errlen);
int yttm_spans_copy_padded(yttm_encoder *enc, void *d_matrix, uint64_t n_sent, uint64_t width, uint64_t *longest, char *err, int errlen);
/* Host to host: yttm_encode_as_ids and the spans of those ids, uint32 (*spans)[n_ids][2]; all three arrays are released with yttm_free. */
int yttm_encode_as_ids_spans(yttm_encoder *enc, const uint8_t *bytes, const uint64_t *offsets, uint64_t n_sent, int bos, int eos, int reverse,
                             double dropout_prob, int32_t **ids, uint64_t **out_offsets, uint32_t **spans, char *err, int errlen);

/* Token frequencies on the device: for n_bins > 0 the result is uint64 counts[n_bins + 1]; counts[v] = the number of ids equal to v for
 * 0 <= v < n_bins, counts[n_bins] = the number of ids outside [0, n_bins) -- negative ids (a parsed id file can hold them), ids >= n_bins,
 * INT32_MIN, INT32_MAX.  No id is an error, and sum(counts) = the number of ids counted, always.  n_bins == 0 means yttm_vocab_size(enc); the
 * largest n_bins is 2^31 (code 1 beyond).  The counts live in a slot of their own inside the encoder: no later encode, decode, parse or file call
 * empties it.  accumulate == 0 zeroes the slot before counting; accumulate != 0 adds on top and requires the slot's n_bins to match (else code 1
 * and nothing is changed; on an encoder that has not counted yet it starts from zero).  Counting never changes or consumes what it counts: a
 * pending encode result is still pending afterwards and fetches the same bytes.  Made in one pass (k_idcount.h) that reads every id once and
 * writes nothing per id; integer sums, so the result is exact whatever the order.
 * yttm_id_counts_device counts the pending encode result, whichever call left it (yttm_encode_device, yttm_encode_text_device,
 * yttm_ids_parse_device, yttm_spans_device, ...); n_sent must be the pending result's, as for yttm_idtext_device.  No pending result: code 1, and
 * nothing pending or counted is changed.  *n_counted (optional): the ids counted by this call. */
int yttm_id_counts_device(yttm_encoder *enc, uint64_t n_sent, uint64_t n_bins, int accumulate, uint64_t *n_counted, double *kernel_ms, char *err,
                          int errlen);
/* ... any int32 ids[n_ids] in HBM (4-byte aligned; the caller synchronises the stream that wrote it first, as for yttm_decode_device).
 * n_ids == 0 is legal. */
int yttm_id_counts_ids_device(yttm_encoder *enc, const void *d_ids, uint64_t n_ids, uint64_t n_bins, int accumulate, double *kernel_ms, char *err,
                              int errlen);
/* The counts, n_bins + 1 values: to a host array, or to device memory the caller owns.  n_bins must be the slot's (0 = vocab size); no counts
 * yet: code 1. */
int yttm_id_counts_fetch(yttm_encoder *enc, uint64_t *counts, uint64_t n_bins, char *err, int errlen);
int yttm_id_counts_copy_device(yttm_encoder *enc, void *d_counts, uint64_t n_bins, char *err, int errlen);
/* The pipeline of yttm_encode_file (upload of one piece beside split + encode + count of the one before) with no download leg but the final
 * vocab_size + 1 integers, written to the caller's counts[vocab_size + 1].  The same file errors and messages as yttm_encode_file, the same
 * <BOS> / <EOS> messages; with dropout_prob == 0 the counts never depend on chunk_bytes.  It uses both lanes, so a pending device result does not
 * survive it; the counts slot afterwards holds the file's counts.  The report's keys are those of yttm_encode_file plus "seconds_count". */
int yttm_encode_file_counts(yttm_encoder *enc, const char *path, int bos, int eos, int reverse, double dropout_prob, uint64_t chunk_bytes,
                            uint64_t *counts, uint64_t *n_lines, uint64_t *n_ids, char *report_json, int report_len, char *err, int errlen);

/* Training blocks: sentences of ids packed into rows of exactly seq_len ids on the device (the reference has no counterpart).
 * Input: a sequence of sentences, each a list of int32 ids in stored order (ids[K], uint64 offsets[S + 1]).
 * Parameters: seq_len L, 1 <= L <= 2^24 (outside that range: code 1; it bounds the open row's buffer); mode, 0 = stream, 1 = whole; pad_value, any
 * int32; tail, 0 = pad, 1 = keep, 2 = drop.
 * An empty sentence contributes nothing anywhere.
 * The open row: the encoder owns one open row.  It holds fewer than L ids with their sentence boundaries, starts empty, and is bound to
 * (L, mode): a call with another L or mode while it is non-empty returns code 1 and changes nothing.  A call packs the sequence
 * "open row ++ the call's sentences".
 * Stream mode: the ids of all sentences are concatenated; row r holds positions [r L, (r + 1) L) of that stream.
 * Whole mode: next-fit in order.  A sentence joins the current row if the row's ids plus its own are <= L; otherwise the row is closed and the
 * sentence starts a new one; a row that reaches exactly L ids is closed.  A sentence longer than L is an error, as yttm_encode_copy_padded
 * refuses width < longest: code 1, the message naming the sentence's index and length; nothing is written and the open row is unchanged.
 * tail: after the complete rows one incomplete row of f ids (0 < f < L) may remain.  tail = 0 emits it with pad_value behind its ids and empties
 * the open row; tail = 1 emits nothing for it and makes it the new open row; tail = 2 discards it and empties the open row.
 * A fragment is a maximal run of ids inside one row that belong to one sentence; in whole mode the fragments are exactly the non-empty
 * sentences, in order.
 * Result, for n_rows rows and n_frags fragments:
 *   int32  rows[n_rows][L]        the ids; pad_value on padding
 *   int32  seg[n_rows][L]         1-based ordinal of the id's fragment within its row; 0 on padding
 *   int32  pos[n_rows][L]         index of the id within its fragment, so a fragment at a row's start begins at 0 even when its sentence began in
 *                                 the row before; 0 on padding
 *   int32  frags[n_frags][2]      (flat start r L + c, length), in ascending order
 *   uint64 row_frags[n_rows + 1]  row r's fragments are frags[row_frags[r] .. row_frags[r + 1])
 * Limit: a call whose n_rows L exceeds 2^31 - 1 returns code 1 (and changes nothing).
 * Consequences: in both modes the rows with padding removed, concatenated, are the input ids in order (but for the ids tail = 2 drops or tail = 1
 * keeps); with tail = 1 on every call but the last, the rows of several calls concatenated are the rows of one call on the concatenated
 * input; in stream mode only the last row can hold padding.
 *
 * yttm_blocks_device packs the pending encode result, whichever call left it (n_sent must be its, as for yttm_idtext_device); the result stays
 * pending and unchanged.  yttm_blocks_ids_device: the same over int32 d_ids[n_ids] + uint64 d_offsets[n_sent + 1] in HBM that the encoder did not
 * make (offsets[0] = 0, the conventions of yttm_decode_device: 4-byte aligned ids, the caller synchronises the stream that wrote them first).
 * The blocks live in a slot of the encoder's own: only the next blocks call replaces it.  kernel_ms (optional) = HIP-event time of all passes.
 * yttm_blocks_flush: the open row as a result of 0 or 1 rows (its tail padded); the open row is then empty.
 * yttm_blocks_open: out = {ids in the open row, its L, its mode} (zeroes when it is empty).  yttm_blocks_discard empties the open row -- the reset,
 * a call of its own so that no argument of another call has a second meaning.
 * yttm_blocks_fetch / yttm_blocks_copy_device: the five arrays to host memory / to device memory the caller owns; any null pointer is skipped;
 * n_rows and n_frags must match the slot's, else code 1.  (seg and pos are kept in the slot: both exits are plain copies.) */
int yttm_blocks_device(yttm_encoder *enc, uint64_t n_sent, uint64_t seq_len, int mode, int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags,
                       double *kernel_ms, char *err, int errlen);
int yttm_blocks_ids_device(yttm_encoder *enc, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, uint64_t seq_len, int mode,
                           int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags, double *kernel_ms, char *err, int errlen);
int yttm_blocks_flush(yttm_encoder *enc, int32_t pad_value, uint64_t *n_rows, uint64_t *n_frags, double *kernel_ms, char *err, int errlen);
int yttm_blocks_open(yttm_encoder *enc, uint64_t out[3]);
int yttm_blocks_discard(yttm_encoder *enc);
int yttm_blocks_fetch(yttm_encoder *enc, int32_t *rows, int32_t *seg, int32_t *pos, int32_t *frags, uint64_t *row_frags, uint64_t n_rows, uint64_t n_frags,
                      char *err, int errlen);
int yttm_blocks_copy_device(yttm_encoder *enc, void *d_rows, void *d_seg, void *d_pos, void *d_frags, void *d_row_frags, uint64_t n_rows, uint64_t n_frags,
                            char *err, int errlen);
/* The pipeline of yttm_encode_file with the packing in place of the download of ids: every piece is packed with tail = 1, the last piece is
 * followed by the flush (tail = 0) or the drop (tail = 2; any other value: code 1).  It writes PREFIX.rows (int32 [n_rows][L]) and PREFIX.frags
 * (uint64 [n_frags][2], the starts flat over the whole file); with dropout_prob == 0 the two files do not depend on chunk_bytes.  The same
 * file errors and <BOS> / <EOS> messages as yttm_encode_file; a sentence longer than L in whole mode names its line number in the file (from 1).
 * It starts from an empty open row and leaves it empty; it uses both lanes, so a pending device result does not survive it.  The report's keys
 * are those of yttm_encode_file plus "rows", "frags" and "seconds_blocks". */
int yttm_encode_file_blocks(yttm_encoder *enc, const char *path, const char *out_prefix, int bos, int eos, int reverse, double dropout_prob,
                            uint64_t chunk_bytes, uint64_t seq_len, int mode, int32_t pad_value, int tail, uint64_t *n_rows, uint64_t *n_frags,
                            uint64_t *n_lines, uint64_t *n_ids, char *report_json, int report_len, char *err, int errlen);

/* Batches by length under a token budget: sentences sorted by length and cut into batches, each a padded matrix as narrow as its longest
 * sentence (fairseq's --max-tokens / --max-sentences, OpenNMT's batch_type tokens; the reference has no counterpart).
 * Input: n sentences with lengths l(0) .. l(n - 1) >= 0; n < 2^32 - 2, as for the training blocks.
 * Parameters: max_tokens T, 1 .. 2^31 - 1; max_sentences M, 0 = no limit, else 1 .. 2^31 - 1; min_len >= 0; max_len, 0 = none.  Anything outside
 * those ranges: code 1, and nothing is changed.
 * Kept and left out: sentence i is kept iff min_len <= l(i) and (max_len == 0 or l(i) <= max_len).  Every other sentence is left out and appears
 * in no batch.  A kept sentence with l(i) > T fits no batch: code 1, the message naming the smallest such i and its length; the slot, the pending
 * result and any earlier plan are unchanged.  (A negative length -- yttm_batches_plan_lengths_device -- is refused the same way; of the sentences
 * the rule refuses for either reason the message names the one of the smallest index.)
 * Order: uint32 order[n] holds the kept sentences by (l, i) ascending -- a stable sort by length --, then the left-out ones by i ascending.
 * n_kept is returned.
 * Batches: ranges of positions of order[0 .. n_kept).  A batch that starts at position a ends at the largest b <= n_kept with both
 *   b - a <= M (when M != 0)   and   (b - a) * l(order[b - 1]) <= T.
 * The order ascends, so the last sentence of a batch is its longest and the product its padded size; b >= a + 1 always holds.  The next batch
 * starts at b.  uint64 batch_first[n_batches + 1], the last entry = n_kept; n_kept == 0 gives n_batches == 0.
 * Consequences: every batch is within both limits; every batch but the last is maximal (its next sentence would break a limit); a batch of
 * empty sentences has width 0 and is bounded by M alone.
 * Gather: the batches of one side -- int32 ids[K] + uint64 offsets[n + 1] with the plan's n: the planned side, or another one with lengths of
 * its own:
 *   uint32 widths[n_batches]          the largest length of this side among the batch's sentences
 *   uint64 batch_off[n_batches + 1]   the exclusive sum of rows_b * widths_b
 *   int32  out[batch_off[n_batches]]  batch b as a row-major matrix [rows_b][widths_b] at batch_off[b]; row k is sentence
 *                                     order[batch_first[b] + k], its ids at the left with pad_value behind them -- with left_pad != 0 at the right
 *                                     with pad_value in front
 * More than 2^31 - 1 elements: code 1, and nothing is changed.
 * Two sides: plan with lengths = max(len_src, len_tgt) (yttm_batches_plan_lengths_device) and gather each side with that plan; the budget then
 * holds for the wider side of every batch.
 *
 * yttm_batches_plan_device plans from the offsets of the pending encode result, whichever call left it (n_sent must be its); the result stays
 * pending and unchanged.  yttm_batches_plan_lengths_device: from int32 d_lengths[n_sent] in HBM (4-byte aligned; the caller synchronises the
 * stream that wrote them first).  yttm_batches_gather_device gathers the pending result, yttm_batches_gather_ids_device int32 d_ids[n_ids] + uint64
 * d_offsets[n_sent + 1] in HBM (offsets[0] = 0; 4-byte aligned ids, 8-byte aligned offsets, the conventions of yttm_blocks_ids_device).  Both
 * return code 1 where there is no plan or n_sent is not the plan's.  kernel_ms (optional) = HIP-event time of all passes.
 * The plan and the gathered arrays live in a slot of the encoder's own: no encode, decode, parse, count, blocks or file call empties it; a plan
 * call replaces the plan and empties the gathered part; a gather replaces the gathered part only.
 * yttm_batches_fetch / yttm_batches_copy_device: the five arrays to host memory / to device memory the caller owns; any null pointer is skipped;
 * n_sent, n_batches and n_elems must be the slot's (n_elems = 0 and no widths, batch_off or out while nothing is gathered), else code 1. */
int yttm_batches_plan_device(yttm_encoder *enc, uint64_t n_sent, uint64_t max_tokens, uint64_t max_sentences, uint64_t min_len, uint64_t max_len,
                             uint64_t *n_kept, uint64_t *n_batches, double *kernel_ms, char *err, int errlen);
int yttm_batches_plan_lengths_device(yttm_encoder *enc, const void *d_lengths, uint64_t n_sent, uint64_t max_tokens, uint64_t max_sentences, uint64_t min_len,
                                     uint64_t max_len, uint64_t *n_kept, uint64_t *n_batches, double *kernel_ms, char *err, int errlen);
int yttm_batches_gather_device(yttm_encoder *enc, uint64_t n_sent, int32_t pad_value, int left_pad, uint64_t *n_elems, double *kernel_ms, char *err, int errlen);
int yttm_batches_gather_ids_device(yttm_encoder *enc, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, int32_t pad_value, int left_pad,
                                   uint64_t *n_elems, double *kernel_ms, char *err, int errlen);
int yttm_batches_fetch(yttm_encoder *enc, uint32_t *order, uint64_t *batch_first, uint32_t *widths, uint64_t *batch_off, int32_t *out, uint64_t n_sent,
                       uint64_t n_batches, uint64_t n_elems, char *err, int errlen);
int yttm_batches_copy_device(yttm_encoder *enc, void *d_order, void *d_batch_first, void *d_widths, void *d_batch_off, void *d_out, uint64_t n_sent,
                             uint64_t n_batches, uint64_t n_elems, char *err, int errlen);

/* Encode under a restricted vocabulary (subword-nmt's --vocabulary / --vocabulary-threshold, SentencePiece's SetVocabulary; the reference has no
 * counterpart).  A model has rules (x, y, z) with distinct z, as written in the model file behind the char section.  Let V = yttm_vocab_size(enc)
 * and A, a subset of [0, V), the allowed set.  The expansion E(v) of an id:
 *   E(v) = [v]            if v is outside [0, V) -- no id is an error, as in the id counts;
 *   E(v) = [v]            if v is in A;
 *   E(v) = [v]            if v is no rule's z: chars, <PAD>, <UNK>, <BOS>, <EOS> -- a leaf stays even when it is not allowed, as in subword-nmt;
 *   E(v) = E(x) ++ E(y)   otherwise, for the one rule with z == v.
 * A sentence's restricted ids are the concatenation of E(id) over its ids in forward order; of a sentence that is stored back to front
 * (reverse) the restricted result is the reverse of that: each stored id is replaced by E(id) reversed.  So: decoding the restricted ids gives
 * the bytes that decoding the originals gives; the units the tokens cover (the spans' rule above) sum to the same value, so spans and SUBWORD
 * text stay well defined; restricting twice equals restricting once; A = [0, V) is the identity.  Every expansion is made without regard to
 * its neighbours: this is NOT the encoding a model trained with fewer merges would give (such a model could merge the pieces differently).
 *
 * yttm_encoder_set_vocabulary: allowed[n], n == V (else code 1), non-zero = allowed; allowed == NULL clears the vocabulary (n is not looked at).
 * It builds exp_off[V + 1] and exp_ids[] in rule order, and the same with every expansion reversed, in HBM.  From then on EVERY encode of this
 * encoder -- ids, tensors, padded matrices, SUBWORD text, id text, spans, counts, files, the command line -- gives restricted ids: a pass
 * (k_restrict.h: measure, scan, write) runs behind the encode kernel; n_ids and kernel_ms of those calls include it.  Off unless asked for:
 * with no vocabulary set nothing changes.  The call waits for both of the encoder's lanes; a result already pending is not changed.  info
 * (optional): {allowed ids, ids whose expansion is longer than one id, the longest expansion}.
 * yttm_encoder_vocabulary_stats: {restricted calls, calls where nothing split, ids in, ids out} since the encoder was made. */
int yttm_encoder_set_vocabulary(yttm_encoder *enc, const uint8_t *allowed, uint64_t n, uint64_t *info, char *err, int errlen);
int yttm_encoder_vocabulary_stats(yttm_encoder *enc, uint64_t out[4]);
/* The pass over ids the encoder did not make: int32 d_ids[n_ids] + uint64 d_offsets[n_sent + 1] in HBM (offsets[0] = 0, the conventions of
 * yttm_decode_device: 4-byte aligned ids, the caller synchronises the stream that wrote them first).  reverse: the sentences are stored back to
 * front.  It leaves a pending encode result of n_sent sentences and *n_out ids, exactly as after yttm_encode_device (yttm_encode_fetch,
 * yttm_encode_copy_device, yttm_encode_copy_padded, yttm_idtext_device, yttm_id_counts_device); the spans slot is emptied.  No vocabulary set:
 * code 1, and nothing pending is replaced.  kernel_ms (optional) = measure + scan + write. */
int yttm_restrict_ids_device(yttm_encoder *enc, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, int reverse,
                             uint64_t *n_out, double *kernel_ms, char *err, int errlen);

/* Byte fallback (SentencePiece's byte_fallback; the reference has no counterpart: a maximal run of valid, non-space code points outside the
 * model's alphabet becomes ONE unk_id, SURVEY.md A.7, and the run's text is gone from the ids).  A setting of an encoder, as the restricted
 * vocabulary is; the model file does not change.  Let V = yttm_vocab_size(enc).  The byte id of byte b is V + b, 0 <= b <= 255.
 * Encode, setting on: take the ids the encoder makes with the setting off, in forward order.  The k-th unk_id of a sentence stands for the
 *   sentence's k-th unknown run (a maximal run of valid non-space code points outside the alphabet; invalid bytes inside it are dropped and do
 *   not end it).  That one id is replaced by V + b for every byte b of the run's valid characters, in text order.  Every other id stays: bos_id,
 *   eos_id, the space token and merged tokens.  A sentence stored back to front (reverse) holds the reverse of the forward result as a whole:
 *   a run's bytes are back to front, and the k-th stored unk_id of a sentence with n of them is run n - 1 - k.  Dropout does not change the
 *   correspondence (rules never match placeholders).  A restricted vocabulary commutes with it: byte ids lie outside [0, V) and pass through E,
 *   unk_id is a leaf.  n_ids and kernel_ms of every encode include the pass (k_bytefb.h: measure, scan, write; the write pass is skipped only
 *   where the measure pass met no unk_id -- a run of one ASCII char keeps the number of ids and still changes one).
 * The stand-alone entry takes ids that did not come from this call: an unk_id whose sentence has no such run stays unk_id, runs beyond the
 *   sentence's unk_ids are ignored, no id is ever lost.
 * Decode, setting on: an id in [V, V + 256) is valid, its piece is the single raw byte, no strip rule applies to it, and it can be named in
 *   ignore_ids.  Ids >= V + 256 or < 0 keep the error and its message.  The bytes come out verbatim: ids the caller made up may form invalid
 *   UTF-8, and the byte and tensor routes return them as they are.  (The device decode strips a leading V + 0x20 of a sentence as it strips
 *   the space of a first piece; no encode makes that id, a space is never part of a run.)
 * Names, setting on: yttm_id_to_subword(V + b) is <0xNN>, two upper-case hex digits; yttm_subword_to_id("<0xNN>") is V + b; SUBWORD text
 *   prints a byte id as that one piece followed by a space.  yttm_vocab_size and yttm_vocabulary do not change.
 * Counts, setting on: n_bins == 0 means V + 256, and yttm_encode_file_counts writes V + 256 + 1 integers: the caller's counts hold that many.
 * Spans are not defined under byte fallback (several ids would share one unit): yttm_spans_device, yttm_spans_text_device and
 *   yttm_encode_as_ids_spans return code 1 with a message before any work, and what was pending stays.
 * Setting off: every call behaves as if the setting did not exist.
 *
 * yttm_encoder_set_byte_fallback waits for both of the encoder's lanes; a result already pending is not changed.  yttm_encoder_byte_fallback:
 * 0 or 1.  yttm_encoder_byte_fallback_stats: {calls of the pass, calls whose write pass was skipped, ids in, ids out} since the encoder was made. */
int yttm_encoder_set_byte_fallback(yttm_encoder *enc, int on, char *err, int errlen);
int yttm_encoder_byte_fallback(yttm_encoder *enc);
int yttm_encoder_byte_fallback_stats(yttm_encoder *enc, uint64_t out[4]);
/* The pass over ids the encoder did not make and the text they were made from, all in HBM: int32 d_ids[n_ids] + uint64 d_id_offsets[n_sent + 1]
 * (the conventions of yttm_restrict_ids_device), sentence s = d_bytes[d_text_offsets[s] .. d_text_offsets[s + 1]), total_bytes in all.  It leaves
 * a pending encode result of n_sent sentences and *n_out ids, exactly as after yttm_encode_device; the spans slot is emptied.  All inputs are
 * only read.  Setting off: code 1, and nothing pending is replaced.  kernel_ms (optional) = measure + scan + write. */
int yttm_byte_fallback_ids_device(yttm_encoder *enc, const void *d_ids, const void *d_id_offsets, const void *d_bytes, const void *d_text_offsets,
                                  uint64_t n_sent, uint64_t n_ids, uint64_t total_bytes, int reverse, uint64_t *n_out, double *kernel_ms, char *err,
                                  int errlen);

/* Added tokens (SentencePiece's user_defined_symbols, Hugging Face's added tokens; the reference has no counterpart): literal byte strings --
 * language tags, separators, <mask>, sentinels, chat markers -- that are one id each and never split.  A setting of an encoder, as the restricted
 * vocabulary and the byte fallback are; the model file does not change.  Let V = yttm_vocab_size(enc) and A = V + 256.
 * The setting: yttm_encoder_set_added_tokens takes n byte strings t_0 .. t_{n-1} as a blob plus tok_offsets[n + 1], in the caller's order.
 *   1 <= n <= 4096; each string is 1 .. 255 bytes of valid UTF-8 without a code point the encoder treats as white space (0x0A included) and
 *   without U+2581; the strings are pairwise different; A + n lies within the encoder's id limit.  A string may be a prefix or a substring of
 *   another.  Anything else: code 1 with a message, and the setting stays as it was.  blob == NULL clears the setting.  The call waits for both
 *   of the encoder's lanes, as yttm_encoder_set_vocabulary does; a result already pending is not changed.  The id of t_k is A + k, whether the
 *   byte fallback is on or off.
 * Matching is byte-wise and per sentence text[off[s] .. off[s + 1]): leftmost first, the longest at a position, non-overlapping.
 *   p = off[s]; while p < off[s + 1]: among the t_k with text[p .. p + len_k) == t_k and p + len_k <= off[s + 1] take the longest; if there is
 *   one it is a match (p, k) and p += len_k, otherwise p += 1.  A match never crosses a sentence boundary.  A sentence with the matches
 *   m_1 .. m_j is cut into the segments g_0 .. g_j: the text in front of, between and behind the matches; a segment may be empty.
 * Encode, setting on: the forward result of the sentence is
 *     [bos_id]? ++ E(g_0) ++ [A + k(m_1)] ++ E(g_1) ++ ... ++ [A + k(m_j)] ++ E(g_j) ++ [eos_id]?
 *   where E(g) is the ids the same encoder makes for g as a sentence of its own with bos = eos = reverse = false, under the encoder's other
 *   settings (the restricted vocabulary, the byte fallback): E of an empty or all-space segment is [], a segment that starts inside a word gets
 *   its own U+2581.  reverse stores the reverse of the forward result as a whole, bos and eos included.  Dropout: the segments
 *   are encoded as ONE batch, the refined batch, whose sentences are g_0, m_1, g_1, .., m_j, g_j of every sentence in text order (2 j + 1 per
 *   sentence), in one pass under the call's salt: with YTTM_DROPOUT_SEED pinned the ids are exactly the join of what yttm_encode_device returns
 *   for that refined batch with the setting off.  Where no sentence of a call holds a match the refined batch is the batch and the ids are the
 *   setting-off ids.  n_ids and kernel_ms include all passes (k_added.h: the split, the encode of the refined batch, the join).
 * Restricted vocabulary: an added id lies outside [0, V) and passes through the restriction.
 * Decode: an id in [A, A + n) is valid, its piece is t_k verbatim, no strip rule applies to it, and it can be named in ignore_ids.  Ids >= A + n
 *   or < 0 keep the error and its message; [V, A) stays an error while the byte fallback is off.
 * Names: yttm_id_to_subword(A + k) is t_k, yttm_subword_to_id(t_k) is A + k.  yttm_vocab_size and yttm_vocabulary do not change.
 * Counts: n_bins == 0 means A + n, and yttm_encode_file_counts writes A + n + 1 integers.
 * Id text, blocks, batches, padded copies, tensors, the sub-batches of a large host batch and file pieces read the pending result or encode
 *   through the same path: they get the setting without code of their own (file pieces are cut at newlines, and no token holds one).
 * Spans are not defined with the setting on: yttm_spans_device, yttm_spans_text_device and yttm_encode_as_ids_spans return code 1 with a message
 *   before any work, and what was pending stays.
 * SUBWORD text (yttm_subword_device, yttm_subword_text_device, yttm_encode_file_subword, yttm_encode_as_subwords, yttm_encode_cli) maps the k-th
 *   unk_id of a sentence to the k-th unknown run of its ORIGINAL text, and a match's text can add to a run or join two: these routes are defined
 *   only with the byte fallback on as well (then no unk_id is left and the text is never consulted); an added id prints as t_k and a space.
 *   With the byte fallback off they return code 1 before any work.
 * Setting off: every call behaves as if the setting did not exist.
 *
 * yttm_encoder_added_tokens: the set as a blob and tok_offsets[n + 1] (both released with yttm_free) and n; n == 0 while nothing is set.
 * yttm_encoder_added_tokens_stats: {calls with the setting on, calls without a match (the split's write pass and the join were skipped),
 * matches, sub-sentences encoded} since the encoder was made. */
int yttm_encoder_set_added_tokens(yttm_encoder *enc, const uint8_t *blob, const uint64_t *tok_offsets, uint64_t n, char *err, int errlen);
int yttm_encoder_added_tokens(yttm_encoder *enc, char **blob, uint64_t **tok_offsets, uint64_t *n);
int yttm_encoder_added_tokens_stats(yttm_encoder *enc, uint64_t out[4]);
/* The split alone, of a text in HBM: sentence s = d_bytes[d_offsets[s] .. d_offsets[s + 1]), total_bytes in all -> the refined batch.  It lives
 * in a slot of the encoder's own that the next split replaces: uint64 sub_first[n_sent + 1] (the first sub-sentence of sentence s; sub_first[n_sent]
 * = *n_sub = n_sent + 2 * *n_matches), uint64 sub_offsets[n_sub + 1] (sub-sentence i = d_bytes[sub_offsets[i] .. sub_offsets[i + 1])) and int32
 * tok[n_sub] (the token's index for a match, -1 for a segment).  The inputs are only read.  Setting off: code 1, and nothing is replaced.
 * _fetch copies the arrays to host memory, _copy_device into device memory the caller owns; n_sent and n_sub must be the slot's (code 1
 * otherwise); a null pointer is skipped.  kernel_ms (optional) = measure + scan + write. */
int yttm_added_split_device(yttm_encoder *enc, const void *d_bytes, const void *d_offsets, uint64_t n_sent, uint64_t total_bytes, uint64_t *n_sub,
                            uint64_t *n_matches, double *kernel_ms, char *err, int errlen);
int yttm_added_split_fetch(yttm_encoder *enc, uint64_t *sub_first, uint64_t *sub_offsets, int32_t *tok, uint64_t n_sent, uint64_t n_sub, char *err,
                           int errlen);
int yttm_added_split_copy_device(yttm_encoder *enc, void *d_sub_first, void *d_sub_offsets, void *d_tok, uint64_t n_sent, uint64_t n_sub, char *err,
                                 int errlen);

/* Word-level encode cache (SURVEY.md 8f "N4"; the reference has no counterpart: bpe.cpp:1497-1632 encodes every word occurrence).
 * mode 0: every batch goes straight through the encode kernel; 1: distinct words are encoded once whenever that is possible
 * (dropout_prob == 0); 2 (default): the same for batches of at least min_bytes.  The ids are identical either way.
 * yttm_encode_cache_words: distinct words of the last yttm_encode_device batch, 0 if it did not go through the cache. */
int yttm_encoder_set_cache(yttm_encoder *enc, int mode, uint64_t min_bytes);
uint64_t yttm_encode_cache_words(yttm_encoder *enc);

/* Status id_to_subword(int id, string* subword, bool replace_space) bpe.h:48, bpe.cpp:1774; yttm.pyx:129-134 */
int yttm_id_to_subword(yttm_encoder *enc, int id, char **subword, char *err, int errlen);
/* int subword_to_id(const string& token) const                       bpe.h:50, bpe.cpp:1809; yttm.pyx:126-127 */
int yttm_subword_to_id(yttm_encoder *enc, const char *token);
/* Status decode(const vector<vector<int>>& ids, vector<string>* sentences, const unordered_set<int>* ignore_ids)
 *                                                                     bpe.h:52-54, bpe.cpp:1828; yttm.pyx:136-158 */
int yttm_decode(yttm_encoder *enc, const int32_t *ids, const uint64_t *offsets, uint64_t n_sent, const int32_t *ignore_ids,
                uint64_t n_ignore, char **blob, uint64_t **out_offsets, char *err, int errlen);
/* Device-resident batch decode.  ids/offsets already in HBM (int32[n_ids], uint64[n_sent+1]); ignore_ids is a host array.  The text stays in HBM
 * inside the encoder until yttm_decode_fetch / yttm_decode_copy_device takes it (char bytes[*n_bytes], uint64 out_offsets[n_sent+1]); it does not
 * replace a pending yttm_encode_device result, nor the other way round.  An id outside [0, vocab_size) that is not ignored fails the call with
 * the message and code (1) of yttm_decode, naming the first such id in sentence order, then position order.  kernel_ms (optional) = HIP-event
 * time of measure + scan + write.  The caller makes ids/offsets visible first (synchronises the stream that wrote them).
 * replaces: BaseEncoder::decode, bpe.h:52-54, bpe.cpp:1828-1861 (on id_to_subword(id, &s, true), bpe.cpp:1774-1807) */
int yttm_decode_device(yttm_encoder *enc, const void *d_ids, const void *d_offsets, uint64_t n_sent, uint64_t n_ids, const int32_t *ignore_ids,
                       uint64_t n_ignore, uint64_t *n_bytes, double *kernel_ms, char *err, int errlen);
/* the same for a padded matrix: row i = d_ids[i*row_stride .. i*row_stride + len_i), len_i = d_lengths ? d_lengths[i] : width
 * (d_lengths: int32[n_sent] in HBM or NULL; a length outside [0, width] counts as 0 or width); row_stride >= width.  bpe.cpp:1828-1861 */
int yttm_decode_device_padded(yttm_encoder *enc, const void *d_ids, uint64_t n_sent, uint64_t width, uint64_t row_stride, const void *d_lengths,
                              const int32_t *ignore_ids, uint64_t n_ignore, uint64_t *n_bytes, double *kernel_ms, char *err, int errlen);
/* the text of the last yttm_decode_device[_padded]: to host arrays / to device memory the caller owns.  bpe.cpp:1828-1841 (the batch loop) */
int yttm_decode_fetch(yttm_encoder *enc, char *bytes, uint64_t *out_offsets, uint64_t n_sent, char *err, int errlen);
int yttm_decode_copy_device(yttm_encoder *enc, void *d_bytes, void *d_out_offsets, uint64_t n_sent, char *err, int errlen);
/* int vocab_size() const                                              bpe.h:62, bpe.cpp:1692; yttm.pyx:160-161 */
int yttm_vocab_size(yttm_encoder *enc);
/* vector<string> vocabulary() const                                   bpe.h:64, bpe.cpp:1884; yttm.pyx:163-165 */
int yttm_vocabulary(yttm_encoder *enc, char **blob, uint64_t **offsets, uint64_t *n);

/* The streaming loops of the `yttm` command line.  The reference's read std::cin and write std::cout; here the file
 * descriptors are arguments (the Python module passes 0 and 1).
 * Status encode_cli(const string& output_type, bool stream, bool bos, bool eos, bool reverse, double dropout_prob) const
 *                                                                     bpe.h:66-68, bpe.cpp:1942-2014; yttm.pyx:167-170
 * batch mode: stdin in batches of >= 10 MiB of line bytes -> H2D / K5 / D2H of one batch overlapped with the formatting of
 * the previous one (two encoder lanes) -> "<token> <token> ...\n" per sentence (utils.h:92-103); progress on stderr. */
int yttm_encode_cli(yttm_encoder *enc, const char *output_type, int stream, int bos, int eos, int reverse, double dropout_prob,
                    int in_fd, int out_fd, char *err, int errlen);
/* Status decode_cli(const unordered_set<int>* ignore_ids) const       bpe.h:70, bpe.cpp:2016-2028; yttm.pyx:172-178 */
int yttm_decode_cli(yttm_encoder *enc, const int32_t *ignore_ids, uint64_t n_ignore, int in_fd, int out_fd, char *err, int errlen);
/* void vocab_cli(bool verbose) const                                  bpe.h:71, bpe.cpp:1896-1940; yttm.pyx:180-181 */
int yttm_vocab_cli(yttm_encoder *enc, int verbose, int out_fd, char *err, int errlen);

/* ---- multi-GPU (one process per GPU) ---------------------------------------------------------------
 * The corpus shards across ranks; the only exchanged quantities are the char histogram (once) and sparse pair-count
 * deltas (after the initial count and after every merge round) -- the RCCL form of the reference's main thread summing
 * per-thread maps (bpe.cpp:1099-1108, :1245-1251).  Every rank passes ITS shard to the *_comm entry points; rank 0
 * writes the model file. */
typedef struct yttm_comm yttm_comm;
/* RCCL over xGMI: rank 0 makes the id, the application broadcasts its 128 bytes, every rank creates its communicator */
int yttm_comm_rccl_unique_id(uint8_t out[128]);
int yttm_comm_rccl_create(const uint8_t id[128], int rank, int world, int device, yttm_comm **out);
/* host-callback transport (torch.distributed/gloo, MPI, ...): in-place sum of n uint64; gather of the other ranks' bytes */
typedef int (*yttm_allreduce_u64_fn)(void *user, unsigned long long *buf, size_t n);
typedef int (*yttm_allgather_bytes_fn)(void *user, const void *send, size_t send_bytes, void *recv, size_t recv_cap,
                                       unsigned long long *recv_bytes);
int yttm_comm_callback_create(int rank, int world, yttm_allreduce_u64_fn allreduce, yttm_allgather_bytes_fn allgather,
                              void *user, yttm_comm **out);
void yttm_comm_destroy(yttm_comm *comm);
/* train_bpe (bpe.h:19) on a node of GPUs: every rank passes the SAME file and reads its own byte range of it, cut at white space like the
 * reference's per-thread split (bpe.cpp:864-873).  comm == NULL: one GPU (yttm_train_bpe_ex with the per-kernel timers: profile = 1). */
int yttm_train_bpe_comm(const char *input_path, const char *model_path, int vocab_size, double coverage, int n_threads, int pad_id,
                        int unk_id, int bos_id, int eos_id, int device, int profile, yttm_comm *comm, char *report_json,
                        int report_len, char *err, int errlen);
int yttm_train_bpe_from_device_comm(const void *d_text, uint64_t n, const char *model_path, int vocab_size, double coverage,
                                    int pad_id, int unk_id, int bos_id, int eos_id, int device, int profile,
                                    yttm_comm *comm, char *report_json, int report_len, char *err, int errlen);
int yttm_train_bpe_from_memory_comm(const uint8_t *text, uint64_t n, const char *model_path, int vocab_size, double coverage,
                                    int pad_id, int unk_id, int bos_id, int eos_id, int device, yttm_comm *comm,
                                    char *report_json, int report_len, char *err, int errlen);

/* Checksum of an encode result for comparisons across implementations: FNV-1a-64 over, per sentence, the little-endian
 * bytes of the uint32 length and of each int32 id (no reference counterpart; oracle/ref_driver.cpp hashes the reference's
 * encode_as_ids output the same way). */
unsigned long long yttm_ids_fnv1a64(const int32_t *ids, const uint64_t *offsets, uint64_t n_sent);

void yttm_free(void *p);
/* "gfx950 MI355X ..." or an error text when no usable GPU is visible */
int yttm_device_info(int device, char *buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif
