// added_plan.h -- the limits, the id ranges, the table sizes and the token validation of the added tokens (the rule is in
// include/yttm_mi355x.h "Added tokens"): which ids are added ids, the bound the kernels and the host loops accept under the two settings that
// lie behind the vocabulary, the sizes of the piece tables and of the matcher's directory, and what a token set must satisfy.
// Plain C++ without HIP, so that tools/dbg/check_added_plan.cpp can walk it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bytefb_plan.h"

namespace yttm {

constexpr uint32_t ADDED_MAX_TOKENS = 4096;  // n of yttm_encoder_set_added_tokens
constexpr uint32_t ADDED_MAX_BYTES = 255;    // bytes of one token
constexpr uint32_t ADDED_DIR = 4096;         // buckets of the matcher's directory (a power of two), keyed by a token's two leading bytes
constexpr uint32_t ADDED_NO_TOKEN = 0xffffffffu;

// the first added id: behind the 256 byte ids, whether the byte fallback is on or off
static inline uint32_t added_first(uint32_t V) { return V + BYTE_IDS; }
// the ids a decode, a SUBWORD format, a name lookup, the ignore bitmap and the counts' default bins accept: [0, bound); n_added == 0: the setting is off
static inline uint32_t added_bound(uint32_t V, bool byte_fallback, uint32_t n_added) { return n_added ? added_first(V) + n_added : bytefb_bound(V, byte_fallback); }
static inline bool added_is_added_id(long long id, uint32_t V, uint32_t n_added) {
  return id >= (long long)added_first(V) && id < (long long)added_first(V) + (long long)n_added;
}
// [V, V + 256) stays invalid under the added tokens while the byte fallback is off
static inline bool added_id_valid(long long id, uint32_t V, bool byte_fallback, uint32_t n_added) {
  if (id < 0) return false;
  if (id < (long long)V) return true;
  if (id < (long long)added_first(V)) return byte_fallback;
  return added_is_added_id(id, V, n_added);
}
// does V leave room for the byte ids and n added ids below the encoder's id limit?
static inline bool added_fits(uint32_t V, unsigned long long n) { return V <= BFB_VOCAB_MAX && n <= ADDED_MAX_TOKENS; }  // (2^30 - 16 + 256 + 4096 < 2^31)
// entries of a piece table's offsets: one per id of [0, V + 256 + n) and the end
static inline size_t added_table_offsets(uint32_t V, uint32_t n_added) { return bytefb_table_offsets(V) + n_added; }
// the directory's bucket of two leading bytes (the one function of this header that the kernels call too)
#if defined(__HIP__)
#define ADDED_HOST_DEVICE __attribute__((host)) __attribute__((device))
#else
#define ADDED_HOST_DEVICE
#endif
ADDED_HOST_DEVICE static inline uint32_t added_bucket(uint32_t b0, uint32_t b1) { return ((b0 | (b1 << 8)) * 0x9E3779B1u) >> 20; }
// An entry of the directory's lists, everything a lane needs about a token in one load: where its bytes start in the blob (bits 0 .. 31), its
// length (32 .. 39) and its index (40 .. 55)
ADDED_HOST_DEVICE static inline unsigned long long added_entry(uint32_t blob_off, uint32_t len, uint32_t k) {
  return (unsigned long long)blob_off | ((unsigned long long)len << 32) | ((unsigned long long)k << 40);
}
ADDED_HOST_DEVICE static inline uint32_t added_entry_off(unsigned long long e) { return (uint32_t)e; }
ADDED_HOST_DEVICE static inline uint32_t added_entry_len(unsigned long long e) { return (uint32_t)(e >> 32) & 0xffu; }
ADDED_HOST_DEVICE static inline uint32_t added_entry_tok(unsigned long long e) { return (uint32_t)(e >> 40) & 0xffffu; }
static_assert(ADDED_MAX_BYTES <= 0xffu && ADDED_MAX_TOKENS <= 0x10000u, "a list entry holds a token's length in 8 bits and its index in 16");
static_assert(ADDED_DIR == 1u << 12, "added_bucket keeps the upper 12 bits");

// One valid UTF-8 char at s[i ..): its length and code point, or 0 (the table of utf8.cpp: no overlong forms, no surrogates, at most U+10FFFF)
static inline uint32_t added_utf8_char(const uint8_t *s, size_t i, size_t n, uint32_t *cp) {
  const uint32_t b0 = s[i];
  if (b0 < 0x80u) {
    *cp = b0;
    return 1;
  }
  const uint32_t len = (b0 >> 5) == 6u ? 2u : (b0 >> 4) == 14u ? 3u : (b0 >> 3) == 30u ? 4u : 0u;
  if (!len || i + len > n) return 0;
  uint32_t v = b0 & (0xffu >> (len + 1u));
  for (uint32_t k = 1; k < len; k++) {
    if ((s[i + k] & 0xc0u) != 0x80u) return 0;
    v = (v << 6) | (s[i + k] & 0x3fu);
  }
  if ((len == 2 && v < 0x80u) || (len == 3 && v < 0x800u) || (len == 4 && v < 0x10000u) || v > 0x10ffffu || (v >= 0xd800u && v <= 0xdfffu)) return 0;
  *cp = v;
  return len;
}
// the code points the encoder treats as white space (utf8.h is_space: U+2581 counts) -- a token holds none of them
static inline bool added_is_space(uint32_t cp) { return cp == 0x2581u || cp == 32u || (cp >= 9u && cp <= 13u); }

// What is wrong with the token set blob[off[0] .. off[n]) (empty string: nothing).  The message names the first offending token.
static inline std::string added_validate(const uint8_t *blob, const unsigned long long *off, unsigned long long n, uint32_t V) {
  if (n < 1 || n > ADDED_MAX_TOKENS) return "set_added_tokens: between 1 and 4096 tokens are accepted. Current value: n = " + std::to_string(n) + ";";
  if (!added_fits(V, n)) return "set_added_tokens: the vocabulary leaves no room for the added ids";
  std::vector<std::string> sorted;
  sorted.reserve((size_t)n);
  for (unsigned long long k = 0; k < n; k++) {
    const std::string at = "set_added_tokens: token " + std::to_string(k);
    if (off[k + 1] < off[k] || off[k + 1] - off[k] < 1 || off[k + 1] - off[k] > ADDED_MAX_BYTES) return at + " must be 1 to 255 bytes long";
    const uint8_t *s = blob + off[k];
    const size_t len = (size_t)(off[k + 1] - off[k]);
    for (size_t i = 0; i < len;) {
      uint32_t cp = 0;
      const uint32_t l = added_utf8_char(s, i, len, &cp);
      if (!l) return at + " is not valid UTF-8";
      if (added_is_space(cp)) return at + " holds white space or U+2581";
      i += l;
    }
    sorted.emplace_back((const char *)s, len);
  }
  std::sort(sorted.begin(), sorted.end());
  for (size_t k = 1; k < sorted.size(); k++)
    if (sorted[k] == sorted[k - 1]) return "set_added_tokens: the token \"" + sorted[k] + "\" is given twice";
  return std::string();
}

// The matcher's tables on the host, as the device gets them: the 256-bit set of first bytes, the one-byte tokens by their byte, and the
// directory -- bucket b lists the tokens of two and more bytes whose leading bytes hash to b, longest first (ties by index)
struct AddedTables {
  uint32_t first[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> one;      // [256]: the token that is this one byte, or ADDED_NO_TOKEN
  std::vector<uint32_t> dir_off;  // [ADDED_DIR + 1]
  std::vector<unsigned long long> list;  // added_entry of every token of two and more bytes, bucket after bucket
  std::vector<uint32_t> tok_off;         // [n + 1] into the blob
};
static inline AddedTables added_tables(const uint8_t *blob, const unsigned long long *off, uint32_t n) {
  AddedTables t;
  t.one.assign(256, ADDED_NO_TOKEN);
  t.dir_off.assign((size_t)ADDED_DIR + 1, 0);
  t.tok_off.resize((size_t)n + 1);
  std::vector<std::vector<uint32_t>> buckets(ADDED_DIR);
  for (uint32_t k = 0; k < n; k++) {
    const uint8_t *s = blob + off[k];
    const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
    t.tok_off[k] = (uint32_t)(off[k] - off[0]);
    t.first[s[0] >> 5] |= 1u << (s[0] & 31u);
    if (len == 1) t.one[s[0]] = k;
    else buckets[added_bucket(s[0], s[1])].push_back(k);
  }
  t.tok_off[n] = (uint32_t)(off[n] - off[0]);
  for (uint32_t b = 0; b < ADDED_DIR; b++) {
    std::stable_sort(buckets[b].begin(), buckets[b].end(), [&](uint32_t x, uint32_t y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
    t.dir_off[b] = (uint32_t)t.list.size();
    for (uint32_t k : buckets[b]) t.list.push_back(added_entry(t.tok_off[k], (uint32_t)(off[k + 1] - off[k]), k));
  }
  t.dir_off[ADDED_DIR] = (uint32_t)t.list.size();
  return t;
}

// the stand-alone split's algorithmic sizes: sub-sentences of n_sent sentences with n_matches matches
static inline unsigned long long added_n_sub(unsigned long long n_sent, unsigned long long n_matches) { return n_sent + 2 * n_matches; }

}  // namespace yttm
