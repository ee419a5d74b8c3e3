// bytefb_plan.h -- the id arithmetic of the byte fallback (the rule is in include/yttm_mi355x.h "Byte fallback"): which ids are byte ids, the
// bound the kernels and the host loops accept, the sizes of the tables that hold V + 256 entries, and the names <0xNN>.
// Plain C++ without HIP, so that tools/dbg/check_bytefb_plan.cpp can walk it over its whole input range under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace yttm {

constexpr uint32_t BYTE_IDS = 256;               // byte b is the id V + b
constexpr uint32_t BFB_VOCAB_MAX = 0x3ffffff0u;  // the encoder refuses models with ids of 2^30 - 16 and above: V + 256 stays an int32

// the ids a decode, a SUBWORD format, a name lookup or the ignore bitmap accept: [0, bound)
static inline uint32_t bytefb_bound(uint32_t V, bool on) { return V + (on ? BYTE_IDS : 0u); }
static inline bool bytefb_is_byte_id(long long id, uint32_t V, bool on) { return on && id >= (long long)V && id < (long long)V + (long long)BYTE_IDS; }
// entries of a piece table's offsets: one per id of [0, V + 256) and the end
static inline size_t bytefb_table_offsets(uint32_t V) { return (size_t)V + BYTE_IDS + 1; }
// words of the ignore bitmap over [0, bound), and one more (decode_on_lane appends the ids outside the bound behind it)
static inline size_t bytefb_bitmap_words(uint32_t bound) { return ((size_t)bound + 31) / 32 + 1; }
// n_bins == 0 of the counts
static inline unsigned long long bytefb_default_bins(uint32_t V, bool on) { return (unsigned long long)bytefb_bound(V, on); }

// "<0xNN>", two upper-case hex digits
static inline std::string bytefb_name(uint32_t b) {
  static const char HEX[] = "0123456789ABCDEF";
  std::string s = "<0x";
  s += HEX[(b >> 4) & 15u];
  s += HEX[b & 15u];
  s += '>';
  return s;
}
// the byte a name stands for, or -1 (lower-case digits are no names: id_to_subword never prints them)
static inline int bytefb_parse_name(const std::string &t) {
  if (t.size() != 6 || t.compare(0, 3, "<0x") != 0 || t[5] != '>') return -1;
  int v = 0;
  for (int k = 3; k < 5; k++) {
    const char c = t[(size_t)k];
    int d;
    if (c >= '0' && c <= '9') d = c - '0';
    else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
    else return -1;
    v = v * 16 + d;
  }
  return v;
}

}  // namespace yttm
