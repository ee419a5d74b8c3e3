// tools/dbg/check_added_plan.cpp -- walks the limits, the id ranges, the table sizes and the token validation of the added tokens
// (youtokentome_amd/csrc/added_plan.h) on the host, under the sanitizers (needs no GPU):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iyoutokentome_amd/csrc tools/dbg/check_added_plan.cpp -o /tmp/check_added_plan
//   /tmp/check_added_plan
// For every vocabulary size of a grid that holds every power of two and its neighbours up to the encoder's limit, with the byte fallback on and
// off and 0, 1, 2 and 4096 tokens: the first added id and the bound stay an int32, [V, V + 256) is valid exactly with the byte fallback on,
// exactly the ids V + 256 .. V + 256 + n - 1 are added ids, the piece tables hold an entry per id below V + 256 + n and the end (filled into
// real vectors: an index past the end is the sanitizer's).  Then the validation on every kind of invalid set, and the matcher's tables for
// sets of 1 to 4096 tokens: every token is found in its bucket (or, one byte long, by its byte), the buckets list longest first, the set of
// first bytes holds exactly the first bytes -- and a matcher written from those tables alone agrees with the loop of the rule.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "added_plan.h"

using namespace yttm;

static unsigned long long checked = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
      exit(1);                                                 \
    }                                                          \
    checked++;                                                 \
  } while (0)

struct Packed {
  std::vector<uint8_t> blob;
  std::vector<unsigned long long> off;
  explicit Packed(const std::vector<std::string> &toks) : off(1, 0) {
    for (const std::string &t : toks) {
      blob.insert(blob.end(), t.begin(), t.end());
      off.push_back(blob.size());
    }
    blob.push_back(0);  // (data() of an empty vector may be null)
  }
  std::string validate(uint32_t V = 600) const { return added_validate(blob.data(), off.data(), off.size() - 1, V); }
};

// the rule's loop: (position, token) of every match of one sentence
static std::vector<std::pair<size_t, uint32_t>> rule_matches(const std::string &text, const std::vector<std::string> &toks) {
  std::vector<std::pair<size_t, uint32_t>> out;
  for (size_t p = 0; p < text.size();) {
    size_t best = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; i < toks.size(); i++)
      if (toks[i].size() > best && p + toks[i].size() <= text.size() && text.compare(p, toks[i].size(), toks[i]) == 0) {
        best = toks[i].size();
        k = i;
      }
    if (best) {
      out.emplace_back(p, k);
      p += best;
    } else {
      p++;
    }
  }
  return out;
}
// the same from the tables, the way the kernel asks them
static std::vector<std::pair<size_t, uint32_t>> table_matches(const std::string &text, const std::vector<std::string> &toks, const AddedTables &t) {
  std::vector<std::pair<size_t, uint32_t>> out;
  for (size_t p = 0; p < text.size();) {
    const uint8_t c0 = (uint8_t)text[p];
    size_t len = 0;
    uint32_t k = 0;
    if ((t.first[c0 >> 5] >> (c0 & 31u)) & 1u) {
      if (p + 1 < text.size()) {
        const uint32_t b = added_bucket(c0, (uint8_t)text[p + 1]);
        for (uint32_t q = t.dir_off[b]; q < t.dir_off[b + 1] && !len; q++) {
          const uint32_t i = added_entry_tok(t.list[q]), l = added_entry_len(t.list[q]);
          if (p + l <= text.size() && text.compare(p, l, toks[i]) == 0) {
            len = l;
            k = i;
          }
        }
      }
      if (!len && t.one[c0] != ADDED_NO_TOKEN) {
        len = 1;
        k = t.one[c0];
      }
    }
    if (len) {
      out.emplace_back(p, k);
      p += len;
    } else {
      p++;
    }
  }
  return out;
}

int main() {
  // ---- the id ranges and the table sizes
  std::set<uint32_t> sizes{0u, 9u, 600u, 32000u, BFB_VOCAB_MAX};
  for (int b = 0; b < 30; b++)
    for (long long d = -2; d <= 2; d++) {
      const long long v = (1ll << b) + d;
      if (v >= 0 && v <= (long long)BFB_VOCAB_MAX) sizes.insert((uint32_t)v);
    }
  for (uint32_t V : sizes)
    for (bool on : {false, true})
      for (uint32_t n : {0u, 1u, 2u, ADDED_MAX_TOKENS}) {
        const uint32_t A = added_first(V), bound = added_bound(V, on, n);
        CHECK(A == V + 256 && A <= 0x7fffffffu && added_fits(V, n));
        CHECK(bound == (n ? A + n : on ? V + 256 : V) && bound <= 0x7fffffffu && bound >= V);
        const long long probe[] = {-1, 0, (long long)V - 1, V, (long long)V + 255, A, (long long)A + 1, (long long)A + n - 1, (long long)A + n, (long long)A + n + 1,
                                   0x7fffffffll, -0x80000000ll};
        for (long long id : probe) {
          CHECK(added_is_added_id(id, V, n) == (id >= (long long)A && id < (long long)A + n));
          const bool want = id >= 0 && (id < (long long)V || (id < (long long)A ? on : id < (long long)A + n));
          CHECK(added_id_valid(id, V, on, n) == want);
          if (added_id_valid(id, V, on, n) && (n || id < (long long)bound)) CHECK(id < (long long)bound || (!n && on));
        }
        CHECK(added_table_offsets(V, n) == (size_t)V + 256 + n + 1);
        CHECK((bytefb_bitmap_words(bound) - 1) * 32 >= (size_t)bound);
        if (V <= (1u << 18)) {  // the table's offsets, filled as host_decode.cpp fills them
          std::vector<uint32_t> off(added_table_offsets(V, n), 0);
          uint32_t blob = 0;
          for (uint32_t id = 0; id < V; id++) {
            off[id] = blob;
            blob += id % 5;
          }
          for (uint32_t b = 0; b <= BYTE_IDS; b++) off[(size_t)V + b] = blob + b;
          blob += BYTE_IDS;
          for (uint32_t k = 0; k < n; k++) {
            blob += 1 + k % ADDED_MAX_BYTES;
            off[(size_t)V + BYTE_IDS + k + 1] = blob;
          }
          for (size_t id = 0; id + 1 < off.size(); id++) CHECK(off[id + 1] >= off[id]);
          if (n) CHECK(off[(size_t)bound] == blob);
        }
      }
  CHECK(!added_fits(BFB_VOCAB_MAX + 1, 1) && !added_fits(600, ADDED_MAX_TOKENS + 1));
  CHECK(added_n_sub(0, 0) == 0 && added_n_sub(7, 3) == 13);

  // ---- the validation
  CHECK(Packed({"<sep>", "<2en>", "a", "ab", "abc", "\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80", std::string(255, 'x')}).validate().empty());
  CHECK(!Packed({}).validate().empty());
  CHECK(!Packed({"a", ""}).validate().empty());
  CHECK(!Packed({std::string(256, 'x')}).validate().empty());
  for (const char *bad : {"a b", "a\nb", "a\tb", "\r", "a\xe2\x96\x81", "\x0b", "\x0c", "\xff", "\xc3", "a\xc3", "\xe2\x82", "\xc0\xaf", "\xed\xa0\x80", "\xf4\x90\x80\x80", "\x80"})
    CHECK(!Packed({"ok", bad}).validate().empty());
  CHECK(!Packed({"a", "b", "a"}).validate().empty());
  CHECK(!Packed({"a"}).validate(BFB_VOCAB_MAX + 1).empty());
  {
    std::vector<std::string> many;
    for (uint32_t k = 0; k < ADDED_MAX_TOKENS + 1; k++) many.push_back("<t" + std::to_string(k) + ">");
    CHECK(!Packed(many).validate().empty());
    many.pop_back();
    CHECK(Packed(many).validate().empty());
  }
  {
    Packed p({"ab", "cd"});  // offsets that run backwards
    std::swap(p.off[1], p.off[2]);
    CHECK(!p.validate().empty());
  }

  // ---- the matcher's tables
  std::vector<std::vector<std::string>> sets = {{"a"}, {"ab", "abc", "bc", "abcd"}, {"aa"}, {"<sep>", "<2en>", "<", ">", "\xc3\xa9", "\xc3"}};
  {
    std::vector<std::string> many;
    for (uint32_t k = 0; k < ADDED_MAX_TOKENS; k++) many.push_back("<ex" + std::to_string(k) + ">");
    sets.push_back(many);
    std::vector<std::string> lens;
    for (uint32_t l = 1; l <= ADDED_MAX_BYTES; l++) lens.push_back(std::string(l, 'q'));
    sets.push_back(lens);
  }
  for (const std::vector<std::string> &toks : sets) {
    const Packed p(toks);
    CHECK(p.validate().empty() || toks[5] == "\xc3");  // (the fourth set holds a lone lead byte on purpose: the tables are bytes, not characters)
    const uint32_t n = (uint32_t)toks.size();
    const AddedTables t = added_tables(p.blob.data(), p.off.data(), n);
    CHECK(t.one.size() == 256 && t.dir_off.size() == ADDED_DIR + 1 && t.tok_off.size() == n + 1 && t.dir_off[ADDED_DIR] == t.list.size());
    std::set<uint8_t> firsts;
    size_t longer = 0;
    for (uint32_t k = 0; k < n; k++) {
      firsts.insert((uint8_t)toks[k][0]);
      CHECK(t.tok_off[k + 1] - t.tok_off[k] == toks[k].size());
      if (toks[k].size() == 1) {
        CHECK(t.one[(uint8_t)toks[k][0]] == k);
        continue;
      }
      longer++;
      const uint32_t b = added_bucket((uint8_t)toks[k][0], (uint8_t)toks[k][1]);
      CHECK(b < ADDED_DIR);
      bool found = false;
      for (uint32_t q = t.dir_off[b]; q < t.dir_off[b + 1]; q++)
        found = found || (added_entry_tok(t.list[q]) == k && added_entry_len(t.list[q]) == toks[k].size() && added_entry_off(t.list[q]) == t.tok_off[k]);
      CHECK(found);
    }
    CHECK(t.list.size() == longer);
    for (uint32_t b = 0; b < ADDED_DIR; b++)
      for (uint32_t q = t.dir_off[b]; q + 1 < t.dir_off[b + 1]; q++) CHECK(added_entry_len(t.list[q]) >= added_entry_len(t.list[q + 1]));
    for (uint32_t c = 0; c < 256; c++) CHECK((((t.first[c >> 5] >> (c & 31u)) & 1u) != 0) == (firsts.count((uint8_t)c) != 0));
    for (const std::string &text : {std::string("abcdabcbc"), std::string("aaaaa"), std::string("x<sep><2en>\xc3\xa9\xc3<"), std::string("<ex7><ex4095><ex40955"),
                                    std::string(600, 'q') + "a", std::string("")})
      CHECK(rule_matches(text, toks) == table_matches(text, toks, t));
  }
  printf("added_plan: %llu checks passed (%zu vocabulary sizes)\n", checked, sizes.size());
  return 0;
}
