// tools/dbg/check_bytefb_plan.cpp -- walks the id arithmetic of the byte fallback (youtokentome_amd/csrc/bytefb_plan.h) over its whole input
// range on the host, under the sanitizers (needs no GPU):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iyoutokentome_amd/csrc tools/dbg/check_bytefb_plan.cpp -o /tmp/check_bytefb_plan
//   /tmp/check_bytefb_plan
// For every vocabulary size of a grid that holds every power of two and its neighbours up to the encoder's limit, with the setting on and off:
// the bound is V or V + 256 and stays an int32; exactly the ids V .. V + 255 are byte ids, and only with the setting on; the tables' offsets
// hold an entry per id of [0, V + 256) and the end, filled as host_decode.cpp fills them (into real vectors: an index past the end is the
// sanitizer's); the ignore bitmap holds a bit for every id below the bound and its extra word; the names <0xNN> and their parser are inverse.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "bytefb_plan.h"

using namespace yttm;

static unsigned long long checked = 0;
#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      fprintf(stderr, "FAILED %s at V %u on %d (line %d)\n", #c, V, (int)on, __LINE__); \
      exit(1);                                                                           \
    }                                                                                    \
    checked++;                                                                           \
  } while (0)

int main() {
  std::set<uint32_t> sizes{0u, 9u, 600u, 32000u, BFB_VOCAB_MAX};
  for (int b = 0; b < 30; b++)
    for (long long d = -2; d <= 2; d++) {
      const long long v = (1ll << b) + d;
      if (v >= 0 && v <= (long long)BFB_VOCAB_MAX) sizes.insert((uint32_t)v);
    }
  for (uint32_t V : sizes)
    for (bool on : {false, true}) {
      const uint32_t bound = bytefb_bound(V, on);
      CHECK(bound == V + (on ? 256u : 0u) && bound >= V && bound <= 0x7fffffffu);
      CHECK(bytefb_default_bins(V, on) == bound);
      const long long probe[] = {-1, 0, (long long)V - 1, V, (long long)V + 1, (long long)V + 255, (long long)V + 256, (long long)V + 257, 0x7fffffffll, -0x80000000ll};
      for (long long id : probe) CHECK(bytefb_is_byte_id(id, V, on) == (on && id >= (long long)V && id <= (long long)V + 255));
      for (long long id : probe)
        if (bytefb_is_byte_id(id, V, on)) CHECK(id >= 0 && id < (long long)bound && id - V < 256);
      CHECK(bytefb_table_offsets(V) == (size_t)V + 257);
      CHECK((bytefb_bitmap_words(bound) - 1) * 32 >= (size_t)bound && (bytefb_bitmap_words(bound) - 1) * 32 < (size_t)bound + 32);
      if (V <= (1u << 20)) {  // the tables themselves, filled as the host fills them
        std::vector<uint32_t> off(bytefb_table_offsets(V), 0);
        uint32_t blob = 0;
        for (uint32_t id = 0; id < V; id++) {
          off[id] = blob;
          blob += id % 7;
        }
        for (uint32_t b = 0; b <= BYTE_IDS; b++) off[(size_t)V + b] = blob + b;
        for (uint32_t id = 0; id + 1 < off.size(); id++) CHECK(off[id + 1] >= off[id]);
        for (uint32_t b = 0; b < BYTE_IDS; b++) CHECK(off[(size_t)V + b + 1] - off[(size_t)V + b] == 1);
        std::vector<uint32_t> bits(bytefb_bitmap_words(bound), 0);
        for (uint32_t id = 0; id < bound; id += (bound > 4096 ? bound / 1024 : 1)) bits[id >> 5] |= 1u << (id & 31u);
        if (bound) {
          bits[(bound - 1) >> 5] |= 1u << ((bound - 1) & 31u);
          CHECK(((bound - 1) >> 5) + 1 < bits.size());  // (the last id's word, and the extra one behind it)
        }
      }
    }
  const uint32_t V = 0;
  const bool on = true;
  for (uint32_t b = 0; b < 256; b++) {
    const std::string name = bytefb_name(b);
    CHECK(name.size() == 6 && bytefb_parse_name(name) == (int)b);
  }
  for (const char *bad : {"", "<0x>", "<0x1>", "<0xab>", "<0xAB", "0xAB>", "<0xAG>", "<0XAB>", "<0xABC>", "<UNK>", "<0x 1>"}) CHECK(bytefb_parse_name(bad) == -1);
  printf("bytefb_plan: %llu checks passed (%zu vocabulary sizes)\n", checked, sizes.size());
  return 0;
}
