// tools/dbg/check_alloc_failure.cpp -- nothing is freed early, or twice, when an allocation of the trainer's context fails: the trainings of
// tests/test_sim_alloc_failure.py (every N of YTTM_TEST_ALLOC_FAIL=N, both index passes) through yttm_train_bpe_from_memory, with the product
// sources on the HIP emulator (tests/hipsim) under AddressSanitizer and UndefinedBehaviorSanitizer.  A program of its own: needs no GPU and
// no Python.  From the repository's root, objects outside the source tree:
//   S='-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -std=c++17 -fPIC'
//   make -C tests/hipsim -j8 asan OUT=/tmp/yttm_check_alloc ASAN_FLAGS="$S -Iinclude -I../../youtokentome_amd/csrc -I../../include -DYTTM_ENCODER_UNITS -Wno-unused-function -Wno-unknown-pragmas -Wno-attributes"
//   g++ $S -pthread -Iinclude tools/dbg/check_alloc_failure.cpp /tmp/yttm_check_alloc/*.o -o /tmp/yttm_check_alloc/check_alloc_failure
//   /tmp/yttm_check_alloc/check_alloc_failure [repository root, default .]
// A block that a failing path returned to the pool while a member or a view still pointed at it shows up in the clean training that follows
// (the pool hands the block to someone else: a wrong model), a block returned twice as a corrupted pool; a read or write of memory the
// emulator has given back to the host's allocator as a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "yttm_gpu.h"
#include "yttm_mi355x.h"

// (the emulator keeps its fibers' stacks, host memory, until the process ends: no leak report for those.  What this program is after --
// device blocks the pool loses -- the pool's own count of bytes in use shows.)
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

static std::string slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path.c_str());
    exit(2);
  }
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

#define CHECK(c, ...)                                             \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAILED %s (line %d): ", #c, __LINE__);    \
      fprintf(stderr, __VA_ARGS__);                               \
      fprintf(stderr, "\n");                                      \
      exit(1);                                                    \
    }                                                             \
  } while (0)

int main(int argc, char **argv) {
  const std::string root = argc > 1 ? argv[1] : ".", g = root + "/tests/golden/train_mix_cov";
  const std::string text = slurp(g + ".txt"), golden = slurp(g + ".model");
  char tmpl[] = "/tmp/check_alloc_failure.XXXXXX";
  const int fd = mkstemp(tmpl);
  CHECK(fd >= 0, "mkstemp");
  const std::string model = tmpl;
  // tests/golden/train_mix_cov.args.json: vocab 90, coverage 0.8, pad 0, unk 1, bos 2, eos 3
  auto train = [&](unsigned long long fail_at, std::string *msg) {
    if (fail_at) setenv("YTTM_TEST_ALLOC_FAIL", std::to_string(fail_at).c_str(), 1);
    else unsetenv("YTTM_TEST_ALLOC_FAIL");
    char err[2048] = "", rep[16384] = "";
    const int rc = yttm_train_bpe_from_memory((const uint8_t *)text.data(), text.size(), model.c_str(), 90, 0.8, 0, 1, 2, 3, 0, rep, sizeof rep, err, sizeof err);
    if (msg) *msg = err;
    return rc;
  };
  auto in_use = [] {
    uint64_t v[4];
    yttm_gpu_pool_stats(v);
    return v[0];
  };
  setenv("YTTM_WORD_MIN_TILES", "0", 1);
  setenv("YTTM_WORD_MIN_TOKENS", "0", 1);
  setenv("YTTM_HOT_TARGET", "40", 1);
  setenv("YTTM_WORD_HINT_FLOOR", "2048", 1);  // (a grid size only: the emulator's time goes with the workgroups it runs)
  unsigned long long tried = 0;
  for (const char *radix_min : {"0", "4611686018427387904"}) {
    setenv("YTTM_INDEX_RADIX_MIN", radix_min, 1);
    std::string msg;
    CHECK(train(0, &msg) == 0, "%s", msg.c_str());
    CHECK(slurp(model) == golden, "the clean training's model");
    uint64_t v[4];
    yttm_gpu_pool_stats(v);
    const unsigned long long k = v[3];
    CHECK(v[0] == 0 && k > 0, "%llu bytes in use after a clean training of %llu allocations", (unsigned long long)v[0], k);
    const unsigned long long step = (k + 299) / 300, before_loop = tried;
    for (unsigned long long n = 1; n <= k; n++) {
      if (!(k <= 400 || n <= 100 || n == k || (n - 100) % step == 0)) continue;  // (the test's choice of N)
      const unsigned long long before = in_use();
      const int rc = train(n, &msg);
      CHECK(rc != 0 && msg.find("injected") != std::string::npos, "N = %llu: status %d, %s", n, rc, msg.c_str());
      CHECK(in_use() == before, "N = %llu: %llu bytes in use, %llu before the call", n, (unsigned long long)in_use(), before);
      CHECK(train(0, &msg) == 0, "N = %llu, the clean training after it: %s", n, msg.c_str());
      CHECK(slurp(model) == golden, "N = %llu: the model of the clean training after it", n);
      tried++;
    }
    printf("YTTM_INDEX_RADIX_MIN=%s: K = %llu allocations, %llu values of N tried\n", radix_min, k, tried - before_loop);
  }
  yttm_release_device_memory();
  remove(model.c_str());
  printf("check_alloc_failure: %llu failing trainings, no block lost, every model golden\n", tried);
  return 0;
}
