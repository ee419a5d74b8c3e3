"""No block of the device-memory pool is lost when an allocation fails (the product sources on the HIP emulator, GPU-less machines).

Every allocation of the trainer's context can throw (the pool ends in hipMalloc), the C ABI catches the error and the process goes on: what the
throwing function held must be back in the pool then.  YTTM_TEST_ALLOC_FAIL=N makes the N-th allocation after a context is made fail;
yttm_gpu_pool_stats reports the pool's bytes in use.  tests/alloc_failure_worker.py, a child process under a time limit (a hang fails instead
of stalling the suite), trains tests/golden/train_mix_cov.txt once cleanly -- that gives K, the allocations of a training -- and then once
for every N in 1 .. K (beyond 400: 1 .. 100, K and every ceil(K / 300)-th in between).  Each failing training must return a status whose message
says `injected` and leave the bytes in use where they were before the call, and the clean training after it must write the golden model byte
for byte.

The hooks are the ones tests/test_round_state.py reaches word mode with on toy corpora; the clean run proves through its report that the paths
were reached (a hot-list rebuild, word mode and an index build -- one pass with the index filled by radix partition, one with the streaming
fill -- and, on this corpus, a tile repack).  tests/golden/train_stress_manual.txt is not trained: it is ten bytes, and a class-C tile takes a
word of more than 2048 tokens."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = {"YTTM_WORD_MIN_TILES": "0", "YTTM_WORD_MIN_TOKENS": "0", "YTTM_HOT_TARGET": "40"}
PASSES = {"index_radix": "0", "index_stream": str(1 << 62)}  # YTTM_INDEX_RADIX_MIN


@pytest.mark.parametrize("index_pass", sorted(PASSES))
def test_no_block_is_lost_on_any_failing_allocation(index_pass, sim_lib, tmp_path):
    env = dict(os.environ, YTTM_AMD_LIB=sim_lib)
    hooks = dict(HOOKS, YTTM_INDEX_RADIX_MIN=PASSES[index_pass])
    r = subprocess.run([sys.executable, os.path.join(HERE, "alloc_failure_worker.py"), str(tmp_path), "mix_cov"] + [f"{k}={v}" for k, v in hooks.items()],
                       capture_output=True, text=True, env=env, timeout=600)
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert r.returncode == 0 and rows and rows[-1]["kind"] == "done", (r.stdout[-2000:], r.stderr[-2000:])
    clean, fails, done = rows[0], [x for x in rows if x["kind"] == "fail"], rows[-1]
    # the clean run: the golden model, nothing left in use, and the paths this test is there for
    assert clean["rc"] == 0 and clean["golden"] and clean["stats"]["in_use"] == 0, clean
    rep = clean["report"]
    assert rep["index_builds"] >= 1 and rep["hot_rebuilds"] >= 1 and rep["word_rounds"] > 0, rep
    assert (rep["index_radix_builds"] >= 1) == (index_pass == "index_radix"), rep
    k = clean["K"]
    print(f"{index_pass}: K = {k} allocations in a clean training, {done['tried']} values of N tried")
    assert k > 0 and done["tried"] == len(fails) and (len(fails) == k if k <= 400 else len(fails) >= 100)
    assert {x["N"] for x in fails} >= set(range(1, min(k, 100) + 1)) | {k}
    bad = [x for x in fails if not (x["rc"] != 0 and "injected" in x["err"] and x["allocs"] == x["N"] and x["in_use_after"] == x["in_use_before"] and
                                    x["clean_rc"] == 0 and x["golden"] and x["in_use_end"] == x["in_use_before"])]
    assert not bad, (len(bad), bad[:5])
