"""Child process of tests/test_sim_alloc_failure.py: trainings of one golden corpus in which the N-th allocation from the device-memory pool
fails (YTTM_TEST_ALLOC_FAIL=N), for every N the test asks for, through the C ABI of the library YTTM_AMD_LIB names.

  python alloc_failure_worker.py OUT_DIR NAME KEY=VALUE ...     (the hooks of the pass; prints one JSON object per line)

First a clean training: the golden model, its report, and K, the allocations it made.  Then for each N the failing training -- it must return
a status whose message says `injected`, and the pool's bytes in use must be what they were before the call -- and a clean training after it,
which must write the golden model again."""
import ctypes as C
import filecmp
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
G = os.path.join(HERE, "golden")


def chosen(k):
    """Every N in 1 .. K; beyond 400: 1 .. 100, K, and every ceil(K / 300)-th in between."""
    if k <= 400:
        return list(range(1, k + 1))
    return sorted(set(range(1, 101)) | set(range(100, k, math.ceil(k / 300))) | {k})


def main():
    out_dir, name = sys.argv[1], sys.argv[2]
    for kv in sys.argv[3:]:
        key, value = kv.split("=", 1)
        os.environ[key] = value
    from youtokentome_amd import _lib
    L = _lib.load()
    a = json.load(open(os.path.join(G, f"train_{name}.args.json")))
    text = open(os.path.join(G, f"train_{name}.txt"), "rb").read()
    golden, model = os.path.join(G, f"train_{name}.model"), os.path.join(out_dir, f"{name}.model")

    def stats():
        v = (C.c_uint64 * 4)()
        L.yttm_gpu_pool_stats(v)
        return dict(in_use=v[0], cached=v[1], peak=v[2], allocs=v[3])

    def train(fail_at):
        if fail_at:
            os.environ["YTTM_TEST_ALLOC_FAIL"] = str(fail_at)
        else:
            os.environ.pop("YTTM_TEST_ALLOC_FAIL", None)
        if os.path.exists(model):
            os.remove(model)
        err, rep = C.create_string_buffer(2048), C.create_string_buffer(16384)
        rc = L.yttm_train_bpe_from_memory(text, len(text), model.encode(), a["vocab"], a["coverage"], a["pad"], a["unk"], a["bos"], a["eos"], 0,
                                          rep, 16384, err, 2048)
        return rc, err.value.decode(errors="replace"), (json.loads(rep.value.decode()) if rc == 0 else None)

    def same_model():
        return os.path.exists(model) and filecmp.cmp(model, golden, shallow=False)

    rc, msg, report = train(0)
    clean = stats()
    k = clean["allocs"]
    print(json.dumps(dict(kind="clean", rc=rc, err=msg, golden=same_model(), K=k, stats=clean, report=report)), flush=True)
    if rc != 0:
        return 1
    ns = chosen(k)
    for n in ns:
        before = stats()
        rc, msg, _ = train(n)
        after = stats()
        rc2, msg2, _ = train(0)
        print(json.dumps(dict(kind="fail", N=n, rc=rc, err=msg, in_use_before=before["in_use"], in_use_after=after["in_use"], allocs=after["allocs"],
                              clean_rc=rc2, clean_err=msg2, golden=same_model(), in_use_end=stats()["in_use"])), flush=True)
    print(json.dumps(dict(kind="done", K=k, tried=len(ns))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
