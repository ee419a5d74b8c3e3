#!/usr/bin/env python3
"""tools/bench_id_counts.py -- token frequencies made on the device (k_idcount.h), on the MI355X.

The ids are those of bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) under the committed golden model
tests/golden/train_readme_small.model, as in tools/bench_encode_spans.py.  One process, the calls alternating within every repeat:
  (a) kernel time of k_idcount (yttm_id_counts_ids_device's kernel_ms: the zeroing of the counts + the kernel) on four inputs of the same
      length: the batch's ids at the vocabulary's size; uniform, Zipf (exponent 1) and all-equal ids at 32 000 bins; each at every window in
      --windows (YTTM_IDCOUNT_WINDOW, one encoder per window).  GB/s by the algorithmic bytes 4 K + 8 (n_bins + 1), as a share of the copy ceiling.
  (b) torch.bincount(ids, minlength=n_bins) on the same device tensors, timed with CUDA events, alternating with (a) at the default window.
  (c) the file route: yttm_encode_file_counts on the batch as a file in the page cache against encode_file to host arrays + numpy.bincount.
Medians and spreads go to profiles/id_counts.json (and stdout).  --once runs (a) once on the batch's ids (the command to profile)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_CEILING_GBS = 6290.0  # the measured copy ceiling of the MI355X (README.md)
HOOK = "YTTM_IDCOUNT_WINDOW"


def stat(v, unit="s"):
    m = statistics.median(v)
    return {"median_" + unit: round(m, 6), "min_" + unit: round(min(v), 6), "max_" + unit: round(max(v), 6), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--file-repeats", type=int, default=5)
    ap.add_argument("--windows", default="0,4096,16384,32768", help="values of " + HOOK + " for (a); the last one is the default build")
    ap.add_argument("--bins", type=int, default=32_000, help="bins of the synthetic inputs")
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--dir", default=None, help="where the input file of (c) goes (default: a temporary directory)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "id_counts.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    windows = [int(w) for w in args.windows.split(",")]
    cores = {}
    for w in windows:  # (an encoder reads the hooks when it is made)
        os.environ[HOOK] = str(w)
        cores[w] = yttm.BPE(model).bpe_cython
    os.environ.pop(HOOK, None)
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    V = core.vocab_size()
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    torch.cuda.synchronize()
    K, _ = core.encode_device_raw(d_text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
    ids = torch.empty(K, dtype=torch.int32, device="cuda")
    core.copy_encode_device(ids.data_ptr(), None, n)
    del d_text, d_off
    torch.cuda.synchronize()

    def count(c, t, n_bins):
        return c.id_counts_ids_device_raw(t.data_ptr(), t.numel(), n_bins)

    if args.once:
        count(core, ids, V)
        print(json.dumps({"once": True, "ids": K, "n_bins": V}))
        return
    g = torch.Generator(device="cuda").manual_seed(7)
    uniform = torch.randint(0, args.bins, (K,), generator=g, device="cuda", dtype=torch.int32)
    # Zipf, exponent 1, by the inverse of its (continuous) distribution function: k = floor(bins ** u) - 1 has P(k) ~ log((k + 2) / (k + 1)) ~ 1 / (k + 1)
    u = torch.rand(K, generator=g, device="cuda", dtype=torch.float64)
    zipf = (torch.pow(float(args.bins), u).floor().to(torch.int64) - 1).clamp_(0, args.bins - 1).to(torch.int32)
    del u
    equal = torch.full((K,), 7, dtype=torch.int32, device="cuda")
    inputs = (("batch", ids, V), ("uniform", uniform, args.bins), ("zipf", zipf, args.bins), ("all_equal", equal, args.bins))
    torch.cuda.synchronize()

    def bincount(t, n_bins):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = torch.bincount(t, minlength=n_bins)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    res = {"metric": "id_counts", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "ids": int(K), "vocab": V, "synthetic_bins": args.bins, "copy_ceiling_gbs": COPY_CEILING_GBS,
           "algorithmic_bytes_note": "4 K + 8 (n_bins + 1): every id read once, the counts written once", "default_window": windows[-1], "kernel": {}, "torch_bincount": {}}
    for name, t, n_bins in inputs:  # the kernel against numpy-free ground truth first: torch.bincount of the same tensor
        want = torch.bincount(t, minlength=n_bins)
        for w in windows:
            count(cores[w], t, n_bins)
            got = torch.empty(n_bins + 1, dtype=torch.int64, device="cuda")
            cores[w].copy_id_counts_device(got.data_ptr(), n_bins)
            assert torch.equal(got[:n_bins], want) and int(got[n_bins]) == 0, (name, w)
    times = {(name, w): [] for name, _, _ in inputs for w in windows}
    tb = {name: [] for name, _, _ in inputs}
    for _ in range(args.repeats):
        for name, t, n_bins in inputs:
            for w in windows:
                times[(name, w)].append(count(cores[w], t, n_bins))
            tb[name].append(bincount(t, n_bins)[0])
    for name, t, n_bins in inputs:
        alg = 4 * K + 8 * (n_bins + 1)
        res["kernel"][name] = {}
        for w in windows:
            ms = statistics.median(times[(name, w)])
            res["kernel"][name]["window_%d" % w] = dict(stat(times[(name, w)], "ms"), n_bins=n_bins, gbs=round(alg / (ms / 1e3) / 1e9, 1),
                                                         share_of_copy_ceiling=round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4))
        res["torch_bincount"][name] = dict(stat(tb[name], "ms"), n_bins=n_bins,
                                           ratio_to_kernel=round(statistics.median(tb[name]) / statistics.median(times[(name, windows[-1])]), 3))
    d = windows[-1]
    res["all_equal_to_uniform"] = round(res["kernel"]["all_equal"]["window_%d" % d]["median_ms"] / res["kernel"]["uniform"]["window_%d" % d]["median_ms"], 3)
    del uniform, zipf, equal, ids
    torch.cuda.empty_cache()
    if not args.no_file:
        tmp = tempfile.TemporaryDirectory(dir=args.dir)
        path = os.path.join(tmp.name, "input.txt")
        with open(path, "wb") as f:
            f.write(host)
        with open(path, "rb") as f:  # (in the page cache)
            while f.read(1 << 26):
                pass
        core.encode_file_counts(path)  # warm-up: pinned chunks, both lanes at full size
        f_new, f_old, rep = [], [], None
        for _ in range(args.file_repeats):
            t0 = time.perf_counter()
            got, rep = core.encode_file_counts(path, report=True)
            f_new.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            h_ids, h_off = core.encode_file(path, None)
            want = np.bincount(h_ids, minlength=V)
            f_old.append(time.perf_counter() - t0)
            assert got[:V].tolist() == want.tolist() and got[V] == 0 and rep["ids"] == len(h_ids)
            del h_ids, h_off
        res["file"] = {"bytes": N, "encode_file_counts": stat(f_new), "encode_file_plus_numpy_bincount": stat(f_old),
                       "ratio": round(statistics.median(f_old) / statistics.median(f_new), 3), "last_report": rep}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
