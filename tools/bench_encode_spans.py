#!/usr/bin/env python3
"""tools/bench_encode_spans.py -- the byte spans made on the device (k_spans.h), on the MI355X.

The input is bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) in HBM; the model is the committed golden
model tests/golden/train_readme_small.model, as in tools/bench_encode_subword.py.  One process, the calls alternating within every repeat:
  (a) yttm_spans_device on the resident batch: its kernel_ms, and yttm_encode_device's kernel_ms for the same batch -- the difference is the
      spans pass; GB/s of the pass by its algorithmic bytes N + 4 K + 16 (S + 1) read, 8 K written, as a share of the copy ceiling
  (b) the same with --unk-share of the chars replaced by a char outside the alphabet (default 1 %)
Medians and spreads go to profiles/encode_spans.json (and stdout).  --once runs (a) once (the command to profile)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_CEILING_GBS = 6290.0  # the measured copy ceiling of the MI355X (README.md)


def stat(v, unit="s"):
    m = statistics.median(v)
    return {"median_" + unit: round(m, 6), "min_" + unit: round(min(v), 6), "max_" + unit: round(max(v), 6), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--unk-share", type=float, default=0.01)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_spans.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    core = yttm.BPE(model).bpe_cython
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    torch.cuda.synchronize()

    def spans(text):
        t0 = time.perf_counter()
        n_ids, ms = core.spans_device_raw(text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return time.perf_counter() - t0, ms, n_ids

    def encode(text):
        n_ids, ms = core.encode_device_raw(text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return ms, n_ids

    if args.once:
        spans(d_text)
        print(json.dumps({"once": True, "lines": n, "bytes": N}))
        return
    # (b): the same batch with a share of its letters replaced by a one-byte char outside the alphabet (the sentences keep their offsets)
    arr = np.frombuffer(host, np.uint8).copy()
    hit = (np.random.default_rng(5).random(len(arr)) < args.unk_share) & (arr != 10) & (arr != 32)
    arr[hit] = ord("Z")
    d_unk = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    del arr, host
    spans(d_text), encode(d_text), spans(d_unk), encode(d_unk)  # warm-up: the lanes' buffers
    a_w, a_k, a_e, b_k, b_e = [], [], [], [], []
    for _ in range(args.repeats):
        w, k, ids_a = spans(d_text)
        a_w.append(w), a_k.append(k)
        ms, ids = encode(d_text)
        a_e.append(ms)
        assert ids == ids_a
        w, k, ids_b = spans(d_unk)
        b_k.append(k)
        ms, ids = encode(d_unk)
        b_e.append(ms)
        assert ids == ids_b

    def gbs(k_ms, e_ms, ids):
        ms = statistics.median(k_ms) - statistics.median(e_ms)
        alg = N + 4 * ids + 16 * (n + 1) + 8 * ids
        return {"spans_ms": round(ms, 4), "algorithmic_bytes": alg, "gbs": round(alg / (ms / 1e3) / 1e9, 1),
                "share_of_copy_ceiling": round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4)}

    res = {"metric": "encode_spans", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "bytes": N, "ids": int(ids_a), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "algorithmic_bytes_note": "N + 4 K + 16 (S + 1) read, 8 K written (N text bytes, K ids, S sentences)",
           "a_spans_device_kernel": stat(a_k, "ms"), "a_encode_device_kernel": stat(a_e, "ms"), "a_spans_device_wall": stat(a_w), "a_spans": gbs(a_k, a_e, ids_a),
           "b_unk_share": args.unk_share, "b_ids": int(ids_b), "b_spans_device_kernel": stat(b_k, "ms"), "b_encode_device_kernel": stat(b_e, "ms"),
           "b_spans": gbs(b_k, b_e, ids_b)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
