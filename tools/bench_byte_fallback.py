#!/usr/bin/env python3
"""tools/bench_byte_fallback.py -- the byte fallback pass (k_bytefb.h) on the MI355X.

The input is bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) in HBM, plain and with --unk-share of its
letters replaced by a char outside the alphabet (default 1 %, tools/bench_encode_subword.py's variant); the model is the committed golden model
tests/golden/train_readme_small.model.  One process, two encoders (setting off / on), the routes alternating within every repeat:
  (a) yttm_encode_device's kernel_ms on the plain batch, setting off and on: the difference is the measure pass (nothing to replace, the write
      pass is skipped -- the encoder's counters prove it)
  (b) the same on the 1 % batch: the difference is measure + scan + write
  (c) yttm_byte_fallback_ids_device on the setting-off ids of the 1 % batch: the pass alone, its own kernel_ms; GB/s by its algorithmic bytes
      4 K_in + 8 (S + 1) + the text of the sentences that hold an unk_id read, 4 K_out + 8 (S + 1) written, as a share of the copy ceiling
Medians and spreads go to profiles/byte_fallback.json (and stdout).  --once runs (c) once (the command to profile: rocprofv3 --kernel-trace
--stats --output-format csv -d DIR -- python tools/bench_byte_fallback.py --once, then tools/pmc_summary.py kernel-stats DIR
profiles/byte_fallback_kernel_stats.csv)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_CEILING_GBS = 6290.0  # the measured copy ceiling of the MI355X (README.md)


def stat(v, unit="ms"):
    m = statistics.median(v)
    return {"median_" + unit: round(m, 4), "min_" + unit: round(min(v), 4), "max_" + unit: round(max(v), 4), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--unk-share", type=float, default=0.01)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "byte_fallback.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    off_core, on_core = yttm.BPE(model).bpe_cython, yttm.BPE(model).bpe_cython
    on_core.set_byte_fallback(True)
    V = on_core.vocab_size()
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    arr = np.frombuffer(host, np.uint8).copy()
    hit = (np.random.default_rng(5).random(len(arr)) < args.unk_share) & (arr != 10) & (arr != 32)
    arr[hit] = ord("Z")
    d_unk = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    del arr, host

    def encode(core, text):
        n_ids, ms = core.encode_device_raw(text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return ms, n_ids

    # the setting-off ids of the 1 % batch, as tensors of their own: the stand-alone pass's input
    _, k_in = encode(off_core, d_unk)
    u_ids, u_off = torch.empty(k_in, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    off_core.copy_encode_device(u_ids.data_ptr(), u_off.data_ptr(), n)

    def alone():
        return on_core.byte_fallback_ids_device_raw(u_ids.data_ptr(), u_off.data_ptr(), d_unk.data_ptr(), d_off.data_ptr(), n, k_in, N)

    if args.once:
        alone()
        print(json.dumps({"once": True, "lines": n, "bytes": N}))
        return
    encode(off_core, d_text), encode(on_core, d_text), encode(on_core, d_unk), alone()  # warm-up: the lanes' buffers
    a_off, a_on, b_off, b_on, c_ms = [], [], [], [], []
    s0 = on_core.byte_fallback_stats()
    for _ in range(args.repeats):
        ms, ids_plain = encode(off_core, d_text)
        a_off.append(ms)
        ms, ids = encode(on_core, d_text)
        a_on.append(ms)
        assert ids == ids_plain
        ms, ids = encode(off_core, d_unk)
        b_off.append(ms)
        assert ids == k_in
        ms, k_out = encode(on_core, d_unk)
        b_on.append(ms)
        k_alone, ms = alone()
        c_ms.append(ms)
        assert k_alone == k_out
    s1 = on_core.byte_fallback_stats()
    assert s1[0] - s0[0] == 3 * args.repeats and s1[1] - s0[1] == args.repeats, "the plain batch skips the write pass, the others run it"
    with_unk = (d_unk.view(n, ENCODE_LINE + 1) == ord("Z")).any(dim=1)
    n_with = int(with_unk.sum())
    text_read = n_with * (ENCODE_LINE + 1)
    read, written = 4 * k_in + 8 * (n + 1) + text_read, 4 * k_out + 8 * (n + 1)
    ms = statistics.median(c_ms)
    gbs = (read + written) / (ms / 1e3) / 1e9
    res = {
        "source_sha16": source_sha16(), "sentences": n, "bytes": N, "vocab": V, "unk_share": args.unk_share,
        "plain": {"encode_off": stat(a_off), "encode_on": stat(a_on), "measure_pass_ms": round(statistics.median(a_on) - statistics.median(a_off), 4),
                  "ids": ids_plain},
        "unk": {"encode_off": stat(b_off), "encode_on": stat(b_on), "pass_in_encode_ms": round(statistics.median(b_on) - statistics.median(b_off), 4),
                "ids_in": k_in, "ids_out": k_out, "sentences_with_unk": n_with},
        "pass_alone": {"kernel": stat(c_ms), "bytes_read": read, "bytes_written": written, "gbs": round(gbs, 1),
                       "share_of_copy_ceiling": round(gbs / COPY_CEILING_GBS, 4)},
    }
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
