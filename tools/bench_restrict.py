#!/usr/bin/env python3
"""tools/bench_restrict.py -- the vocabulary restriction made on the device (k_restrict.h), on the MI355X.

The ids are those of bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) under the committed golden model
tests/golden/train_readme_small.model, as in the sibling tools.  One process, the calls alternating within every repeat:
  (a) kernel time of the pass (yttm_restrict_ids_device's kernel_ms: measure + scan + write) under three masks: every id allowed (through this
      entry the write pass runs and copies; behind an encode it is skipped), no id allowed, and a mask chosen from the batch's counts that splits
      about a tenth of the id occurrences.  GB/s by the algorithmic bytes, 4 K_in + 8 (S + 1) read and 4 K_out + 8 (S + 1) written, as a share of
      the copy ceiling.
  (b) the same expansion with torch ops on the same tensors (a gather of the lengths, cumsum, repeat_interleave, a gather of the ids), the
      route a user has without the pass, timed with CUDA events.
  (c) yttm_encode_device's kernel time with no vocabulary set, with every id allowed (the measure pass alone on top) and with none allowed.
Medians and spreads go to profiles/restrict.json (and stdout).  --once runs the pass once under the none-allowed mask (the command to profile)."""
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
    return {"median_" + unit: round(m, 6), "min_" + unit: round(min(v), 6), "max_" + unit: round(max(v), 6), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--share", type=float, default=0.10, help="share of the id occurrences the third mask splits")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restrict.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    from restrict_checks import Rules
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    V = core.vocab_size()
    R = Rules(model, V)
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_toff = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    del host
    torch.cuda.synchronize()

    def encode_ms():
        return core.encode_device_raw(d_text.data_ptr(), d_toff.data_ptr(), n, N, ENCODE_LINE + 1)

    K, _ = encode_ms()
    ids = torch.empty(K, dtype=torch.int32, device="cuda")
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    core.copy_encode_device(ids.data_ptr(), off.data_ptr(), n)
    torch.cuda.synchronize()
    counts = torch.bincount(ids, minlength=V).cpu().numpy()
    # the third mask: merged ids from the rarest up until about `share` of the occurrences split
    merged = sorted((z for z in R.by_z if counts[z]), key=lambda z: counts[z])
    tenth, acc = np.ones(V, bool), 0
    for z in merged:
        if acc + counts[z] > args.share * K and acc:
            break
        tenth[z] = False
        acc += int(counts[z])
    masks = (("all_allowed", np.ones(V, bool)), ("none_allowed", np.zeros(V, bool)), ("tenth_splits", tenth))

    def run_pass():
        return core.restrict_ids_device_raw(ids.data_ptr(), off.data_ptr(), n, K)

    if args.once:
        core.set_vocabulary(masks[1][1])
        k_out, ms = run_pass()
        print(json.dumps({"once": True, "ids_in": int(K), "ids_out": int(k_out)}))
        return

    def torch_expand(L, src, flat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lens = L[ids]
        start = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=start[1:])
        total = int(start[-1])
        delta = src[ids] - start[:-1]
        out = flat[torch.repeat_interleave(delta, lens, output_size=total) + torch.arange(total, device="cuda")]
        out_off = start[off]
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out, out_off

    res = {"metric": "restrict", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "ids_in": int(K), "vocab": V, "copy_ceiling_gbs": COPY_CEILING_GBS,
           "algorithmic_bytes_note": "4 K_in + 8 (S + 1) read, 4 K_out + 8 (S + 1) written", "kernel": {}, "torch_ops": {}, "encode_device_kernel_ms": {}}
    tables, k_outs, split_share = {}, {}, {}
    for name, allowed in masks:  # the pass against the torch expansion first: both from the oracle's table
        E = R.table(allowed)
        L = torch.tensor([len(E[v]) for v in range(V)], dtype=torch.int64, device="cuda")
        src = torch.zeros(V + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(L, 0, out=src[1:])
        flat = torch.tensor([u for v in range(V) for u in E[v]], dtype=torch.int32, device="cuda")
        tables[name] = (L, src, flat)
        split_share[name] = round(sum(int(counts[v]) for v in range(V) if len(E[v]) > 1) / K, 4)  # of the id occurrences
        core.set_vocabulary(allowed)
        k_out, _ = run_pass()
        got, got_off = torch.empty(k_out, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        core.copy_encode_device(got.data_ptr(), got_off.data_ptr(), n)
        _, want, want_off = torch_expand(L, src, flat)
        assert torch.equal(got, want) and torch.equal(got_off, want_off), name
        k_outs[name] = int(k_out)
        del got, got_off, want, want_off
    t_k = {name: [] for name, _ in masks}
    t_t = {name: [] for name, _ in masks}
    t_e = {"no_vocabulary": [], "all_allowed": [], "none_allowed": []}
    for _ in range(args.repeats):
        for name, allowed in masks:
            core.set_vocabulary(allowed)
            t_k[name].append(run_pass()[1])
            ms, out, out_off = torch_expand(*tables[name])
            t_t[name].append(ms)
            del out, out_off
            if name != "tenth_splits":
                t_e[name].append(encode_ms()[1])
        core.set_vocabulary(None)
        t_e["no_vocabulary"].append(encode_ms()[1])
    for name, _ in masks:
        ms = statistics.median(t_k[name])
        alg = 4 * K + 4 * k_outs[name] + 16 * (n + 1)
        res["kernel"][name] = dict(stat(t_k[name]), ids_out=k_outs[name], split_share=split_share[name], gbs=round(alg / (ms / 1e3) / 1e9, 1),
                                   share_of_copy_ceiling=round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4))
        res["torch_ops"][name] = dict(stat(t_t[name]), ratio_to_kernel=round(statistics.median(t_t[name]) / ms, 2))
    for name, v in t_e.items():
        res["encode_device_kernel_ms"][name] = stat(v)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
