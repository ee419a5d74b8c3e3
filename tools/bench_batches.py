#!/usr/bin/env python3
"""tools/bench_batches.py -- batches by length under a token budget made on the device (k_batches.h), on the MI355X.

The ids are those of bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) under the committed golden model
tests/golden/train_readme_small.model, as in tools/bench_blocks.py.  One process, the calls alternating within every repeat:
  (a) kernel time of the plan (yttm_batches_plan_lengths_device's kernel_ms: the key pass, the passes of the sort, the cuts, their
      synchronisations included) and of the gather (yttm_batches_gather_ids_device's: measure, scan, write) at every max_tokens of --tokens with
      max_sentences = 0.  GB/s by the algorithmic bytes -- plan 4 S read, 4 S + 8 (B + 1) written; gather 4 K + 8 (S + 1) + 4 S + 8 (B + 1)
      read, 4 E + 4 B + 8 (B + 1) written -- as a share of the copy ceiling.
  (b) the route a user has today, on the same tensors, as three figures: torch.sort(lengths, stable=True) (CUDA events); the cut loop in Python
      on the downloaded sorted lengths (timed once per budget: it is a sequential recurrence); the matrices by ONE vectorised torch
      formulation -- segment maxima by scatter_reduce, the row starts by cumsum, every id's place by repeat_interleave, one scatter into the
      padded output -- which is faster than a Python loop of one gather per batch; that loop is timed on the first --loop-batches batches and
      scaled to all of them.  The torch arrays are compared with (a)'s.
  (c) --kernel-stats CSV: the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of --once, among them k_bat_chain's -- the serial step
      that remains in the cuts.
Medians and spreads go to profiles/batches.json (and stdout).  --once runs plan + gather once at the first budget (the command to profile)."""
import argparse
import csv
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


def host_cuts(sorted_lens, T):
    """batch_first by the loop a user writes today"""
    first, a, n = [0], 0, len(sorted_lens)
    for b in range(1, n):
        if (b + 1 - a) * sorted_lens[b] > T:
            first.append(b)
            a = b
    first.append(n)
    return first


def torch_matrices(torch, ids, off, order, first, pad):
    """widths, batch_off and the padded output of every batch by array operations on the device"""
    lens = (off[1:] - off[:-1])[order]
    rows = first[1:] - first[:-1]
    b_of = torch.repeat_interleave(torch.arange(rows.numel(), device=ids.device), rows)
    widths = torch.zeros(rows.numel(), dtype=torch.int64, device=ids.device).scatter_reduce(0, b_of, lens, "amax")
    batch_off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(rows * widths, 0, out=batch_off[1:])
    row_start = batch_off[b_of] + (torch.arange(order.numel(), device=ids.device) - first[b_of]) * widths[b_of]
    src_start = off[:-1][order]
    sent_of = torch.repeat_interleave(torch.arange(order.numel(), device=ids.device), lens)
    within = torch.arange(sent_of.numel(), device=ids.device) - (torch.cumsum(lens, 0) - lens)[sent_of]
    out = torch.full((int(batch_off[-1]),), pad, dtype=torch.int32, device=ids.device)
    out[row_start[sent_of] + within] = ids[src_start[sent_of] + within]
    return widths, batch_off, out


def torch_loop(torch, ids, off, order, first, pad, n_batches):
    """one gather per batch, the first n_batches batches"""
    outs = []
    for b in range(n_batches):
        idx = order[first[b]:first[b + 1]]
        a, ln = off[idx], off[idx + 1] - off[idx]
        w = int(ln.max())
        col = torch.arange(w, device=ids.device)
        m = ids[(a[:, None] + col[None, :]).clamp_(max=ids.numel() - 1)]
        outs.append(torch.where(col[None, :] < ln[:, None], m, pad))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tokens", default="4096,16384")
    ap.add_argument("--loop-batches", type=int, default=2000)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="the summary (tools/pmc_summary.py kernel-stats) of a rocprofv3 --kernel-trace --stats run of --once")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batches.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    budgets = [int(v) for v in args.tokens.split(",")]
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    pad = bpe.subword_to_id("<PAD>")
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    torch.cuda.synchronize()
    K, enc_ms = core.encode_device_raw(d_text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
    ids = torch.empty(K, dtype=torch.int32, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    core.copy_encode_device(ids.data_ptr(), off.data_ptr(), n)
    lengths = (off[1:] - off[:-1]).to(torch.int32)
    del d_text, d_off, host
    torch.cuda.synchronize()

    def plan(T):
        return core.batches_plan_lengths_device_raw(lengths.data_ptr(), n, T)

    def gather():
        return core.batches_gather_ids_device_raw(ids.data_ptr(), off.data_ptr(), n, K, pad, False)

    if args.once:
        plan(budgets[0])
        gather()
        print(json.dumps({"once": True, "ids": K, "sentences": n, "max_tokens": budgets[0]}))
        return
    res = {"metric": "batches", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "ids": int(K), "encode_kernel_ms": round(enc_ms, 3), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "algorithmic_bytes_note": "plan: read 4 S, written 4 S + 8 (B + 1); gather: read 4 K + 8 (S + 1) + 4 S + 8 (B + 1), written 4 E + 4 B + 8 (B + 1)",
           "kernel": {}, "torch_route": {}}
    shape, t_plan, t_gather, t_sort, t_mat = {}, {T: [] for T in budgets}, {T: [] for T in budgets}, [], {T: [] for T in budgets}
    dev = {}
    for T in budgets:  # once: the shapes, and (a)'s arrays against (b)'s
        n_kept, nb, _ = plan(T)
        ne, _ = gather()
        shape[T] = (n_kept, nb, ne)
        order = torch.empty(n, dtype=torch.int32, device="cuda")
        first, boff = torch.empty(nb + 1, dtype=torch.int64, device="cuda"), torch.empty(nb + 1, dtype=torch.int64, device="cuda")
        widths, out = torch.empty(nb, dtype=torch.int32, device="cuda"), torch.empty(ne, dtype=torch.int32, device="cuda")
        core.copy_batches_device(order.data_ptr(), first.data_ptr(), widths.data_ptr(), boff.data_ptr(), out.data_ptr(), n, nb, ne)
        s_len, s_idx = torch.sort(lengths, stable=True)
        assert torch.equal(s_idx.to(torch.int32), order), T
        t0 = time.perf_counter()
        h_first = host_cuts(s_len.cpu().tolist(), T)
        dt_cuts = time.perf_counter() - t0
        assert h_first == first.cpu().tolist(), T
        w2, o2, out2 = torch_matrices(torch, ids, off, s_idx, first, pad)
        assert torch.equal(w2.to(torch.int32), widths) and torch.equal(o2, boff) and torch.equal(out2, out), T
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k = min(args.loop_batches, nb)
        torch_loop(torch, ids, off, s_idx, h_first, pad, min(k, 50))  # (warm-up)
        a.record()
        outs = torch_loop(torch, ids, off, s_idx, h_first, pad, k)
        b.record()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([m.reshape(-1) for m in outs]), out[:int(boff[k])]), T
        dev[T] = (s_idx, first)
        res["torch_route"]["T%d" % T] = {"cut_loop_seconds_once": round(dt_cuts, 3), "per_batch_gather_loop": {
            "batches_timed": k, "ms_timed": round(a.elapsed_time(b), 3), "ms_scaled_to_all_batches": round(a.elapsed_time(b) * nb / k, 1)}}
        del order, boff, widths, out, w2, o2, out2, outs, s_len
    for _ in range(args.repeats):
        for T in budgets:
            t_plan[T].append(plan(T)[2])
            t_gather[T].append(gather()[1])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            got = torch_matrices(torch, ids, off, dev[T][0], dev[T][1], pad)
            b.record()
            torch.cuda.synchronize()
            t_mat[T].append(a.elapsed_time(b))
            del got
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = torch.sort(lengths, stable=True)
        b.record()
        torch.cuda.synchronize()
        t_sort.append(a.elapsed_time(b))
        del got
    for T in budgets:
        n_kept, nb, ne = shape[T]
        alg_plan = 4 * n + 4 * n + 8 * (nb + 1)
        alg_gather = 4 * K + 8 * (n + 1) + 4 * n + 8 * (nb + 1) + 4 * ne + 4 * nb + 8 * (nb + 1)
        for name, times, alg in (("plan", t_plan[T], alg_plan), ("gather", t_gather[T], alg_gather)):
            ms = statistics.median(times)
            res["kernel"]["%s_T%d" % (name, T)] = dict(stat(times, "ms"), kept=n_kept, batches=nb, elements=ne, algorithmic_bytes=alg,
                                                       gbs=round(alg / (ms / 1e3) / 1e9, 1), share_of_copy_ceiling=round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4))
        r = res["torch_route"]["T%d" % T]
        r["sort_stable"] = stat(t_sort, "ms")
        r["matrices_vectorised"] = stat(t_mat[T], "ms")
        ours = statistics.median(t_plan[T]) + statistics.median(t_gather[T])
        theirs = statistics.median(t_sort) + r["cut_loop_seconds_once"] * 1e3 + statistics.median(t_mat[T])
        r["plan_plus_gather_ms"] = round(ours, 3)
        r["sort_plus_cut_loop_plus_matrices_ms"] = round(theirs, 1)
        r["ratio_to_kernel"] = round(theirs / ours, 1)
        r["ratio_to_kernel_without_the_cut_loop"] = round((statistics.median(t_sort) + statistics.median(t_mat[T])) / ours, 2)
    if args.kernel_stats:
        rowsk = {}
        for r in csv.DictReader(open(args.kernel_stats)):  # (the summary tools/pmc_summary.py kernel-stats writes)
            if r["kernel"].startswith("k_bat_") or "scan" in r["kernel"]:
                rowsk[r["kernel"]] = {"calls": int(r["calls"]), "avg_us": float(r["avg_us"]), "total_ms": float(r["total_ms"])}
        res["kernel_stats_once"] = rowsk
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
