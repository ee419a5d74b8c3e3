#!/usr/bin/env python3
"""tools/bench_blocks.py -- training blocks made on the device (k_blocks.h), on the MI355X.

The ids are those of bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) under the committed golden model
tests/golden/train_readme_small.model, as in tools/bench_id_counts.py.  One process, the calls alternating within every repeat:
  (a) kernel time of the pass (yttm_blocks_ids_device's kernel_ms: every kernel from the sentence flags to the write pass, the scans and their
      synchronisations included) for stream and whole mode at every seq_len of --lens, tail = pad.  GB/s by the algorithmic bytes
      4 K + 8 (S + 1) read, 12 n_rows L + 8 n_frags + 8 (n_rows + 1) written, as a share of the copy ceiling.
  (b) the same arrays made by torch ops on the same tensors, the route a user has today: stream mode with searchsorted / cumsum / scatter, timed
      with CUDA events and compared with (a)'s arrays; whole mode by the host loop over the sentence lengths (next-fit is a sequential
      recurrence), timed once.
  (c) the file route: yttm_encode_file_blocks on the batch as a file in the page cache against encode_file to host arrays + numpy.
  (d) --kernel-stats CSV: the per-kernel times of a `rocprofv3 --kernel-trace --stats` run of --once (whole mode), among them k_blk_chain's -- the
      orbit chain's time alone.
Medians and spreads go to profiles/blocks.json (and stdout).  --once runs (a) once per mode at the first seq_len (the command to profile)."""
import argparse
import csv
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
STREAM, WHOLE = 0, 1


def stat(v, unit="s"):
    m = statistics.median(v)
    return {"median_" + unit: round(m, 6), "min_" + unit: round(min(v), 6), "max_" + unit: round(max(v), 6), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def torch_stream(torch, ids, off, L, pad):
    """rows, seg, pos of stream mode (tail = pad) with torch ops on the device tensors"""
    K = ids.numel()
    n_rows = (K + L - 1) // L
    rows = torch.full((n_rows * L,), pad, dtype=torch.int32, device=ids.device)
    rows[:K] = ids
    e = torch.arange(n_rows * L, device=ids.device)
    valid = e < K
    starts = off[:-1][off[1:] > off[:-1]]                      # the non-empty sentences' first ids
    sent = torch.searchsorted(starts, e, right=True) - 1       # the sentence of every position
    frag_start = torch.maximum(starts[sent.clamp_(0)], (e // L) * L)
    pos = torch.where(valid, e - frag_start, 0).to(torch.int32)
    is_start = torch.zeros(n_rows * L, dtype=torch.int64, device=ids.device)
    is_start[starts] = 1
    is_start[::L] = 1
    c = torch.cumsum(is_start, 0)
    row_first = c.view(n_rows, L)[:, :1] - 1
    seg = torch.where(valid.view(n_rows, L), c.view(n_rows, L) - row_first, 0).to(torch.int32)
    return rows.view(n_rows, L), seg, pos.view(n_rows, L)


def host_whole(lens, L):
    """the first sentence of every row of whole mode: the loop a user writes today"""
    starts, fill = [0], 0
    for i, n in enumerate(lens):
        if n == 0:
            continue
        if fill + n > L:
            starts.append(i)
            fill = 0
        fill += n
        if fill == L:
            starts.append(i + 1)
            fill = 0
    return starts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--lens", default="512,2048,8192")
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--dir", default=None, help="where the input file of (c) goes (default: a temporary directory)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="the summary (tools/pmc_summary.py kernel-stats) of a rocprofv3 --kernel-trace --stats run of --once")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    lens_L = [int(v) for v in args.lens.split(",")]
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
    del d_text, d_off
    torch.cuda.synchronize()

    def pack(L, mode):
        core.blocks_discard()
        return core.blocks_ids_device_raw(ids.data_ptr(), off.data_ptr(), n, K, L, mode, pad, 0)

    if args.once:
        for mode in (STREAM, WHOLE):
            pack(lens_L[0], mode)
        print(json.dumps({"once": True, "ids": K, "sentences": n, "seq_len": lens_L[0]}))
        return
    res = {"metric": "blocks", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "ids": int(K), "encode_kernel_ms": round(enc_ms, 3), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "algorithmic_bytes_note": "read 4 K + 8 (S + 1); written 12 n_rows L + 8 n_frags + 8 (n_rows + 1)", "kernel": {}, "torch_ops_stream": {}, "host_loop_whole": {}}
    shape, times = {}, {}
    for L in lens_L:
        for mode in (STREAM, WHOLE):
            nr, nf, _ = pack(L, mode)
            shape[(L, mode)] = (nr, nf)
            times[(L, mode)] = []
    t_torch = {L: [] for L in lens_L}
    for L in lens_L:  # (a) against (b), once: the same arrays
        nr, nf, _ = pack(L, STREAM)
        rows = torch.empty((nr, L), dtype=torch.int32, device="cuda")
        seg, pos = torch.empty_like(rows), torch.empty_like(rows)
        core.copy_blocks_device(rows.data_ptr(), seg.data_ptr(), pos.data_ptr(), None, None, nr, nf)
        r2, s2, p2 = torch_stream(torch, ids, off, L, pad)
        assert torch.equal(rows, r2) and torch.equal(seg, s2) and torch.equal(pos, p2), L
        del rows, seg, pos, r2, s2, p2
    for _ in range(args.repeats):
        for L in lens_L:
            for mode in (STREAM, WHOLE):
                times[(L, mode)].append(pack(L, mode)[2])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = torch_stream(torch, ids, off, L, pad)
            b.record()
            torch.cuda.synchronize()
            t_torch[L].append(a.elapsed_time(b))
            del out
    for L in lens_L:
        for mode in (STREAM, WHOLE):
            nr, nf = shape[(L, mode)]
            alg = 4 * K + 8 * (n + 1) + 12 * nr * L + 8 * nf + 8 * (nr + 1)
            ms = statistics.median(times[(L, mode)])
            res["kernel"]["%s_L%d" % ("stream" if mode == STREAM else "whole", L)] = dict(
                stat(times[(L, mode)], "ms"), rows=nr, frags=nf, algorithmic_bytes=alg, gbs=round(alg / (ms / 1e3) / 1e9, 1),
                share_of_copy_ceiling=round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4))
        res["torch_ops_stream"]["L%d" % L] = dict(stat(t_torch[L], "ms"), ratio_to_kernel=round(statistics.median(t_torch[L]) / statistics.median(times[(L, STREAM)]), 2))
    h_lens = np.diff(off.cpu().numpy()).tolist()
    for L in lens_L:  # whole mode today: the row starts by a host loop (timed once), before any array is built from them
        t0 = time.perf_counter()
        starts = host_whole(h_lens, L)
        dt = time.perf_counter() - t0
        res["host_loop_whole"]["L%d" % L] = {"seconds_row_starts_only": round(dt, 3), "rows": len(starts) - (1 if starts[-1] >= n else 0),
                                             "ratio_to_kernel": round(dt * 1e3 / statistics.median(times[(L, WHOLE)]), 1)}
    if args.kernel_stats:
        rowsk = {}
        for r in csv.DictReader(open(args.kernel_stats)):  # (the summary tools/pmc_summary.py kernel-stats writes)
            if r["kernel"].startswith("k_blk_") or r["kernel"].startswith("k_scan") or "scan" in r["kernel"]:
                rowsk[r["kernel"]] = {"calls": int(r["calls"]), "avg_us": float(r["avg_us"]), "total_ms": float(r["total_ms"])}
        res["kernel_stats_once"] = rowsk
    del ids, off
    torch.cuda.empty_cache()
    if not args.no_file:
        tmp = tempfile.TemporaryDirectory(dir=args.dir)
        path, prefix, L = os.path.join(tmp.name, "input.txt"), os.path.join(tmp.name, "out"), lens_L[0]
        with open(path, "wb") as f:
            f.write(host)
        with open(path, "rb") as f:  # (in the page cache)
            while f.read(1 << 26):
                pass
        core.encode_file_blocks(path, prefix, L, STREAM, pad_value=pad)  # warm-up: pinned chunks, both lanes at full size
        f_new, f_old, rep = [], [], None
        for _ in range(args.file_repeats):
            t0 = time.perf_counter()
            rep = core.encode_file_blocks(path, prefix, L, STREAM, pad_value=pad, report=True)
            f_new.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            h_ids, h_off = core.encode_file(path, None)
            nr = (len(h_ids) + L - 1) // L
            rows = np.full(nr * L, pad, np.int32)
            rows[:len(h_ids)] = h_ids
            rows.tofile(prefix + ".np.rows")
            f_old.append(time.perf_counter() - t0)
            assert rep["rows"] == nr and rep["ids"] == len(h_ids)
            del h_ids, h_off, rows
        assert open(prefix + ".rows", "rb").read(1 << 24) == open(prefix + ".np.rows", "rb").read(1 << 24)
        res["file"] = {"bytes": N, "seq_len": L, "encode_file_blocks": stat(f_new), "encode_file_plus_numpy_rows_only": stat(f_old),
                       "ratio": round(statistics.median(f_old) / statistics.median(f_new), 3), "last_report": rep}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
