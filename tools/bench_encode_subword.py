#!/usr/bin/env python3
"""tools/bench_encode_subword.py -- SUBWORD output made on the device (k_subword.h) against the parent commit's only route, on the MI355X.

The input is bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed), in HBM and written to a file (read once
before the timing, so it sits in the page cache); the model is the committed golden model tests/golden/train_readme_small.model, as in
tools/bench_encode_file.py.  One process, the routes alternating within every repeat:
  (a) yttm_subword_device on the resident batch: its kernel_ms, and yttm_encode_device's kernel_ms for the same batch -- the difference is the
      format (measure + scan + write); GB/s of the format by its algorithmic bytes 4 K + 8 (S + 1) read (+ the text of the sentences that hold
      an unk_id: none in this batch), B_out + 8 (S + 1) written, as a share of the copy ceiling
  (b) the same with --unk-share of the chars replaced by chars outside the alphabet (default 1 %): most sentences then walk their text
  (c) yttm_encode_file_subword, file -> file
  (d) the parent's only route: `python -m youtokentome_amd.yttm_cli encode --output_type subword < file > out`
  (e) for scale: yttm_encode_file to PREFIX.ids / PREFIX.off
Medians and spreads go to profiles/encode_subword.json (and stdout).  --once runs (a) once (the command to profile: rocprofv3 --kernel-trace
--stats --output-format csv -d DIR -- python tools/bench_encode_subword.py --once, then tools/pmc_summary.py kernel-stats DIR
profiles/encode_subword_kernel_stats.csv)."""
import argparse
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile
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
    ap.add_argument("--file-repeats", type=int, default=5, help="runs of the routes (c) and (e)")
    ap.add_argument("--parent-repeats", type=int, default=5, help="runs of the route (d)")
    ap.add_argument("--unk-share", type=float, default=0.01)
    ap.add_argument("--dir", default=None, help="where the input and output files go (default: a temporary directory)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_subword.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // (ENCODE_LINE + 1), len(host)
    d_text = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    torch.cuda.synchronize()

    def subword(text):
        t0 = time.perf_counter()
        n_ids, n_text, ms = core.subword_device_raw(text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return time.perf_counter() - t0, ms, n_ids, n_text

    def encode(text):
        n_ids, ms = core.encode_device_raw(text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return ms, n_ids

    if args.once:
        subword(d_text)
        print(json.dumps({"once": True, "lines": n, "bytes": N}))
        return
    # (b): the same batch with a share of its letters replaced by a one-byte char outside the alphabet (the sentences keep their offsets)
    arr = np.frombuffer(host, np.uint8).copy()
    hit = (np.random.default_rng(5).random(len(arr)) < args.unk_share) & (arr != 10) & (arr != 32)
    arr[hit] = ord("Z")
    d_unk = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    del arr
    subword(d_text), encode(d_text), subword(d_unk), encode(d_unk)  # warm-up: the lanes' buffers
    a_w, a_k, a_e, b_k, b_e = [], [], [], [], []
    for _ in range(args.repeats):
        w, k, ids_a, text_a = subword(d_text)
        a_w.append(w), a_k.append(k)
        ms, ids = encode(d_text)
        a_e.append(ms)
        assert ids == ids_a
        w, k, ids_b, text_b = subword(d_unk)
        b_k.append(k)
        ms, ids = encode(d_unk)
        b_e.append(ms)
        assert ids == ids_b
    # sentences of (b) that hold a replaced char, and so an unk_id: those walk their text (counted on the device, from the text itself)
    b_sentences_with_unk = int((d_unk.view(n, ENCODE_LINE + 1) == ord("Z")).any(dim=1).sum())
    del d_text, d_off, d_unk
    torch.cuda.empty_cache()

    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    path, out_c, out_d, prefix = (os.path.join(tmp.name, x) for x in ("input.txt", "device.txt", "parent.txt", "ids"))
    with open(path, "wb") as f:
        f.write(host)
    del host
    with open(path, "rb") as f:  # (in the page cache)
        while f.read(1 << 26):
            pass
    core.encode_file_subword(path, out_c)  # warm-up: pinned chunks, both lanes at full size
    c_w, c_in, d_w, e_w = [], [], [], []
    report = None
    env = dict(os.environ, PYTHONPATH=ROOT)
    for rep in range(max(args.file_repeats, args.parent_repeats)):
        if rep < args.file_repeats:
            t0 = time.perf_counter()
            report = core.encode_file_subword(path, out_c, report=True)
            c_w.append(time.perf_counter() - t0)
            c_in.append(report["seconds_total"])
            t0 = time.perf_counter()
            core.encode_file(path, prefix)
            e_w.append(time.perf_counter() - t0)
        if rep < args.parent_repeats:
            t0 = time.perf_counter()
            with open(path, "rb") as fin, open(out_d, "wb") as fout:
                r = subprocess.run([sys.executable, "-m", "youtokentome_amd.yttm_cli", "encode", "--model", model, "--output_type", "subword"], stdin=fin,
                                   stdout=fout, stderr=subprocess.DEVNULL, env=env)
            assert r.returncode == 0
            d_w.append(time.perf_counter() - t0)
    same = filecmp.cmp(out_c, out_d, shallow=False) if d_w else None

    def gbs(k_ms, e_ms, ids, text, read_text):
        fmt = statistics.median(k_ms) - statistics.median(e_ms)
        alg = 4 * ids + 8 * (n + 1) + read_text + text + 8 * (n + 1)
        return {"format_ms": round(fmt, 4), "algorithmic_bytes": alg, "gbs": round(alg / (fmt / 1e3) / 1e9, 1),
                "share_of_copy_ceiling": round(alg / (fmt / 1e3) / 1e9 / COPY_CEILING_GBS, 4)}

    res = {"metric": "encode_subword", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "bytes": N, "ids": int(ids_a), "text_bytes": int(text_a), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "a_subword_device_kernel": stat(a_k, "ms"), "a_encode_device_kernel": stat(a_e, "ms"), "a_subword_device_wall": stat(a_w),
           "a_format": gbs(a_k, a_e, ids_a, text_a, 0),
           "a_algorithmic_bytes_note": "4 K + 8 (S + 1) read (no sentence of this batch holds an unk_id), B_out + 8 (S + 1) written; the write pass reads the ids a second time, which is not counted",
           "b_unk_share": args.unk_share, "b_ids": int(ids_b), "b_text_bytes": int(text_b), "b_sentences_with_unk": b_sentences_with_unk,
           "b_subword_device_kernel": stat(b_k, "ms"), "b_encode_device_kernel": stat(b_e, "ms"),
           "b_format": gbs(b_k, b_e, ids_b, text_b, b_sentences_with_unk * (ENCODE_LINE + 1)),
           "b_algorithmic_bytes_note": "as (a) + the text of the sentences that hold an unk_id, counted once",
           "c_encode_file_subword_file_to_file": stat(c_w), "c_inside_the_library": stat(c_in), "c_last_report": report,
           "d_parent_cli_encode_output_type_subword": stat(d_w) if d_w else None,
           "e_encode_file_to_ids_and_off": stat(e_w),
           "ratio_d_over_c": round(statistics.median(d_w) / statistics.median(c_w), 2) if d_w else None,
           "c_and_d_wrote_the_same_file": same}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
