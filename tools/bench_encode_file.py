#!/usr/bin/env python3
"""tools/bench_encode_file.py -- the line split on the device and the file route on top of it, against the routes of the parent commit, on the MI355X.

The input is bench.py --full's encode batch written to a file (10^7 lines of 128 chars, the same generator and seed; read once before the
timing, so it sits in the page cache); the model is the committed golden model tests/golden/train_readme_small.model, as in tools/bench_decode.py.
One process, the routes alternating within every repeat:
  (a) yttm_lines_device alone on the text in HBM: its kernel_ms, GB/s by its algorithmic bytes N + 8 (n + 1), as a share of the copy ceiling
  (b) yttm_encode_text_device on the resident text against yttm_encode_device with offsets made beforehand: the difference is the split's price
  (c) yttm_encode_file, file -> host arrays and file -> PREFIX.ids / .off, at several piece sizes and with the default (chunk_bytes = 0)
  (d) the parent's routes: numpy split (np.flatnonzero(buf == 10)) + encode_packed on the file's bytes; and
      `python -m youtokentome_amd.yttm_cli encode --output_type id < file > /dev/null`
Medians and spreads go to profiles/encode_file.json (and stdout).  --once runs (a) and (b) once each (the command to profile: rocprofv3
--kernel-trace --stats --output-format csv -d DIR -- python tools/bench_encode_file.py --once, then tools/pmc_summary.py kernel-stats DIR
profiles/encode_file_kernel_stats.csv)."""
import argparse
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
    ap.add_argument("--file-repeats", type=int, default=3, help="runs of every piece size of route (c)")
    ap.add_argument("--parent-repeats", type=int, default=2, help="runs of the routes (d)")
    ap.add_argument("--piece-mb", default="64,128,256,512,1024", help="piece sizes of route (c); the default size and the whole file in one piece are added")
    ap.add_argument("--dir", default=None, help="where the input and output files go (default: a temporary directory)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_file.json"))
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

    def route_a():
        t0 = time.perf_counter()
        n_lines, longest, ms = core.lines_device_raw(d_text.data_ptr(), N)
        assert (n_lines, longest) == (n, ENCODE_LINE + 1)
        return time.perf_counter() - t0, ms

    def route_b_text():
        t0 = time.perf_counter()
        n_lines, n_ids, ms = core.encode_text_device_raw(d_text.data_ptr(), N)
        return time.perf_counter() - t0, ms, n_ids

    def route_b_offsets():
        t0 = time.perf_counter()
        n_ids, ms = core.encode_device_raw(d_text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        return time.perf_counter() - t0, ms, n_ids

    if args.once:
        route_a()
        route_b_text()
        print(json.dumps({"once": True, "lines": n, "bytes": N}))
        return
    route_a(), route_b_text(), route_b_offsets()  # warm-up: the lanes' buffers
    a_w, a_k, bt_w, bt_k, bo_w, bo_k = [], [], [], [], [], []
    for _ in range(args.repeats):
        w, k = route_a()
        a_w.append(w), a_k.append(k)
        w, k, ids_text = route_b_text()
        bt_w.append(w), bt_k.append(k)
        w, k, ids_off = route_b_offsets()
        bo_w.append(w), bo_k.append(k)
        assert ids_text == ids_off
    want_ids, want_off = core.fetch_encode(n, ids_off)
    want_ids = want_ids.copy()
    del d_text, d_off
    torch.cuda.empty_cache()

    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    path, prefix = os.path.join(tmp.name, "input.txt"), os.path.join(tmp.name, "out")
    with open(path, "wb") as f:
        f.write(host)
    del host
    with open(path, "rb") as f:  # (in the page cache)
        while f.read(1 << 26):
            pass
    whole = N + 1
    sizes = [0] + [int(x) << 20 for x in args.piece_mb.split(",") if x] + [whole]
    names = {0: "default", whole: "whole_file"}
    core.encode_file(path, None, chunk_bytes=whole)  # warm-up: pinned chunks, both lanes at full size
    table = {names.get(s, "%d_MB" % (s >> 20)): {"arrays": [], "files": [], "inside": [], "report": None} for s in sizes}
    same = True
    d_np, d_cli = [], []
    env = dict(os.environ, PYTHONPATH=ROOT)

    def parent_numpy():
        t0 = time.perf_counter()
        buf = np.fromfile(path, np.uint8)
        nl = np.flatnonzero(buf == 10)
        off = np.zeros(len(nl) + 1 + (1 if len(buf) and buf[-1] != 10 else 0), np.uint64)
        off[1:len(nl) + 1] = nl + 1
        off[-1] = len(buf)
        ids, o = core.encode_packed(buf.tobytes(), off)
        dt = time.perf_counter() - t0
        return dt, bool(np.array_equal(ids, want_ids) and np.array_equal(o, want_off))

    def parent_cli():
        t0 = time.perf_counter()
        with open(path, "rb") as fin, open(os.devnull, "wb") as fout:
            r = subprocess.run([sys.executable, "-m", "youtokentome_amd.yttm_cli", "encode", "--model", model, "--output_type", "id"], stdin=fin, stdout=fout,
                               stderr=subprocess.DEVNULL, env=env)
        assert r.returncode == 0
        return time.perf_counter() - t0

    for rep in range(max(args.file_repeats, args.parent_repeats)):
        if rep < args.file_repeats:
            for s in sizes:
                row = table[names.get(s, "%d_MB" % (s >> 20))]
                t0 = time.perf_counter()
                ids, off, report = core.encode_file(path, None, chunk_bytes=s, report=True)
                row["arrays"].append(time.perf_counter() - t0)
                row["inside"].append(report["seconds_total"])
                same = same and bool(np.array_equal(ids, want_ids) and np.array_equal(off, want_off))
                del ids, off
                t0 = time.perf_counter()
                core.encode_file(path, prefix, chunk_bytes=s)
                row["files"].append(time.perf_counter() - t0)
                row["report"] = report
        if rep < args.parent_repeats:
            dt, ok = parent_numpy()
            d_np.append(dt)
            same = same and ok
            d_cli.append(parent_cli())
    f_ids, f_off = np.fromfile(prefix + ".ids", np.int32), np.fromfile(prefix + ".off", np.uint64)
    same = same and bool(np.array_equal(f_ids, want_ids) and np.array_equal(f_off, want_off))

    alg = N + 8 * (n + 1)
    ak = statistics.median(a_k) / 1e3
    c_table = {k: {"piece_bytes": v["report"]["piece_bytes"], "pieces": v["report"]["pieces"], "file_to_arrays": stat(v["arrays"]), "file_to_arrays_inside_the_library": stat(v["inside"]), "file_to_files": stat(v["files"]),
                   "last_report": v["report"]} for k, v in table.items()}
    best = min((k for k in c_table if k != "default"), key=lambda k: c_table[k]["file_to_arrays"]["median_s"])
    c_def = c_table["default"]
    res = {"metric": "encode_file", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "bytes": N, "ids": int(ids_off),
           "a_lines_device_kernel": stat(a_k, "ms"), "a_lines_device_wall": stat(a_w),
           "a_algorithmic_bytes": {"total": alg, "note": "N read + 8 (n + 1) written; the write pass reads the text a second time, which is not counted"},
           "a_kernel_gbs": round(alg / ak / 1e9, 1), "a_share_of_copy_ceiling": round(alg / ak / 1e9 / COPY_CEILING_GBS, 4), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "b_encode_text_device_kernel": stat(bt_k, "ms"), "b_encode_device_precomputed_offsets_kernel": stat(bo_k, "ms"),
           "b_encode_text_device_wall": stat(bt_w), "b_encode_device_precomputed_offsets_wall": stat(bo_w),
           "b_price_of_the_split_ms": round(statistics.median(bt_k) - statistics.median(bo_k), 4),
           "c_encode_file_by_piece_size": c_table, "c_best_piece_size_file_to_arrays": best,
           "d_parent_numpy_split_plus_encode_packed": stat(d_np), "d_parent_cli_encode_output_type_id": stat(d_cli),
           "ratio_d_numpy_over_c_default": round(statistics.median(d_np) / c_def["file_to_arrays"]["median_s"], 2),
           "ratio_d_cli_over_c_default_files": round(statistics.median(d_cli) / c_def["file_to_files"]["median_s"], 2),
           "c_default_beats_d_beyond_spread": bool(max(table["default"]["arrays"]) * 1.03 < min(d_np) and max(table["default"]["files"]) * 1.03 < min(d_cli)),
           "b_within_a_plus_noise": bool(statistics.median(bt_k) - statistics.median(bo_k) <= statistics.median(a_k) + 0.03 * statistics.median(bo_k)),
           "routes_agree_ids_and_offsets": same}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
