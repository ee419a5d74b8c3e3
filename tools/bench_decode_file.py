#!/usr/bin/env python3
"""tools/bench_decode_file.py -- decimal id text parsed and printed on the device (k_idtext.h) against the parent commit's only routes, on the MI355X.

The input is bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed), in HBM and written to a file (read once
before the timing, so it sits in the page cache); the model is the committed golden model tests/golden/train_readme_small.model, as in
tools/bench_encode_subword.py.  Its id text -- what `yttm encode --output_type id` prints for it -- is made once by the printer and is the
parser's input, in HBM and as a second file.  One process, the routes alternating within every repeat:
  (a) the printer: yttm_idtext_device's kernel_ms on the pending encode result; GB/s by 4 K + 8 (S + 1) read, B_out + 8 (S + 1) written
  (b) the parser: yttm_ids_parse_device's kernel_ms minus yttm_lines_device's for the same text; GB/s by N + 8 (n + 1) read, 4 K + 8 (n + 1) written
  (c) yttm_decode_text_device's kernel_ms: split + parse + decode
  (d) yttm_decode_file, file -> file, against the parent's only route `python -m youtokentome_amd.yttm_cli decode < ids.txt > out`
  (e) yttm_encode_file_idtext, file -> file, against `python -m youtokentome_amd.yttm_cli encode --output_type id < file > out`
Medians and spreads go to profiles/decode_file.json (and stdout).  --once runs (a), (b) and (c) once (the command to profile: rocprofv3
--kernel-trace --stats --output-format csv -d DIR -- python tools/bench_decode_file.py --once, then tools/pmc_summary.py kernel-stats DIR
profiles/decode_file_kernel_stats.csv)."""
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


def rate(ms, alg):
    return {"ms": round(ms, 4), "algorithmic_bytes": alg, "gbs": round(alg / (ms / 1e3) / 1e9, 1), "share_of_copy_ceiling": round(alg / (ms / 1e3) / 1e9 / COPY_CEILING_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--file-repeats", type=int, default=5, help="runs of the device routes of (d) and (e)")
    ap.add_argument("--parent-repeats", type=int, default=3, help="runs of the parent's routes of (d) and (e)")
    ap.add_argument("--dir", default=None, help="where the input and output files go (default: a temporary directory)")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_file.json"))
    args = ap.parse_args()
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

    def printed():
        n_ids, _ = core.encode_device_raw(d_text.data_ptr(), d_off.data_ptr(), n, N, ENCODE_LINE + 1)
        n_text, ms = core.idtext_device_raw(n)
        return ms, n_ids, n_text

    _, K, B_out = printed()
    d_ids_text = torch.empty(B_out, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    core.copy_decode_device(d_ids_text.data_ptr(), None, n)

    def parsed():
        _, _, ms_split = core.lines_device_raw(d_ids_text.data_ptr(), B_out)
        nl, ni, ms = core.ids_parse_device_raw(d_ids_text.data_ptr(), B_out)
        assert (nl, ni) == (n, K)
        return ms - ms_split, ms

    def decoded():
        nl, ni, nt, ms = core.decode_text_device_raw(d_ids_text.data_ptr(), B_out)
        assert (nl, ni) == (n, K)
        return ms, nt

    if args.once:
        printed(), parsed(), decoded()
        print(json.dumps({"once": True, "lines": n, "bytes": N, "ids": K, "id_text_bytes": B_out}))
        return
    printed(), parsed(), decoded()  # warm-up: the lanes' buffers
    a_k, b_k, b_all, c_k = [], [], [], []
    for _ in range(args.repeats):
        a_k.append(printed()[0])
        p, whole = parsed()
        b_k.append(p), b_all.append(whole)
        ms, dec_bytes = decoded()
        c_k.append(ms)
    ids_host = d_ids_text.cpu().numpy()
    del d_text, d_off, d_ids_text
    torch.cuda.empty_cache()

    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    path, ids_path, out_dev, out_par = (os.path.join(tmp.name, x) for x in ("input.txt", "ids.txt", "device.txt", "parent.txt"))
    with open(path, "wb") as f:
        f.write(host)
    ids_host.tofile(ids_path)
    del host, ids_host
    for p in (path, ids_path):  # (in the page cache)
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def parent(cmd, src, dst):
        t0 = time.perf_counter()
        with open(src, "rb") as fin, open(dst, "wb") as fout:
            r = subprocess.run(cli + cmd, stdin=fin, stdout=fout, stderr=subprocess.DEVNULL, env=env)
        assert r.returncode == 0
        return time.perf_counter() - t0

    res_files = {}
    for key, device_call, cmd, src in (("d_decode_file", lambda: core.decode_file(ids_path, out_dev, report=True), ["decode", "--model", model], ids_path),
                                       ("e_encode_file_idtext", lambda: core.encode_file_idtext(path, out_dev, report=True), ["encode", "--model", model, "--output_type", "id"], path)):
        device_call()  # warm-up: pinned chunks, both lanes at full size
        dev_w, par_w, report = [], [], None
        for rep in range(max(args.file_repeats, args.parent_repeats)):
            if rep < args.file_repeats:
                t0 = time.perf_counter()
                report = device_call()
                dev_w.append(time.perf_counter() - t0)
            if rep < args.parent_repeats:
                par_w.append(parent(cmd, src, out_par))
        res_files[key] = {"device_file_to_file": stat(dev_w), "last_report": report, "parent_cli": stat(par_w) if par_w else None,
                          "ratio_parent_over_device": round(statistics.median(par_w) / statistics.median(dev_w), 2) if par_w else None,
                          "wrote_the_same_file": filecmp.cmp(out_dev, out_par, shallow=False) if par_w else None}

    res = {"metric": "decode_file", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "lines": n, "line_chars": ENCODE_LINE,
           "bytes": N, "ids": int(K), "id_text_bytes": int(B_out), "decoded_text_bytes": int(dec_bytes), "copy_ceiling_gbs": COPY_CEILING_GBS,
           "a_idtext_device_kernel": stat(a_k, "ms"), "a_print": rate(statistics.median(a_k), 4 * K + 8 * (n + 1) + B_out + 8 * (n + 1)),
           "b_parse_kernel": stat(b_k, "ms"), "b_split_plus_parse_kernel": stat(b_all, "ms"),
           "b_parse": rate(statistics.median(b_k), B_out + 8 * (n + 1) + 4 * K + 8 * (n + 1)),
           "bytes_note": "print: 4 K + 8 (S + 1) read, B_out + 8 (S + 1) written; parse: N + 8 (n + 1) read, 4 K + 8 (n + 1) written (N = the id text); each write pass reads its input a second time, which is not counted",
           "c_decode_text_device_kernel": stat(c_k, "ms")}
    res.update(res_files)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
