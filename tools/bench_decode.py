#!/usr/bin/env python3
"""tools/bench_decode.py -- the device decode against the host route it replaces, on the MI355X.

The batch is bench.py --full's encode batch (10^7 sentences of 128 chars, the same generator and seed); the model is the committed golden
model tests/golden/train_readme_small.model (vocab 600, trained on the same kind of text) -- training bench.py's 32 000-entry model here would
cost a training per run.  The batch is encoded once; then, in one process and alternating:
  (a) yttm_decode_device alone: its kernel_ms, and host wall time up to its return (the stream has synchronised)
  (b) the full device route: yttm_decode_device + yttm_decode_fetch
  (c) the route of the parent commit: yttm_encode_fetch + host yttm_decode
Each is warmed up once; medians and spreads of --repeats runs go to profiles/decode_device.json (and stdout).  --once runs (a) and (b) once
each (the command to profile: rocprofv3 --kernel-trace --stats -- python tools/bench_decode.py --once, then tools/pmc_summary.py kernel-stats).
--merge-kernel-stats FILE adds that run's per-kernel split of the decode to the result file, if both are of the same sources (no GPU needed)."""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=0, help="runs of route (c); 0: as many as --repeats")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_device.json"))
    ap.add_argument("--merge-kernel-stats", metavar="CSV")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        import csv
        from pmc_summary import source_sha16
        res = json.load(open(args.out))
        if res["source_sha16"] != source_sha16(ROOT):
            raise SystemExit("%s is of sources %s, this tree is %s" % (args.out, res["source_sha16"], source_sha16(ROOT)))
        rows = {r["kernel"]: r for r in csv.DictReader(open(args.merge_kernel_stats))}
        split = {k: round(float(rows[k]["avg_us"]) / 1e3, 3) for k in ("k_decode<false, false>", "k_scan_block_sums", "k_scan_sums", "k_scan_apply", "k_decode<false, true>") if k in rows}
        res["kernel_split_ms_per_launch"] = dict(split, source="%s (rocprofv3 --kernel-trace --stats of `tools/bench_decode.py --once`; the scan kernels' average includes the encoder's scans)"
                                                 % os.path.relpath(args.merge_kernel_stats, ROOT))
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res["kernel_split_ms_per_launch"]))
        return
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    from youtokentome_amd import _lib
    L = _lib.load()
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    bpe = yttm.BPE(model)
    h = bpe.bpe_cython._h
    err = C.create_string_buffer(_lib.ERRLEN)
    host = gen.abcd_corpus(args.sentences * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n = len(host) // (ENCODE_LINE + 1)
    d_bytes = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    del host
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    ids, off = bpe.encode_tensor((d_bytes, d_off), padded=False)  # the ids in HBM, in tensors of our own; the encoder keeps its copy for route (c)
    del d_bytes, d_off
    K = ids.numel()
    torch.cuda.synchronize()
    n_bytes, kms = C.c_uint64(), C.c_double()

    def check(rc):
        if rc != 0:
            raise RuntimeError(err.value.decode())

    def route_a():
        t0 = time.perf_counter()
        check(L.yttm_decode_device(h, C.c_void_p(ids.data_ptr()), C.c_void_p(off.data_ptr()), n, K, None, 0, C.byref(n_bytes), C.byref(kms), err, _lib.ERRLEN))
        return time.perf_counter() - t0, kms.value / 1e3

    text = np.empty(1, np.uint8)
    toff = np.empty(n + 1, np.uint64)

    def route_b():
        nonlocal text
        t0 = time.perf_counter()
        check(L.yttm_decode_device(h, C.c_void_p(ids.data_ptr()), C.c_void_p(off.data_ptr()), n, K, None, 0, C.byref(n_bytes), None, err, _lib.ERRLEN))
        if text.size < n_bytes.value:
            text = np.empty(n_bytes.value, np.uint8)
        check(L.yttm_decode_fetch(h, C.c_void_p(text.ctypes.data), toff.ctypes.data_as(_lib.u64p), n, err, _lib.ERRLEN))
        return time.perf_counter() - t0

    h_ids, h_off = np.empty(K, np.int32), np.empty(n + 1, np.uint64)
    last_c = {}

    def route_c():
        t0 = time.perf_counter()
        check(L.yttm_encode_fetch(h, h_ids.ctypes.data_as(_lib.i32p), h_off.ctypes.data_as(_lib.u64p), n, err, _lib.ERRLEN))
        blob_p, ooff = C.c_void_p(), _lib.u64p()
        check(L.yttm_decode(h, h_ids.ctypes.data_as(_lib.i32p), h_off.ctypes.data_as(_lib.u64p), n, None, 0, C.byref(blob_p), C.byref(ooff), err, _lib.ERRLEN))
        dt = time.perf_counter() - t0
        oo = np.ctypeslib.as_array(ooff, shape=(n + 1,))
        last_c["same"] = bool(np.array_equal(oo, toff) and np.array_equal(np.ctypeslib.as_array(C.cast(blob_p, C.POINTER(C.c_uint8)), shape=(int(oo[-1]),)), text[:int(oo[-1])]))
        L.yttm_free(blob_p)
        L.yttm_free(C.cast(ooff, C.c_void_p))
        return dt

    if args.once:
        route_a()
        route_b()
        print(json.dumps({"once": True, "sentences": n, "ids": K, "out_bytes": n_bytes.value}))
        return
    route_a(), route_b(), route_c()  # warm-up: the piece table, the lanes' buffers, the host allocator
    ta, tk, tb, tc = [], [], [], []
    host_repeats = args.host_repeats or args.repeats
    for i in range(args.repeats):
        w, k = route_a()
        ta.append(w)
        tk.append(k)
        tb.append(route_b())
        if i < host_repeats:
            tc.append(route_c())

    def stat(v):
        return {"median_s": round(statistics.median(v), 6), "min_s": round(min(v), 6), "max_s": round(max(v), 6), "runs": len(v),
                "spread": round((max(v) - min(v)) / statistics.median(v), 4)}
    B_out = n_bytes.value
    alg = {"read": 4 * K + 8 * (n + 1), "written": B_out + 8 * (n + 1)}
    a_k = statistics.median(tk)
    res = {"metric": "decode_device", "source_sha16": source_sha16(ROOT), "model": "tests/golden/train_readme_small.model", "sentences": n, "sentence_chars": ENCODE_LINE,
           "ids": K, "out_bytes": B_out, "algorithmic_bytes": dict(alg, total=alg["read"] + alg["written"], note="4 K + 8 (S+1) read, B_out + 8 (S+1) written; the piece table stays in L2"),
           "a_decode_device_kernel": stat(tk), "a_decode_device_wall": stat(ta), "b_device_route_decode_plus_fetch": stat(tb), "c_parent_route_encode_fetch_plus_host_decode": stat(tc),
           "a_kernel_gbs": round((alg["read"] + alg["written"]) / a_k / 1e9, 1), "a_share_of_copy_ceiling": round((alg["read"] + alg["written"]) / a_k / 1e9 / COPY_CEILING_GBS, 4),
           "copy_ceiling_gbs": COPY_CEILING_GBS, "a_sentences_per_s": round(n / a_k, 1),
           "ratio_c_over_b": round(statistics.median(tc) / statistics.median(tb), 2), "b_beats_c_beyond_spread": bool(max(tb) < min(tc)),
           "routes_agree_bytes_and_offsets": last_c.get("same")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
