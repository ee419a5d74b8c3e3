#!/usr/bin/env python3
"""Calls every text route of the device encoder once on the golden readme_small model, so that a profiler's kernel trace of the run lists the
kernels and copies each route issues (profiles/text_routes_kernel_calls.txt: two builds, their lists compared).

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/text_routes_kernel_calls.py     # on its own, no counters
  python tools/text_routes_kernel_calls.py --summarise DIR                                # -> "calls  kernel name" lines, sorted by name

YTTM_AMD_LIB chooses the build.  The routes: encode_device + fetch, encode_text_device, decode_device + copy, subword_device, idtext_device,
ids_parse_device, decode_text_device, spans_device, encode_file, encode_file_subword, decode_file in three pieces."""
import csv
import glob
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarise(d):
    """the profiler's kernel statistics, from its CSV or from its database (whichever format it was asked for)"""
    csvs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if csvs:
        rows = [(r["Name"], int(r["Calls"])) for r in csv.DictReader(open(csvs[0]))]
    else:
        import sqlite3
        db = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)[0]
        rows = sqlite3.connect(db).execute("select name, count(*) from kernels group by name").fetchall()
    for name, calls in sorted(rows):
        print("%6d  %s" % (calls, name))
    print("%6d  calls of %d kernels" % (sum(c for _, c in rows), len(rows)))


def main():
    import numpy as np
    import torch

    import youtokentome_amd as yttm
    golden = os.path.join(ROOT, "tests", "golden")
    bpe = yttm.BPE(os.path.join(golden, "train_readme_small.model"))
    core = bpe.bpe_cython
    dev = torch.device("cuda", core.device)
    text = open(os.path.join(golden, "train_readme_small.txt"), "rb").read()
    lines = text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n")
    off = np.zeros(len(lines) + 1, np.int64)
    np.cumsum([len(ln) for ln in lines], out=off[1:])
    n, total, longest = len(lines), int(off[-1]), int(np.diff(off).max())

    def put(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        torch.cuda.synchronize()
        return t

    d_bytes, d_off, d_text = put(np.frombuffer(b"".join(lines), np.uint8).copy()), put(off), put(np.frombuffer(text, np.uint8).copy())
    # encode_device + fetch
    n_ids, _ = core.encode_device_raw(d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest)
    ids, ioff = core.fetch_encode(n, n_ids)
    # encode_text_device
    core.encode_text_device_raw(d_text.data_ptr(), len(text))
    # decode_device + copy
    d_ids, d_ioff = put(ids), put(ioff.view(np.int64))
    n_bytes, _ = core.decode_device_raw(d_ids.data_ptr(), d_ioff.data_ptr(), n, n_ids)
    out_text, out_off = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    core.copy_decode_device(out_text.data_ptr(), out_off.data_ptr(), n)
    # subword_device, idtext_device (of the ids the line before left pending)
    core.subword_device_raw(d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest)
    n_idtext, _ = core.idtext_device_raw(n)
    idtext, _ = core.fetch_decode(n, n_idtext)
    # ids_parse_device, decode_text_device
    d_idtext = put(idtext)
    core.ids_parse_device_raw(d_idtext.data_ptr(), int(n_idtext))
    core.decode_text_device_raw(d_idtext.data_ptr(), int(n_idtext))
    # spans_device
    core.spans_device_raw(d_bytes.data_ptr(), d_off.data_ptr(), n, total, longest)
    # the files
    with tempfile.TemporaryDirectory() as tmp:
        src, ids_txt = os.path.join(golden, "train_readme_small.txt"), os.path.join(tmp, "ids.txt")
        open(ids_txt, "wb").write(idtext.tobytes())
        bpe.encode_file(src)
        bpe.encode_file(src, os.path.join(tmp, "sub.txt"), output_type=yttm.OutputType.SUBWORD)
        rep = bpe.decode_file(ids_txt, os.path.join(tmp, "dec.txt"), chunk_bytes=int(n_idtext) * 9 // 20, report=True)  # (a piece ends behind its last newline: three pieces)
    print("text routes: %d sentences, %d ids, %d bytes of id text, decode_file in %d pieces" % (n, n_ids, n_idtext, rep["pieces"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
