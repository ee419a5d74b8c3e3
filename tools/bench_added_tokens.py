#!/usr/bin/env python3
"""tools/bench_added_tokens.py -- the added tokens (k_added.h) on the MI355X.

The input is bench.py --full's encode batch (10^7 lines of 128 chars, the same generator and seed) in HBM; the model is the committed golden
model tests/golden/train_readme_small.model.  One process, the cases alternating within every repeat:
  (a) yttm_encode_device's kernel_ms on the plain batch with the setting off
  (b) the same with 100 tokens set that never match: the difference to (a) is the split's measure pass and its scan (the write pass, the
      second encode and the join are skipped -- the encoder's counters prove it)
  (c) a tag in front of every sentence (alternately <2en> and <2de>), setting on
  (d) the tag plus the token <mask> inside --inside-share of the words (default 1 %), setting on
  (e) yttm_added_split_device alone on the text of (d): its own kernel_ms, GB/s by its algorithmic bytes N + 8 (S + 1) read and
      8 (n_sub + 1) + 4 n_sub + 8 (S + 1) written, as a share of the copy ceiling; beside it yttm_lines_device (k_lines.h) on the same text, what a
      streaming reader of these bytes achieves in this code base
(c) and (d) are also run with the setting off on the same texts: what the encoder costs there without the feature (the tags are then ordinary
words).  Medians and spreads go to profiles/added_tokens.json (and stdout).  --once runs (e) and one encode of (d) once (the command to
profile: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_added_tokens.py --once, then tools/pmc_summary.py
kernel-stats DIR profiles/added_tokens_kernel_stats.csv)."""
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
TAGS = [b"<2en>", b"<2de>"]
INSIDE = b"<mask>"


def stat(v, unit="ms"):
    m = statistics.median(v)
    return {"median_" + unit: round(m, 4), "min_" + unit: round(min(v), 4), "max_" + unit: round(max(v), 4), "runs": len(v), "spread": round((max(v) - min(v)) / m, 4) if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inside-share", type=float, default=0.01)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "added_tokens.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import gen
    from bench import ENCODE_LINE
    from pmc_summary import source_sha16
    import youtokentome_amd as yttm
    model = os.path.join(ROOT, "tests", "golden", "train_readme_small.model")
    off_core, on_core, idle_core = yttm.BPE(model).bpe_cython, yttm.BPE(model).bpe_cython, yttm.BPE(model).bpe_cython
    on_core.set_added_tokens(TAGS + [INSIDE])
    idle_core.set_added_tokens([b"<never%d>" % k for k in range(100)])
    W = ENCODE_LINE + 1
    host = gen.abcd_corpus(args.sentences * W, seed=123, line=ENCODE_LINE, survey_stream=True)
    n, N = len(host) // W, len(host)
    plain = np.frombuffer(host, np.uint8)[:n * W].reshape(n, W)
    # (c): a tag in front of every sentence
    T = len(TAGS[0])
    tagged = np.empty((n, T + W), np.uint8)
    tagged[0::2, :T] = np.frombuffer(TAGS[0], np.uint8)
    tagged[1::2, :T] = np.frombuffer(TAGS[1], np.uint8)
    tagged[:, T:] = plain
    tagged = tagged.reshape(-1)
    tag_off = np.arange(n + 1, dtype=np.int64) * (T + W)
    # (d): and <mask> inside a share of the words: at byte positions whose neighbours on both sides are letters
    letter = (tagged != 10) & (tagged != 32)
    n_words = int(len(letter) - np.count_nonzero(letter))
    rng = np.random.default_rng(5)
    want = int(n_words * args.inside_share)
    pos = np.unique(rng.integers(1, len(tagged), size=3 * want))  # (sorted) candidates: kept where both neighbours are letters, behind the tag
    pos = pos[letter[pos] & letter[pos - 1] & (pos % (T + W) > T)]
    pos = pos[np.concatenate(([True], np.diff(pos) > 1))]  # (never two insertions at neighbouring bytes)
    pos = np.sort(rng.permutation(pos)[:want])
    mixed = np.insert(tagged, np.repeat(pos, len(INSIDE)), np.tile(np.frombuffer(INSIDE, np.uint8), len(pos)))
    mix_off = tag_off + len(INSIDE) * np.searchsorted(pos, tag_off, side="left")
    d_plain = torch.from_numpy(plain.reshape(-1).copy()).cuda()
    d_plain_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * W
    d_tag, d_tag_off = torch.from_numpy(tagged).cuda(), torch.from_numpy(tag_off).cuda()
    d_mix, d_mix_off = torch.from_numpy(mixed).cuda(), torch.from_numpy(mix_off).cuda()
    mix_longest = int(np.diff(mix_off).max())
    n_inside = len(pos)
    n_mix = len(mixed)
    torch.cuda.synchronize()
    del host, plain, tagged, mixed, letter

    def encode(core, text, off, total, longest):
        n_ids, ms = core.encode_device_raw(text.data_ptr(), off.data_ptr(), n, total, longest)
        return ms, n_ids

    def enc_plain(core):
        return encode(core, d_plain, d_plain_off, n * W, W)

    def enc_tag(core):
        return encode(core, d_tag, d_tag_off, n * (T + W), T + W)

    def enc_mix(core):
        return encode(core, d_mix, d_mix_off, n_mix, mix_longest)

    def split():
        return on_core.added_split_device_raw(d_mix.data_ptr(), d_mix_off.data_ptr(), n, n_mix)

    def lines():
        return on_core.lines_device_raw(d_mix.data_ptr(), n_mix)

    if args.once:
        split()
        enc_mix(on_core)
        print(json.dumps({"once": True, "lines": n, "bytes": n_mix}))
        return
    enc_plain(off_core), enc_plain(idle_core), enc_tag(on_core), enc_mix(on_core), enc_tag(off_core), enc_mix(off_core), split(), lines()  # warm-up: the lanes' buffers
    a, b, c, d, c0, d0, e_ms, l_ms = [], [], [], [], [], [], [], []
    s_idle0, s_on0 = idle_core.added_tokens_stats(), on_core.added_tokens_stats()
    for _ in range(args.repeats):
        ms, ids_plain = enc_plain(off_core)
        a.append(ms)
        ms, ids = enc_plain(idle_core)
        b.append(ms)
        assert ids == ids_plain
        ms, _ = enc_tag(off_core)
        c0.append(ms)
        ms, ids_tag = enc_tag(on_core)
        c.append(ms)
        ms, _ = enc_mix(off_core)
        d0.append(ms)
        ms, ids_mix = enc_mix(on_core)
        d.append(ms)
        n_sub, n_matches, ms = split()
        e_ms.append(ms)
        l_ms.append(lines()[2])
    s_idle1, s_on1 = idle_core.added_tokens_stats(), on_core.added_tokens_stats()
    R = args.repeats
    assert (s_idle1[0] - s_idle0[0], s_idle1[1] - s_idle0[1], s_idle1[2] - s_idle0[2]) == (R, R, 0), "tokens that never match skip the write pass and the join"
    assert (s_on1[0] - s_on0[0], s_on1[1] - s_on0[1]) == (2 * R, 0) and s_on1[2] - s_on0[2] == R * (n + n + n_inside)
    assert n_matches == n + n_inside and n_sub == n + 2 * n_matches
    read, written = n_mix + 8 * (n + 1), 8 * (n_sub + 1) + 4 * n_sub + 8 * (n + 1)
    ms = statistics.median(e_ms)
    gbs = (read + written) / (ms / 1e3) / 1e9
    med = statistics.median
    res = {
        "source_sha16": source_sha16(), "sentences": n, "bytes_plain": N, "bytes_tagged": n * (T + W), "bytes_tagged_inside": n_mix, "inside_share": args.inside_share,
        "tokens_inside": n_inside,
        "encode_off_plain": stat(a), "encode_idle_tokens_plain": stat(b), "idle_price_ms": round(med(b) - med(a), 4),
        "tagged": {"encode_off": stat(c0), "encode_on": stat(c), "price_over_plain_off_ms": round(med(c) - med(a), 4), "ids_on": ids_tag},
        "tagged_inside": {"encode_off": stat(d0), "encode_on": stat(d), "price_over_plain_off_ms": round(med(d) - med(a), 4), "ids_on": ids_mix},
        "split_alone": {"kernel": stat(e_ms), "n_sub": n_sub, "matches": n_matches, "bytes_read": read, "bytes_written": written, "gbs": round(gbs, 1),
                        "share_of_copy_ceiling": round(gbs / COPY_CEILING_GBS, 4), "k_lines_same_text": stat(l_ms)},
    }
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
