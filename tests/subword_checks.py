"""Checks of SUBWORD output made on the device (yttm_subword_device, yttm_subword_text_device, yttm_encode_file_subword; the text is taken with
yttm_decode_fetch / yttm_decode_copy_device), shared by the emulator tests (test_subword_device.py, test_subword_device_sched.py: numpy arrays
are "device" memory there) and the MI355X tests (test_gpu_subword.py: torch tensors).

The output for a batch: per sentence every piece followed by one space, then "\\n"; one blob + uint64 line_off[n + 1].  Yardsticks, none of
them the code under test:
  1. the host path yttm_encode_as_subwords on the same sentences, formatted piece + " " ... "\\n" (pinned to the reference by the goldens'
     subword_000 lists and test_reference_suite.py);
  2. the subword_000 lists of tests/golden/encode_*.json, which the reference made;
  3. an independent formatter (format_ids) written from the rules: the ids PENDING after the call, BPE.vocab(), the alphabet from the model
     file's char section, white space = isspace() in the C locale or U+2581.  Valid UTF-8 only; it is what checks dropout;
  4. the ids: pending ids == yttm_encode_device's ids for the same arguments.
Equality is exact everywhere: bytes and offsets."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import refbin
from decode_checks import G, NumpyBuf, TorchBuf, golden_names, golden_sentences, model_args  # noqa: F401  (the buffers are re-exported)
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ((0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1))
BOS_MSG = "Can't add <BOS> token. Model was trained without it."


def model_path(name):
    return name if os.path.sep in name else os.path.join(G, f"train_{name}.model")


def bpe_of(name):
    import youtokentome_amd as yttm
    return yttm.BPE(model_path(name))


def to_bytes(sents):
    return [s.encode() if isinstance(s, str) else bytes(s) for s in sents]


# ---- yardstick 1: the host path ----------------------------------------------------------------------------------------------------------
def host_text(core, sents, bos=0, eos=0, rev=0, dropout=0.0):
    """yttm_encode_as_subwords, formatted: (code, message, text bytes, line_off uint64[n + 1])"""
    L = _lib.load()
    blob, off = K.pack(to_bytes(sents))
    n = len(sents)
    blob_p, poff, soff, npieces, err = C.c_void_p(), _lib.u64p(), _lib.u64p(), C.c_uint64(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_encode_as_subwords(core._h, blob, off.ctypes.data_as(_lib.u64p), n, bos, eos, rev, float(dropout), C.byref(blob_p), C.byref(poff),
                                   C.byref(npieces), C.byref(soff), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None
    P = npieces.value
    po = np.ctypeslib.as_array(poff, shape=(P + 1,)).astype(np.int64)
    so = np.ctypeslib.as_array(soff, shape=(n + 1,)).astype(np.int64)
    raw = np.frombuffer(C.string_at(blob_p, int(po[-1])), np.uint8)
    for p in (blob_p, C.cast(poff, C.c_void_p), C.cast(soff, C.c_void_p)):
        L.yttm_free(p)
    # piece i of sentence j lands behind i spaces and j newlines
    sent_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(so))
    shift = np.arange(P, dtype=np.int64) + sent_of
    out = np.zeros(int(po[-1]) + P + n, np.uint8)
    out[np.arange(len(raw), dtype=np.int64) + np.repeat(shift, np.diff(po))] = raw
    out[po[1:] + shift] = 0x20
    nl = po[so[1:]] + so[1:] + np.arange(n, dtype=np.int64)
    out[nl] = 0x0A
    line_off = np.zeros(n + 1, np.uint64)
    line_off[1:] = nl + 1
    return 0, "", out.tobytes(), line_off


# ---- yardstick 3: an independent formatter -------------------------------------------------------------------------------------------------
def alphabet_of(path):
    """the model file's char section: "n_chars n_rules", then n_chars lines "code point, id" """
    tok = open(path).read().split()
    n = int(tok[0])
    return {int(tok[2 + 2 * i]) for i in range(n)}


def is_space(cp):
    return cp == 0x2581 or cp == 32 or 9 <= cp <= 13


def runs_of(sentence, alphabet):
    """maximal runs of non-space code points outside the alphabet (valid UTF-8 only)"""
    runs, cur = [], ""
    for ch in sentence:
        if not is_space(ord(ch)) and ord(ch) not in alphabet:
            cur += ch
            continue
        if cur:
            runs.append(cur)
        cur = ""
    if cur:
        runs.append(cur)
    return runs


def format_ids(sentence, ids, vocab, alphabet, unk, rev):
    runs = runs_of(sentence, alphabet)
    out, k = [], 0
    for t in ids:
        if t == unk:
            r = len(runs) - 1 - k if rev else k
            out.append(runs[r] if 0 <= r < len(runs) else "")
            k += 1
        else:
            out.append(vocab[t])
    return ("".join(p + " " for p in out) + "\n").encode()


# ---- the device path -----------------------------------------------------------------------------------------------------------------------
def dev_subword(core, B, sents, bos=0, eos=0, rev=0, dropout=0.0):
    """yttm_subword_device on bytes + offsets in device memory, the text by both exits (which must agree; 3 guard bytes behind it stay), the
    ids by yttm_encode_fetch: (code, message, text, line_off, ids, ids_off)"""
    L = _lib.load()
    raw = to_bytes(sents)
    blob, off = K.pack(raw)
    n = len(raw)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    ni, nt, ms, err = C.c_uint64(77), C.c_uint64(77), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_subword_device(core._h, C.c_void_p(B.ptr(d_b)), C.c_void_p(B.ptr(d_o)), n, len(blob), max([len(s) for s in raw] + [0]), bos, eos, rev,
                               float(dropout), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None, None, None
    text, line_off = D._take_result(core, B, n, nt.value)
    ids, ioff = D.encode_fetch(core, n, ni.value)
    return 0, "", text, line_off, ids, ioff


def dev_ids(core, B, sents, bos=0, eos=0, rev=0, dropout=0.0):
    """yardstick 4: yttm_encode_device + yttm_encode_fetch"""
    L = _lib.load()
    raw = to_bytes(sents)
    blob, off = K.pack(raw)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    ni, ms, err = C.c_uint64(), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_encode_device(core._h, C.c_void_p(B.ptr(d_b)), C.c_void_p(B.ptr(d_o)), len(raw), len(blob), max([len(s) for s in raw] + [0]), bos, eos, rev,
                              float(dropout), C.byref(ni), C.byref(ms), err, _lib.ERRLEN)
    assert rc == 0, err.value
    return D.encode_fetch(core, len(raw), ni.value)


def same(core, B, sents, bos=0, eos=0, rev=0, what="", fmt=None):
    """device == host path (bytes and offsets), pending ids == yttm_encode_device's; fmt = (vocab, alphabet, unk): also == format_ids of the
    pending ids (valid UTF-8 sentences only).  Returns (lines, ids per sentence)."""
    want = host_text(core, sents, bos, eos, rev)
    got = dev_subword(core, B, sents, bos, eos, rev)
    assert got[:2] == want[:2], (what, got[:2], want[:2])
    if want[0] != 0:
        return None, None
    assert got[3].tolist() == want[3].tolist(), what
    assert got[2] == want[2], what
    ids, ioff = got[4], got[5]
    w_ids, w_off = dev_ids(core, B, sents, bos, eos, rev)
    assert ids.tolist() == w_ids.tolist() and ioff.tolist() == w_off.tolist(), what
    o, io = got[3].tolist(), ioff.tolist()
    lines = [got[2][o[i]:o[i + 1]] for i in range(len(sents))]
    rows = [ids[io[i]:io[i + 1]].tolist() for i in range(len(sents))]
    assert all(ln.endswith(b"\n") for ln in lines)
    if fmt is not None:
        vocab, alphabet, unk = fmt
        for s, ln, row in zip(sents, lines, rows):
            s = s if isinstance(s, str) else s.decode()
            assert ln == format_ids(s, row, vocab, alphabet, unk, rev), (what, s[:60])
    return lines, rows


def fmt_of(name):
    bpe = bpe_of(name)
    return bpe, (bpe.vocab(), alphabet_of(model_path(name)), model_args(name)["unk"] if os.path.sep not in name else None)


def all_flags(core, B, sents, what, fmt=None):
    out = {}
    for b, e, r in FLAGS:
        out[(b, e, r)] = same(core, B, sents, b, e, r, (what, b, e, r), fmt)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
def check_golden(B, name):
    """every golden model x the four flag sets, against the host path, the reference's own subword_000 lists and the formatter"""
    a = model_args(name)
    bpe, fmt = fmt_of(name)
    core = bpe.bpe_cython
    sents = golden_sentences(name)
    want = json.load(open(os.path.join(G, f"encode_{name}.json")))["subword_000"]
    for b, e, r in FLAGS:
        if (b and a["bos"] == -1) or (e and a["eos"] == -1):  # the host's error, same code and message
            rc, msg = dev_subword(core, B, sents, b, e, r)[:2]
            assert (rc, msg) == (1, BOS_MSG) and (rc, msg) == host_text(core, sents, b, e, r)[:2]
            continue
        lines, _ = same(core, B, sents, b, e, r, (name, b, e, r), fmt)
        if (b, e, r) == (0, 0, 0):
            assert len(want) == len(lines)
            assert lines == [("".join(p + " " for p in row) + "\n").encode() for row in want], name


def single_id_words(bpe, k=6):
    """words that encode to exactly one id, of different lengths"""
    out = []
    for i, piece in enumerate(bpe.vocab()):
        if piece.startswith("▁") and len(piece) > 1 and "<" not in piece and bpe.encode([piece[1:]])[0] == [i]:
            out.append(piece[1:])
    out.sort(key=len)
    assert len(out) >= k
    return out[::max(1, len(out) // k)][:k]


def check_lengths(B, name="readme_small"):
    """sentences of exactly 0, 1, 2, 63, 64, 65, 511, 512, 513 and 5000 ids; empty and all-space sentences; an empty batch; a batch of one"""
    bpe, fmt = fmt_of(name)
    core = bpe.bpe_cython
    words = single_id_words(bpe)
    sents = [" ".join(words[j % len(words)] for j in range(n)) for n in D.LENGTHS]
    sents += ["", " ", " \t \n ", "▁▁ ▁"]
    for key, (lines, rows) in all_flags(core, B, sents, "lengths", fmt).items():
        extra = key[0] + key[1]
        assert [len(r) - extra for r in rows[:len(D.LENGTHS)]] == list(D.LENGTHS)
        ends = ([b"<BOS>"] if key[0] else []) + ([b"<EOS>"] if key[1] else [])
        assert lines[len(D.LENGTHS):] == [b"".join(p + b" " for p in (ends[::-1] if key[2] else ends)) + b"\n"] * 4
    lines, rows = same(core, B, sents, 0, 0, 0, "lengths")
    assert lines[0] == b"\n" and rows[0] == []
    for b, e, r in FLAGS:
        assert same(core, B, [], b, e, r, "empty batch") == ([], [])
        for s in (sents[4], "", sents[9]):
            same(core, B, [s], b, e, r, "a batch of one", fmt)
    # an empty batch through null pointers, and its text by both exits
    L = _lib.load()
    ni, nt, ms, err = C.c_uint64(5), C.c_uint64(5), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    assert L.yttm_subword_device(core._h, None, None, 0, 0, 0, 0, 0, 0, 0.0, C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 0
    assert (ni.value, nt.value) == (0, 0)
    off = np.full(1, 9, np.uint64)
    assert L.yttm_decode_fetch(core._h, None, off.ctypes.data_as(_lib.u64p), 0, err, _lib.ERRLEN) == 0 and off[0] == 0


def line_of_bytes(words, target):
    """a sentence of single-id words whose SUBWORD line holds exactly `target` bytes in front of its newline ("▁" + word + " " per word)"""
    cost = {len(w.encode()) + 4: w for w in words}
    best = {0: []}  # bytes -> words
    for t in range(1, target + 1):
        for c, w in cost.items():
            if t - c in best:
                best[t] = best[t - c] + [w]
                break
    assert target in best, (target, sorted(cost))
    return " ".join(best[target])


def check_full_tile(B, name="readme_small"):
    """sentences whose pieces and spaces fill the write pass's 2048-byte staging tile to its last byte, one short of it and one past it, each alone
    in its group and behind a first 16-byte unit shared with the sentence before: the newline behind them has no room unless the tile is flushed first"""
    bpe, fmt = fmt_of(name)
    core = bpe.bpe_cython
    words = single_id_words(bpe)
    tile, sents, cursor = 2048, [], 0
    for delta in (0, 0, -1, 1, 0, -17, 0):
        body = tile - cursor % 16 + delta  # (the tile holds the cursor's unit from its start)
        sents.append(line_of_bytes(words, body))
        cursor += body + 1
    for b, e, r in ((0, 0, 0), (0, 0, 1)):
        lines, rows = same(core, B, sents, b, e, r, ("full tile", b, e, r), fmt)
        assert [len(ln) for ln in lines] == [len(host_text(core, [s])[2]) for s in sents]
    lines, _ = same(core, B, sents, 0, 0, 0, "full tile")
    assert len(lines[0]) == tile + 1 and len(lines[1]) == tile - 1 + 1 and all(len(r) > 256 for r in _)


def unknown_chars(alphabet):
    u = {1: "Z", 2: "é", 3: "中", 4: "😀"}
    assert all(ord(c) not in alphabet and len(c.encode()) == n for n, c in u.items())
    return u


def valid_run_sentences(alphabet):
    """every sentence has at least one unknown run; valid UTF-8"""
    u = unknown_chars(alphabet)
    a, b = "a", "b"
    assert ord(a) in alphabet and ord(b) in alphabet
    s = ["ab Z ba", "Z", "中中中", u[4], "é中😀Z", "abZba", "Zab", "abZ", "a Z", "Z a", "ZZ ab éé"]
    s += [" ".join(u[1 + j % 4] * (1 + j % 3) for j in range(n)) for n in (64, 65, 127, 128, 129, 300)]       # many runs: more than a step, more than the directory
    s += [" ".join(("ab" + u[1 + j % 4]) if j % 2 else (u[1 + j % 4] + "ba") for j in range(140))]           # runs beside known chars, 140 of them
    s += [u[n] * 3 + " ab" for n in (1, 2, 3, 4)]
    for start in (61, 62, 63, 64, 65):                                                                          # a run that starts here and crosses the 64-byte step
        for n in (1, 2, 3, 4):
            s.append(("ab " * 30)[:start - 1] + " " + u[n] * 5 + " ab")
            s.append(("ab" * 40)[:start] + u[n] * 2)                                                            # ... without a space in front
    s += [u[2] * 1500, u[3] * 1000 + " ab " + u[4] * 750, "ab" + u[1] * 3000 + "ba", (u[2] + u[1] + u[4] + u[3]) * 400]  # longer than the staging tile
    s += [u[1] + sp + u[2] + sp + "ab" + sp + u[3] for sp in ("▁", "\t", "\r", "\v", "\f", "\n", " ▁ ")]
    s += ["Z▁Z\tZ\rZ\vZ\fZ", "▁Z▁"]
    s += [(u[3] + " ") * 70 + "ab " * 200 + (u[4] + "b ") * 70]                                                 # a long sentence: runs in its first and last steps
    return s


def invalid_run_sentences():
    """invalid bytes inside a run and at either end: dropped, and they do not end the run"""
    bad = [b"\x80", b"\xbf\x80", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf8\x88\x80\x80\x80", b"\xff", b"\xfe\xfe", b"\xf4\x90\x80\x80", b"\xe4\xb8"]
    s = []
    for x in bad:
        s += [x + b"ZZ", b"ZZ" + x, b"Z" + x + b"Z", b"ab " + x + b"Z" + x + b" ab", b"a" + x + b"Z", b"Z" + x + b"a", "中".encode() + x + "é".encode(),
              b"ab " * 20 + b"Z" * 3 + x + b"Z" * 3, x + "😀".encode() + x + x + b"Z b"]
    s += [b"ZZ\xc3", b"ab Z\xe4\xb8", b"Z\xf0\x9f\x98", b"Z ab\xc3"]                                              # a truncated lead at the sentence's end
    s += [b"Z" + x for x in bad] + [(b"Z" * 50 + x) * 60 for x in bad[:4]] + [("中".encode() + b"\x80") * 1100]  # ... in runs longer than the tile
    s += [b"ab " * 21 + x + b"ZZ" for x in bad]                                                                 # at the 64-byte step
    return s


def python_runs(raw, alphabet):
    """unknown runs of a byte string that may hold invalid UTF-8: code points as the reference's decoder keeps them"""
    i, n, runs, cur = 0, len(raw), [], 0
    while i < n:
        b0 = raw[i]
        ln = 1 if b0 < 0x80 else 2 if b0 >> 5 == 6 else 3 if b0 >> 4 == 14 else 4 if b0 >> 3 == 30 else 0
        cp = None
        if ln and i + ln <= n and all(raw[i + j] >> 6 == 2 for j in range(1, ln)):
            try:
                ch = raw[i:i + ln].decode()
                cp = ord(ch) if len(ch) == 1 else None
            except UnicodeDecodeError:
                cp = None
        if cp is None:
            i += 1
            continue
        i += ln
        if not is_space(cp) and cp not in alphabet:
            cur += 1
        else:
            runs.append(cur)
            cur = 0
    runs.append(cur)
    return sum(1 for r in runs if r)


def check_unknown_runs(B, name="readme_small"):
    bpe, fmt = fmt_of(name)
    core = bpe.bpe_cython
    alphabet, unk = fmt[1], fmt[2]
    valid = valid_run_sentences(alphabet)
    for key, (lines, rows) in all_flags(core, B, valid, "unknown runs", fmt).items():
        seen = [row.count(unk) for row in rows]
        assert seen == [len(runs_of(s, alphabet)) for s in valid] and min(seen) >= 1 and max(seen) >= 300, key
    bad = invalid_run_sentences()
    for key, (lines, rows) in all_flags(core, B, bad, "runs with invalid bytes").items():
        seen = [row.count(unk) for row in rows]
        assert seen == [python_runs(s, alphabet) for s in bad] and min(seen) >= 1, key
    # the other golden alphabets (Cyrillic, kana and kanji, coverage < 1: chars of the training text itself are unknown)
    for other in ("manual_ru", "manual_ja", "mix_cov", "readme_rename", "nopad"):
        b2, f2 = fmt_of(other)
        assert ord("Ω") not in f2[1]
        sents = valid_run_sentences(f2[1]) if other in ("readme_rename", "nopad") else \
            [s + " Ω " + s[::-1] + "Ω" for s in golden_sentences(other)[:40]] + ["Ω", "ΩΩ 中"]
        for b, e, r in FLAGS:
            if (b and model_args(other)["bos"] == -1) or (e and model_args(other)["eos"] == -1):
                continue
            lines, rows = same(b2.bpe_cython, B, sents, b, e, r, (other, b, e, r), f2)
            assert sum(row.count(f2[2]) for row in rows) >= len(sents) // 2


def long_model(tmp_path):
    """a model in which one piece is a word of 2300 chars, longer than a wavefront's 2 KB staging tile: (bpe, word, fmt)"""
    import youtokentome_amd as yttm
    rng = random.Random(4)
    word = "".join(rng.choice("abcdefgh") for _ in range(2300))
    corpus, model = str(tmp_path / "long.txt"), str(tmp_path / "long.model")
    open(corpus, "w").write((word + " xy ") * 6 + "ab cd\n")
    yttm.BPE.train(corpus, model, 4 + 11 + 2400, 1.0, 1, 0, 1, 2, 3)
    bpe = yttm.BPE(model)
    assert bpe.encode([word])[0] == [bpe.bpe_cython.subword_to_id("▁" + word)], "the long word did not become one piece"
    return bpe, word, (bpe.vocab(), alphabet_of(model), 1)


def check_long_piece(B, tmp_path):
    """a piece longer than the staging tile streams through it"""
    bpe, word, fmt = long_model(tmp_path)
    sents = [word, "xy " + word + " " + word + " ab", word + "Z", "Z" * 2500 + " " + word, "", word[:1200], "ab " * 50 + word + " Z " + word]
    for key, (lines, rows) in all_flags(bpe.bpe_cython, B, sents, "long piece", fmt).items():
        assert ("▁" + word).encode() + b" " in lines[0]
    check_long_neighbours(B, bpe, word, fmt)


def check_long_neighbours(B, bpe, word, fmt, flags=FLAGS):
    """Long pieces and long runs while the OTHER wavefronts of the workgroup have staged data of their own: sentences of more than 256 ids on
    average make every sentence a group of its own (k_subword.h sub_group), so consecutive sentences sit on the four waves of one workgroup,
    whose staging tiles and run directories are neighbours in LDS.  A wave that writes outside its tile spoils a neighbour's text.  The long
    piece directly behind a long run (no short piece in between), behind a short run, in front of one, and twice in a row."""
    filler = "xy " * 3000
    shapes = ["Z" * 2500 + " " + word + " xy" * 300, "Z" * 700 + " " + word + " " + word + " xy" * 300, "xy Z " + word + " " + "é" * 900 + " " + word + "Z" * 1000,
              word + " " + "中" * 500 + " " + word + " " + "Z" * 70 + " " + word + " xy" * 300]
    sents = []
    for k, sh in enumerate(shapes * 2):  # each shape on every wave of a workgroup, the other three staging filler
        row = [filler] * 4
        row[(k + k // 4) % 4] = sh
        sents += row
    for b, e, r in flags:
        lines, rows = same(bpe.bpe_cython, B, sents, b, e, r, ("long piece beside busy waves", b, e, r), fmt)
        assert sum(len(row) for row in rows) > 256 * len(rows), "the sentences would share groups"


def check_groups(B, name="readme_small"):
    """many short sentences: a group's first and last 16-byte units are shared with its neighbours (the guard bytes behind the text are checked by
    both exits in every case of this file)"""
    bpe, fmt = fmt_of(name)
    core = bpe.bpe_cython
    rng = random.Random(3)
    pool = ["", "a", "ab", "Z", "ab Z", "é", "abcd ab", " ", "中 a", "b" * 9, "abZ中 d"]
    for n in (1, 2, 3, 64, 700, 5000):
        sents = [rng.choice(pool) for _ in range(n)]
        for b, e, r in ((0, 0, 0), (1, 1, 1)):
            same(core, B, sents, b, e, r, ("groups", n), fmt if n <= 700 else None)
    same(core, B, [""] * 333 + ["Z"] + [""] * 200, 0, 0, 0, "empty sentences around", fmt)


def check_errors(B):
    """bos / eos on a model trained without them: the host's error, and nothing is pending afterwards that was not pending before"""
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    core = bpe_of("nopad").bpe_cython
    sents = ["ab Z cd", "", "abcd"]
    # a fresh encoder: nothing is pending after the failure
    for b, e in ((1, 0), (0, 1), (1, 1)):
        for r in (0, 1):
            rc, msg = dev_subword(core, B, sents, b, e, r)[:2]
            assert (rc, msg) == host_text(core, sents, b, e, r)[:2] and rc == 1 and "token. Model was trained without it." in msg
    assert L.yttm_decode_fetch(core._h, None, None, 3, err, _lib.ERRLEN) != 0
    assert L.yttm_encode_fetch(core._h, None, None, 3, err, _lib.ERRLEN) != 0
    # a good call, then failures: its ids and its text are still there
    good = dev_subword(core, B, sents)
    assert good[0] == 0
    assert dev_subword(core, B, sents + ["x"], 1, 1, 0)[0] == 1
    P = K.Placed(B, b"ab\nZ\n")
    nl, ni, nt, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
    assert L.yttm_subword_text_device(core._h, C.c_void_p(P.ptr), 5, 0, 1, 0, 0.0, C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 1
    assert err.value.decode() == "Can't add <EOS> token. Model was trained without it." and (nl.value, ni.value, nt.value) == (0, 0, 0)
    text, off = D._take_result(core, B, 3, len(good[2]))
    ids, ioff = D.encode_fetch(core, 3, len(good[4]))
    assert (text, off.tolist(), ids.tolist(), ioff.tolist()) == (good[2], good[3].tolist(), good[4].tolist(), good[5].tolist())
    # the text slot is the decode's: a decode replaces the text, not the ids; a subword call replaces a decode result
    core = bpe_of("readme_small").bpe_cython
    good = dev_subword(core, B, ["ab Z", "cd"])
    dec = D.dev_decode(core, B, np.array([5, 6, 7], np.int32), np.array([0, 3], np.uint64))
    assert dec[0] == 0 and L.yttm_decode_fetch(core._h, None, None, 2, err, _lib.ERRLEN) != 0
    ids, ioff = D.encode_fetch(core, 2, len(good[4]))
    assert ids.tolist() == good[4].tolist()
    again = dev_subword(core, B, ["ab Z", "cd"])
    assert again[2] == good[2] and L.yttm_decode_fetch(core._h, None, None, 1, err, _lib.ERRLEN) != 0


def check_dropout(B, name="readme_small", ps=(0.1, 1.0)):
    """with the salt pinned: text == format_ids(the pending ids), and the pending ids are those of yttm_encode_device on an encoder in the same state"""
    alphabet = alphabet_of(model_path(name))
    unk = model_args(name)["unk"]
    sents = golden_sentences(name)[:60] + [s for s in valid_run_sentences(alphabet) if len(s) < 700]
    base = None
    for p in ps:
        for b, e, r in FLAGS:
            with DC.env():
                bpe = bpe_of(name)
                got = dev_subword(bpe.bpe_cython, B, sents, b, e, r, p)
                w_ids, w_off = dev_ids(bpe_of(name).bpe_cython, B, sents, b, e, r, p)
            assert got[0] == 0
            assert got[4].tolist() == w_ids.tolist() and got[5].tolist() == w_off.tolist(), (p, b, e, r)
            o, io, vocab = got[3].tolist(), got[5].tolist(), bpe.vocab()
            for i, s in enumerate(sents):
                assert got[2][o[i]:o[i + 1]] == format_ids(s, got[4][io[i]:io[i + 1]].tolist(), vocab, alphabet, unk, r), (p, b, e, r, i)
            if (b, e, r) == (0, 0, 0):
                if base is None:
                    base = dev_subword(bpe.bpe_cython, B, sents)[4].tolist()
                assert got[4].tolist() != base, "the dropout changed nothing"
            if p == 1.0:  # no merge at all: deterministic, the host path agrees
                assert got[2] == host_text(bpe.bpe_cython, sents, b, e, r, 1.0)[2]


# ---- unsplit text and files ---------------------------------------------------------------------------------------------------------------
def texts(name="readme_small"):
    data, _ = K.golden(name)
    rng = random.Random(6)
    mixed = b"".join(rng.choice([b"ab cd", b"", b"Z", "é中 ab".encode(), b"ab\r", b"\xc3", b"a\x80Z b", b"abcd " * 30, b" "]) + b"\n" for _ in range(400))
    return [data, data[:-1], b"", b"\n", b"\n\n\n", b"Z", b"ab Z\r\ncd\r\n\r\n", b"no newline Z", mixed, mixed + b"Z" * 5000 + b"\nab" + b" cd" * 900, b"x\n" * 300 + "中".encode() * 2000 + b"\nz"]


def dev_subword_text(core, B, data, bos=0, eos=0, rev=0, dropout=0.0, align=0):
    L = _lib.load()
    P = K.Placed(B, data, align)
    nl, ni, nt, ms, err = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_subword_text_device(core._h, C.c_void_p(P.ptr), len(data), bos, eos, rev, float(dropout), C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms),
                                    err, _lib.ERRLEN)
    assert rc == 0, err.value
    assert P.intact(), "the text or its guard bytes were written"
    text, line_off = D._take_result(core, B, nl.value, nt.value)
    ids, ioff = D.encode_fetch(core, nl.value, ni.value)
    return text, line_off, ids, ioff, core.fetch_lines(nl.value)


def check_text(B, name="readme_small"):
    """yttm_subword_text_device == the host path on the lines without their newlines; the lines' offsets are pending as after yttm_lines_device"""
    core = bpe_of(name).bpe_cython
    for k, data in enumerate(texts(name)):
        lines = K.py_split(data)
        for b, e, r in FLAGS:
            want = host_text(core, lines, b, e, r)
            for align in ((0, 5) if k < 3 else (3,)):
                text, line_off, ids, ioff, lo = dev_subword_text(core, B, data, b, e, r, align=align)
                assert text == want[2] and line_off.tolist() == want[3].tolist(), (k, b, e, r)
                assert lo.tolist() == K.py_offsets(data).tolist()
                w_ids, w_off = K.host_encode(core, data, b, e, r)
                assert ids.tolist() == w_ids.tolist() and ioff.tolist() == w_off.tolist()


def ref_subword_file(model, path, b, e, r):
    """the compiled reference's `encode --output_type subword` of the file, or None where it is not built"""
    if not refbin.available("prod"):
        return None
    p = subprocess.run([refbin.path("prod"), "encode", model, path, "-", "1", str(b), str(e), str(r), "0.0", "subword"], capture_output=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def check_file(tmp_path, name="readme_small", use_ref=False):
    """yttm_encode_file_subword: the same file whatever the piece size and the transfer chunk, equal to the host path's text (and to the compiled
    reference's output of the same file where it is present)"""
    model = model_path(name)
    a = model_args(name)
    for k, data in enumerate(texts(name)):
        path = str(tmp_path / f"in{k}.txt")
        open(path, "wb").write(data)
        lines = K.py_split(data)
        longest = max([len(ln) for ln in lines] + [0]) + 1
        for b, e, r in FLAGS if k in (0, 9) else ((0, 0, 0), (1, 1, 1)):
            if (b and a["bos"] == -1) or (e and a["eos"] == -1):
                continue
            core = bpe_of(name).bpe_cython
            want = host_text(core, lines, b, e, r)
            files = []
            for j, (chunk, io_kb) in enumerate(((None, None), (max(len(data) // 8, 1), 1), (longest - 2 if longest > 2 else 1, 1), (1, None), (len(data) + 9, 1))):
                out = str(tmp_path / f"out{k}_{j}.txt")
                with DC.env(**({"YTTM_IO_CHUNK_KB": io_kb} if io_kb else {})):
                    c2 = bpe_of(name).bpe_cython
                    rep = c2.encode_file_subword(path, out, b, e, r, 0.0, chunk, report=True)
                got = open(out, "rb").read()
                files.append(got)
                assert got == want[2], (k, b, e, r, chunk)
                assert (rep["lines"], rep["text_bytes"], rep["bytes"]) == (len(lines), len(got), len(data))
                assert {"pieces", "piece_bytes", "ids", "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_format",
                        "seconds_download_write"} <= set(rep)
                if j == 1 and k == 0:
                    assert rep["pieces"] >= 5, rep
                if j in (0, 4) and data:
                    assert rep["pieces"] == 1, rep
                if j == 0:
                    assert c2.encode_file_subword(path, out, b, e, r, 0.0, chunk) == (len(lines), rep["ids"], len(got))
            assert len(set(files)) == 1
            if use_ref and b"\r" not in data and all(ln.decode(errors="ignore").encode() == ln for ln in lines):
                ref = ref_subword_file(model, path, b, e, r)
                assert ref is None or ref == want[2], (k, b, e, r)


def check_file_errors(tmp_path, name="readme_small"):
    import pytest
    import youtokentome_amd as yttm
    bpe = bpe_of(name)
    path = str(tmp_path / "in.txt")
    open(path, "wb").write(b"ab Z\ncd\n")
    with pytest.raises(ValueError, match="Failed to open file: .*no_such_file"):
        bpe.encode_file(str(tmp_path / "no_such_file.txt"), str(tmp_path / "o.txt"), output_type=yttm.OutputType.SUBWORD)
    with pytest.raises(ValueError, match="Failed to open file for writing: .*no_such_dir"):
        bpe.encode_file(path, str(tmp_path / "no_such_dir" / "o.txt"), output_type=yttm.OutputType.SUBWORD)
    L, err = _lib.load(), C.create_string_buffer(_lib.ERRLEN)
    z = C.c_uint64()
    for src, dst in ((str(tmp_path / "no_such_file.txt"), str(tmp_path / "o.txt")), (path, str(tmp_path / "no_such_dir" / "o.txt")), (str(tmp_path), str(tmp_path / "o.txt"))):
        assert L.yttm_encode_file_subword(bpe.bpe_cython._h, os.fsencode(src), os.fsencode(dst), 0, 0, 0, 0.0, 0, C.byref(z), C.byref(z), C.byref(z), None, 0,
                                          err, _lib.ERRLEN) == 1, err.value
    # the input itself as the output, under its own name or another: refused before anything is truncated; no output path at all: code 1 too
    os.link(path, str(tmp_path / "same.txt"))
    os.symlink(path, str(tmp_path / "link.txt"))
    for dst in (path, str(tmp_path / "same.txt"), str(tmp_path / "link.txt")):
        with pytest.raises(ValueError, match="Failed to open file for writing: .* is the input file"):
            bpe.encode_file(path, dst, output_type=yttm.OutputType.SUBWORD)
        assert open(path, "rb").read() == b"ab Z\ncd\n"
    assert L.yttm_encode_file_subword(bpe.bpe_cython._h, os.fsencode(path), None, 0, 0, 0, 0.0, 0, C.byref(z), C.byref(z), C.byref(z), None, 0, err, _lib.ERRLEN) == 1
    assert L.yttm_encode_file_subword(bpe.bpe_cython._h, os.fsencode(path), b"", 0, 0, 0, 0.0, 0, C.byref(z), C.byref(z), C.byref(z), None, 0, err, _lib.ERRLEN) == 1
    # an existing, longer output file is replaced, not overwritten in place
    open(str(tmp_path / "old.txt"), "wb").write(b"x" * 1000)
    bpe.encode_file(path, str(tmp_path / "old.txt"), output_type=yttm.OutputType.SUBWORD)
    assert open(str(tmp_path / "old.txt"), "rb").read() == host_text(bpe.bpe_cython, [b"ab Z", b"cd"])[2]
    os.symlink("/dev/full", str(tmp_path / "full.txt"))
    with pytest.raises(ValueError, match="Failed to write file: .*full.txt"):
        bpe.encode_file(path, str(tmp_path / "full.txt"), output_type=yttm.OutputType.SUBWORD)
    with pytest.raises(ValueError, match="needs out"):
        bpe.encode_file(path, output_type=yttm.OutputType.SUBWORD)
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_file(path, str(tmp_path / "o.txt"), dropout_prob=2, output_type=yttm.OutputType.SUBWORD)
    with pytest.raises(ValueError, match=BOS_MSG):
        bpe_of("nopad").encode_file(path, str(tmp_path / "o.txt"), bos=True, output_type=yttm.OutputType.SUBWORD)
    # the lanes are as good as before
    assert bpe.encode_file(path, str(tmp_path / "o.txt"), output_type=yttm.OutputType.SUBWORD)[0] == 2
    assert open(str(tmp_path / "o.txt"), "rb").read() == host_text(bpe.bpe_cython, [b"ab Z", b"cd"])[2]
    # the ID default is what it was
    ids, off = bpe.encode_file(path)
    w_ids, w_off = K.host_encode(bpe.bpe_cython, b"ab Z\ncd\n")
    assert ids.tolist() == w_ids.tolist() and off.tolist() == w_off.tolist()
    assert bpe.encode_file(path, str(tmp_path / "pre")) == (2, len(w_ids))


def check_cli(tmp_path, name="readme_small"):
    """`yttm encode_file --output_type subword` writes the bytes `yttm encode --output_type subword` prints; the id default writes its two files"""
    core = bpe_of(name).bpe_cython
    data = texts(name)[9]
    path, model = str(tmp_path / "in.txt"), model_path(name)
    open(path, "wb").write(data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]
    for extra, (b, e, r) in (([], (0, 0, 0)), (["--bos", "--eos", "--reverse"], (1, 1, 1))):
        out = str(tmp_path / ("cli" + "".join(extra) + ".txt"))
        p = subprocess.run(cli + ["encode_file", f"--model={model}", f"--input={path}", f"--output={out}", "--output_type=subword"] + extra, capture_output=True, env=env)
        assert p.returncode == 0, p.stderr.decode()
        q = subprocess.run(cli + ["encode", f"--model={model}", "--output_type=subword"] + extra, stdin=open(path, "rb"), capture_output=True, env=env)
        assert q.returncode == 0, q.stderr.decode()
        assert open(out, "rb").read() == q.stdout
        assert q.stdout == host_text(core, K.py_split(data), b, e, r)[2]
    prefix = str(tmp_path / "ids")
    p = subprocess.run(cli + ["encode_file", f"--model={model}", f"--input={path}", f"--output={prefix}"], capture_output=True, env=env)
    assert p.returncode == 0, p.stderr.decode()
    w_ids, w_off = K.host_encode(core, data)
    f_ids, f_off = K.read_out(prefix)
    assert f_ids.tolist() == w_ids.tolist() and f_off.tolist() == w_off.tolist()


def check_large(B, name="zipf", n=50_000, width=128, frac=0.01):
    """one larger pass: n sentences of `width` chars of Zipf text, about 1 % of the chars outside the alphabet, against the host path"""
    import gen
    bpe, fmt = fmt_of(name)
    u = unknown_chars(fmt[1])
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=23, vocab=20000).replace(b"\n", b" ")[:n * width]
    assert len(raw) == n * width
    cps = np.frombuffer(raw, np.uint8).astype("<u4")
    rng = np.random.default_rng(5)
    hit = rng.random(len(cps)) < frac
    cps[hit] = rng.choice(np.array([ord(c) for c in u.values()], "<u4"), size=int(hit.sum()))
    text = cps.tobytes().decode("utf-32-le")
    sents = [text[i * width:(i + 1) * width] for i in range(n)]
    for b, e, r in ((0, 0, 0), (1, 1, 1)):
        lines, rows = same(bpe.bpe_cython, B, sents, b, e, r, ("large", b, e, r))
        with_unk = sum(1 for row in rows if fmt[2] in row)
        assert n * 0.5 < with_unk < n * 0.9, with_unk
