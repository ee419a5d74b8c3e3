"""Checks of the byte spans made on the device (yttm_spans_device, yttm_spans_text_device, yttm_spans_fetch / _copy_device / _copy_padded,
yttm_encode_as_ids_spans, BPE.encode_with_spans), shared by the emulator tests (test_spans_device.py, test_spans_device_sched.py: numpy arrays
are "device" memory there) and the MI355X tests (test_gpu_spans.py: torch tensors).

Two checkers, neither the code under test, and they share no code with each other:
  1. rule_spans: the rule of include/yttm_mi355x.h ("Byte spans") written out in Python -- units of the text, units per id, prefix sums --,
     compared exactly;
  2. check_properties: what any correct alignment satisfies, from the pieces' own text: spans in forward order neither decrease nor overlap;
     the valid chars inside a non-unk token's span are its piece without "▁"; an unk span starts and ends on a valid char outside the
     alphabet; between two non-empty spans lie only white space and invalid bytes.
The ids beside the spans are those of yttm_encode_as_ids / yttm_encode_device with the same arguments (dropout_prob == 0)."""
import ctypes as C
import os
import random

import numpy as np

import decode_checks as D
import lines_checks as K
from decode_checks import G, NumpyBuf, TorchBuf, golden_names, golden_sentences, model_args  # noqa: F401  (the buffers are re-exported)
from youtokentome_amd import _lib

FLAGS = ((0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1))
BOS_MSG = "Can't add <BOS> token. Model was trained without it."
EOS_MSG = "Can't add <EOS> token. Model was trained without it."
SPECIAL = ("<PAD>", "<BOS>", "<EOS>")


def model_path(name):
    return name if os.path.sep in name else os.path.join(G, f"train_{name}.model")


def all_models():
    """every model under tests/golden"""
    return sorted(p[len("train_"):-len(".model")] for p in os.listdir(G) if p.startswith("train_") and p.endswith(".model"))


def sentences_of(name, most=60):
    """the golden sentences of a model, or lines of its training text"""
    if os.path.exists(os.path.join(G, f"encode_{name}.lines")):
        return golden_sentences(name)[:most]
    lines = [ln[:400] for ln in open(os.path.join(G, f"train_{name}.txt"), "rb").read().decode(errors="ignore").split("\n") if ln]
    return lines[:most // 2] + lines[-(most // 2):]


def to_bytes(sents):
    return [s.encode() if isinstance(s, str) else bytes(s) for s in sents]


class Model:
    """what the checkers need of a model: the pieces, the alphabet (the model file's char section), unk_id"""

    def __init__(self, name):
        import youtokentome_amd as yttm
        self.path = model_path(name)
        self.bpe = yttm.BPE(self.path)
        self.core = self.bpe.bpe_cython
        self.vocab = self.bpe.vocab()
        tok = open(self.path).read().split()
        self.alphabet = {int(tok[2 + 2 * i]) for i in range(int(tok[0]))}
        self.unk = self.vocab.index("<UNK>")
        self.text_of = ["" if p in SPECIAL else p.replace("▁", "") for p in self.vocab]  # (the property check: what a piece shows of the text)
        self.has_bos, self.has_eos = "<BOS>" in self.vocab, "<EOS>" in self.vocab

    def flags(self):
        return [f for f in FLAGS if (not f[0] or self.has_bos) and (not f[1] or self.has_eos)]


_models = {}


def model(name):
    if name not in _models:
        _models[name] = Model(name)
    return _models[name]


# ---- checker 1: the rule ------------------------------------------------------------------------------------------------------------------
def is_space(cp):
    return cp == 0x2581 or cp == 32 or 9 <= cp <= 13


def valid_chars(raw):
    """(first byte, bytes, code point) of every char the encoder's left-to-right decode keeps; an invalid byte is skipped one at a time"""
    i, n, out = 0, len(raw), []
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
        out.append((i, ln, cp))
        i += ln
    return out


def units_of(raw, alphabet):
    """[start, end) of every unit"""
    units, run_open = [], False
    for i, ln, cp in valid_chars(raw):
        if is_space(cp):
            run_open = False
        elif cp in alphabet:
            units.append([i, i + ln])
            run_open = False
        elif run_open:
            units[-1][1] = i + ln
        else:
            units.append([i, i + ln])
            run_open = True
    return units


def units_per_id(M, t):
    if t == M.unk:
        return 1
    piece = M.vocab[t]
    return 0 if piece in SPECIAL else sum(1 for ch in piece if ch != "▁")


def rule_spans(M, raw, ids, rev):
    """the spans of the stored ids of one sentence"""
    units = units_of(raw, M.alphabet)
    fwd = ids[::-1] if rev else ids
    out, a = [], 0
    for t in fwd:
        u = units_per_id(M, t)
        if u:
            assert a + u <= len(units), "more units in the ids than in the text"
            out.append((units[a][0], units[a + u - 1][1]))
        else:
            p = units[a][0] if a < len(units) else (units[-1][1] if units else 0)
            out.append((p, p))
        a += u
    assert a == len(units), "the ids cover %d units, the text has %d" % (a, len(units))
    return out[::-1] if rev else out


# ---- checker 2: properties ------------------------------------------------------------------------------------------------------------------
WHITE = " \t\n\r\v\f▁"  # what separates words: isspace() in the C locale, and U+2581


def check_properties(M, raw, ids, spans, rev, what=""):
    unk, alphabet, text_of = M.unk, M.alphabet, M.text_of
    if rev:
        ids, spans = ids[::-1], spans[::-1]
    assert len(ids) == len(spans), what
    prev_end, gap_from, size = 0, 0, len(raw)
    for t, (a, b) in zip(ids, spans):
        assert prev_end <= a <= b <= size, (what, "order", a, b, prev_end)
        prev_end = b
        if a == b:
            assert t != unk and text_of[t] == "", (what, "a token with text has an empty span", M.vocab[t])
            continue
        inside = raw[a:b].decode(errors="ignore")
        if t != unk:
            assert inside == text_of[t], (what, M.vocab[t], inside)
        else:
            first, last = inside[0], inside[-1]
            for ch in (first, last):
                assert ord(ch) not in alphabet and ch not in WHITE, (what, "unk span on a known char", ch)
            assert raw[a:a + len(first.encode())] == first.encode() and raw[b - len(last.encode()):b] == last.encode(), (what, "unk span off a char")
        if a > gap_from:
            between = raw[gap_from:a].decode(errors="ignore")
            assert all(ch in WHITE for ch in between), (what, "text between two spans", between)
        gap_from = b
    tail = raw[gap_from:].decode(errors="ignore")
    assert all(ch in WHITE for ch in tail), (what, "text behind the last span", tail)


# ---- the device path ------------------------------------------------------------------------------------------------------------------------
def host_ids(core, sents, bos=0, eos=0, rev=0):
    blob, off = K.pack(to_bytes(sents))
    return core.encode_packed(blob, off, bool(bos), bool(eos), bool(rev), 0.0)


def take_spans(core, B, n, n_ids):
    """the pending spans by both exits, which must agree; the bytes behind them stay"""
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    host = np.full((n_ids + 1, 2), 0x5A5A5A5A, np.uint32)
    assert L.yttm_spans_fetch(core._h, host.ctypes.data_as(_lib.u32p), n, err, _lib.ERRLEN) == 0, err.value
    dev = B.empty(2 * n_ids + 2, np.int32)
    assert L.yttm_spans_copy_device(core._h, C.c_void_p(B.ptr(dev)), n, err, _lib.ERRLEN) == 0, err.value
    got = B.get(dev).view(np.uint32).reshape(-1, 2)
    assert np.array_equal(got[:n_ids], host[:n_ids])
    assert host[n_ids].tolist() == [0x5A5A5A5A] * 2 and got[n_ids].view(np.int32).tolist() == [-7, -7], "written behind the spans"
    return host[:n_ids].astype(np.int64)


def dev_spans(core, B, sents, bos=0, eos=0, rev=0, dropout=0.0, align=None):
    """yttm_spans_device on bytes + offsets in device memory: (code, message, ids, ids_off, spans [n_ids, 2])"""
    L = _lib.load()
    raw = to_bytes(sents)
    blob, off = K.pack(raw)
    n = len(raw)
    if align is None:
        d_b = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8))
        p_b = B.ptr(d_b)
    else:
        P = K.Placed(B, blob, align)
        p_b = P.ptr
    d_o = B.put(off)
    ni, ms, err = C.c_uint64(77), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_spans_device(core._h, C.c_void_p(p_b), C.c_void_p(B.ptr(d_o)), n, len(blob), max([len(s) for s in raw] + [0]), bos, eos, rev, float(dropout),
                             C.byref(ni), C.byref(ms), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None, None
    assert align is None or P.intact(), "the text or its guard bytes were written"
    ids, ioff = D.encode_fetch(core, n, ni.value)
    return 0, "", ids, ioff, take_spans(core, B, n, ni.value)


def rows(a, off):
    o = [int(x) for x in off]
    a = a.tolist()
    return [a[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def check_batch(M, B, sents, bos=0, eos=0, rev=0, dropout=0.0, what="", align=None, rule=True):
    """both checkers on one call's own ids; without dropout the ids are the host path's.  Returns (ids, spans) per sentence."""
    rc, msg, ids, ioff, spans = dev_spans(M.core, B, sents, bos, eos, rev, dropout, align)
    assert rc == 0, (what, msg)
    if dropout == 0:
        w_ids, w_off = host_ids(M.core, sents, bos, eos, rev)
        assert np.array_equal(ids, w_ids) and np.array_equal(ioff, w_off), what
    id_rows, sp_rows = rows(ids, ioff), rows(spans, ioff)
    for k, (raw, r_ids, r_sp) in enumerate(zip(to_bytes(sents), id_rows, sp_rows)):
        r_sp = [tuple(p) for p in r_sp]
        if rule:
            assert r_sp == rule_spans(M, raw, r_ids, rev), (what, k, raw[:80], bos, eos, rev)
        check_properties(M, raw, r_ids, r_sp, rev, (what, k, raw[:80], bos, eos, rev))
    return id_rows, sp_rows


def all_flags(M, B, sents, what, **kw):
    return {f: check_batch(M, B, sents, *f, what=what, **kw) for f in M.flags()}


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def check_golden(B, name):
    """a golden model x the four flag sets; bos / eos on a model without them: the host's message and code"""
    M = model(name)
    sents = sentences_of(name)
    for b, e, r in FLAGS:
        if (b, e, r) in M.flags():
            id_rows, _ = check_batch(M, B, sents, b, e, r, what=name)
            assert sum(len(x) for x in id_rows) > len(sents)
        else:
            rc, msg = dev_spans(M.core, B, sents, b, e, r)[:2]
            assert (rc, msg) == (1, BOS_MSG if b and not M.has_bos else EOS_MSG)


def unknown_chars(alphabet):
    u = {1: "Z", 2: "é", 3: "中", 4: "😀"}
    assert all(ord(c) not in alphabet and len(c.encode()) == n for n, c in u.items())
    return u


BAD = [b"\x80", b"\xbf\x80", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf8\x88\x80\x80\x80", b"\xff", b"\xfe\xfe", b"\xf4\x90\x80\x80", b"\xe4\xb8"]


def mixed_sentences(M, n=120, seed=11):
    """golden sentences with unknown chars, tabs, U+2581 and invalid bytes thrown in"""
    rng = random.Random(seed)
    u = unknown_chars(M.alphabet)
    extra = [c.encode() for c in u.values()] + BAD + [b"\t", b"  ", "▁".encode(), b" \xff ", "中Z".encode()]
    out = []
    base = sentences_of("readme_small")
    for k in range(n):
        raw = bytearray(base[k % len(base)].encode()[:200])
        for _ in range(rng.randrange(0, 6)):
            at = rng.randrange(0, len(raw) + 1)
            raw[at:at] = rng.choice(extra)
        out.append(bytes(raw))
    return out


def check_dropout(B, name="readme_small", ps=(0.1, 1.0)):
    """alignment holds for any segmentation: both checkers on the call's own ids"""
    M = model(name)
    sents = sentences_of(name)[:40] + mixed_sentences(M, 60)
    base = None
    for p in ps:
        for f in M.flags():
            id_rows, _ = check_batch(M, B, sents, *f, dropout=p, what=("dropout", p))
            if f == (0, 0, 0):
                if base is None:
                    base = check_batch(M, B, sents, what="no dropout")[0]
                assert id_rows != base, "the dropout changed nothing"


def check_id0_quirk(B, tmp_path):
    """no special token owns id 0, U+2581 does: the encoder drops a word's unmerged leading U+2581"""
    import youtokentome_amd as yttm
    corpus, path = str(tmp_path / "q.txt"), str(tmp_path / "q.model")
    open(corpus, "w").write("ab abc abcd b c d bc cd a\n" * 20)
    yttm.BPE.train(corpus, path, 14, 1.0, 1, 5, 1, 2, 3)
    M = model(path)
    assert M.vocab[0] == "▁", M.vocab[:6]
    sents = ["ab cd", "a b c d", "Z", "ZZ 中", "Z a 中中 b", "d Z", " ", "", "abcd abcd", "▁a▁▁Z", "d" * 70, "Z " * 70, "a\xffZ\xff".encode("latin-1")]
    for p in (0.0, 1.0):
        for f, (id_rows, _) in all_flags(M, B, sents, "id 0 is U+2581", dropout=p).items():
            if p == 1.0 and f == (0, 0, 0):
                assert id_rows[1] == [M.vocab.index(c) for c in "abcd"], "the lone U+2581 of a word was expected to be dropped"


def check_step_boundaries(B):
    """every shift 0 .. 130 of a fixed tail against the 64-byte step: 1- to 4-byte chars, an unknown run, an invalid byte and a space run"""
    M = model("readme_small")
    u = unknown_chars(M.alphabet)
    tails = ["ab cd", u[1] * 3 + " ab", u[2] * 3 + "ab", "a" + u[3] * 2 + " b", u[4] * 2 + u[1], u[4] + " " + u[3] + "ab",
             b"a\xffb", b"Z\x80Z ab", b"Z\xe4\xb8 Z", "a    b", " \t▁ ab", b"a\xf0\x9f\x98 b"]
    sents = []
    for tail in tails:
        tail = tail.encode() if isinstance(tail, str) else tail
        for shift in range(131):
            sents.append(("ab " * 44)[:shift].encode() + tail)
            if shift % 3 == 0:
                sents.append(("Z" * 131)[:shift].encode() + tail)  # the open run reaches the boundary
    all_flags(M, B, sents, "step boundaries")
    check_batch(M, B, sents, dropout=1.0, what="step boundaries, no merges")
    for name, nbytes in (("manual_ru", 2), ("manual_ja", 3)):  # known chars of 2 and 3 bytes (a 4-byte char is in no golden alphabet)
        M2 = model(name)
        ch = min(chr(cp) for cp in M2.alphabet if len(chr(cp).encode()) == nbytes and chr(cp) not in WHITE)
        sents = [("a " * 66)[:shift] + ch * 3 + " " + ch + "Ω" + ch for shift in range(131)]
        for f in M2.flags():
            check_batch(M2, B, sents, *f, what=("step boundaries", name))


def check_large_sentences(B, tmp_path):
    """sentences of 0, 1, 63, 64, 65 and 5000 ids; a token of more than 64 chars and one of 2300; more than 64 tokens inside one text step"""
    import subword_checks as S
    M = model("readme_small")
    words = S.single_id_words(M.bpe)
    sents = [" ".join(words[j % len(words)] for j in range(n)) for n in (0, 1, 63, 64, 65, 5000)]
    for f, (id_rows, _) in all_flags(M, B, sents, "lengths").items():
        assert [len(r) - f[0] - f[1] for r in id_rows] == [0, 1, 63, 64, 65, 5000]
    dense = ["a b c d e a b c d e a b c d e a b c d e a b c d e a b c d e a b c d" * 3, "Z a " * 40]
    id_rows, _ = check_batch(M, B, dense, dropout=1.0, what="more than 64 tokens in a step")
    assert len(id_rows[0]) > 64 * 3 - 10
    bpe, word, _ = S.long_model(tmp_path)
    ML = model(bpe.model)
    assert len(word) == 2300
    sents = [word, "xy " + word + " " + word + " ab", word + "Z", "Z" * 2500 + " " + word, "", word[:1200], "ab " * 50 + word + " Z " + word, word[:70]]
    for f, (id_rows, sp_rows) in all_flags(ML, B, sents, "long piece").items():
        assert max(b - a for a, b in sp_rows[0]) == 2300
    check_batch(ML, B, sents, dropout=0.1, what="long piece, dropout")


def check_spaces_and_invalid(B):
    """white space and invalid bytes behind the last unit; sentences without units, each with bos / eos"""
    M = model("readme_small")
    sents = [b"ab   ", b"ab\xff\xff", b"ab \xff \x80", b"Z\xff", b"Z \xff", b"   ", b" \t\n ", b"\xff\x80\xfe", b"", "▁▁".encode(), b"\xff", b" " * 200, b"\x80" * 130,
             b"ab" + b" " * 100, b"Z" + b"\xff" * 100, b"Z" + b"\xff" * 100 + b"Z", b"\xff" * 70 + b"ab"]
    for f, (id_rows, sp_rows) in all_flags(M, B, sents, "spaces and invalid bytes").items():
        for k in (5, 6, 7, 8, 9, 10, 11, 12):
            assert len(id_rows[k]) == f[0] + f[1] and all(p == [0, 0] for p in sp_rows[k]), (f, k)
        if f[1] and not f[2]:
            assert sp_rows[0][-1] == [2, 2] and sp_rows[1][-1] == [2, 2], "an <EOS> sits at the end of the last unit"
        assert [p for p in sp_rows[15] if p[0] != p[1]][0] == [0, 102]


def check_groups(B, aligns=(0, 5)):
    """groups of short sentences, guard bytes around the text, the text at different address alignments"""
    M = model("readme_small")
    rng = random.Random(3)
    pool = ["", "a", "ab", "Z", "ab Z", "é", "abcd ab", " ", "中 a", "b" * 9, "abZ中 d", b"a\xffb", b"\x80"]
    for n in (1, 2, 3, 64, 700):
        sents = [rng.choice(pool) for _ in range(n)]
        for align in aligns:
            for f in ((0, 0, 0), (1, 1, 1)):
                check_batch(M, B, sents, *f, what=("groups", n, align), align=align)
    sents = [rng.choice(pool) for _ in range(5000)]
    check_batch(M, B, sents, 1, 1, 0, what="groups, 5000", align=aligns[-1])


def check_api_forms(B):
    """reverse with more than 64 ids; the padded form, width > longest; the text route against the split route; the list API in both units"""
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    M = model("readme_small")
    core = M.core
    sents = sentences_of("readme_small")[:30] + ["ab Z " * 40, "", "é中 ab", " "] + mixed_sentences(M, 20)
    id_rows, sp_rows = check_batch(M, B, sents, 1, 1, 1, what="reverse")
    assert max(len(r) for r in id_rows) > 64
    fwd = check_batch(M, B, sents, 1, 1, 0, what="forward")
    assert [r[::-1] for r in sp_rows] == fwd[1], "reverse is the forward spans back to front"
    # padded: the spans pending after the forward call
    n, longest = len(sents), max(len(r) for r in fwd[0])
    need = C.c_uint64()
    for width in (longest, longest + 3):
        d_m = B.empty(n * width * 2 + 2, np.int32)
        assert L.yttm_spans_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), n, width, C.byref(need), err, _lib.ERRLEN) == 0, err.value
        got = B.get(d_m).view(np.uint32)
        assert got[n * width * 2:].view(np.int32).tolist() == [-7, -7], "written behind the matrix"
        m = got[:n * width * 2].reshape(n, width, 2).tolist()
        assert need.value == longest and m == [r + [[0, 0]] * (width - len(r)) for r in fwd[1]]
    d_m = B.empty(n * longest * 2, np.int32)
    rc = L.yttm_spans_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), n, longest - 1, C.byref(need), err, _lib.ERRLEN)
    rc2 = L.yttm_encode_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), C.c_void_p(B.ptr(d_m)), n, longest - 1, 0, None, err, _lib.ERRLEN)
    msg2 = err.value
    assert rc == 1 and rc2 == 1 and need.value == longest
    L.yttm_spans_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), n, longest - 1, C.byref(need), err, _lib.ERRLEN)
    assert err.value == msg2 and set(B.get(d_m).tolist()) == {-7}
    # the text route: a sentence is a line with its newline
    for data in (b"".join(x + b"\n" for x in to_bytes(sents) if b"\n" not in x), b"ab Z\r\ncd", b"", b"\n\nZ"):
        lines = K.py_split(data)
        for b, e, r in FLAGS:
            for align in (0, 3):
                P = K.Placed(B, data, align)
                nl, ni, ms = C.c_uint64(), C.c_uint64(), C.c_double()
                assert L.yttm_spans_text_device(core._h, C.c_void_p(P.ptr), len(data), b, e, r, 0.0, C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN) == 0, err.value
                assert P.intact() and nl.value == len(lines)
                ids, ioff = D.encode_fetch(core, nl.value, ni.value)
                spans = take_spans(core, B, nl.value, ni.value)
                assert core.fetch_lines(nl.value).tolist() == K.py_offsets(data).tolist()
                rc, _, w_ids, w_off, w_spans = dev_spans(core, B, lines, b, e, r)
                assert rc == 0 and ids.tolist() == w_ids.tolist() and ioff.tolist() == w_off.tolist() and spans.tolist() == w_spans.tolist(), (data[:40], b, e, r)
    # host to host, and the list API: s[a:b] is the token's text
    strs = [s for s in sents if isinstance(s, str)] + ["жук ab", "日本 の Z😀Z b", "é" * 70 + " ab"]
    for b, e, r in FLAGS:
        ids_l, by = M.bpe.encode_with_spans(strs, bos=bool(b), eos=bool(e), reverse=bool(r), unit="byte")
        ids_c, ch = M.bpe.encode_with_spans(strs, bos=bool(b), eos=bool(e), reverse=bool(r), unit="char")
        assert ids_l == ids_c == M.bpe.encode(strs, bos=bool(b), eos=bool(e), reverse=bool(r))
        rc, _, w_ids, w_off, w_spans = dev_spans(core, B, strs, b, e, r)
        assert [[list(p) for p in row] for row in by] == rows(w_spans, w_off)
        for s, row, r_by, r_ch in zip(strs, ids_l, by, ch):
            raw = s.encode()
            for t, (a0, b0), (a1, b1) in zip(row, r_by, r_ch):
                assert raw[a0:b0].decode() == s[a1:b1]
                if t != M.unk and M.vocab[t] not in SPECIAL:
                    assert s[a1:b1] == M.vocab[t].replace("▁", "")
                elif t == M.unk:
                    assert s[a1:b1] and all(ord(c) not in M.alphabet for c in s[a1:b1])
    assert M.bpe.encode_with_spans([]) == ([], [])
    assert M.bpe.encode_with_spans(["", "ab"], unit="byte")[1][0] == []
    import pytest
    with pytest.raises(ValueError, match="unit must be"):
        M.bpe.encode_with_spans(["ab"], unit="word")
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        M.bpe.encode_with_spans(["ab"], dropout_prob=2)


def check_errors(B):
    """bos / eos on a model without them: the existing message and code, nothing pending is replaced; a plain encode empties the span slot"""
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    M = model("nopad")
    core = M.core
    sents = ["ab Z cd", "", "abcd"]
    buf = np.zeros((64, 2), np.uint32)
    fetch = lambda n: L.yttm_spans_fetch(core._h, buf.ctypes.data_as(_lib.u32p), n, err, _lib.ERRLEN)  # noqa: E731
    assert fetch(3) == 1, "a fresh encoder has no spans"
    for b, e in ((1, 0), (0, 1), (1, 1)):
        rc, msg = dev_spans(core, B, sents, b, e, 0)[:2]
        assert rc == 1 and "token. Model was trained without it." in msg
        ids, off, spans = C.POINTER(C.c_int32)(), _lib.u64p(), _lib.u32p()
        blob, o = K.pack(to_bytes(sents))
        assert L.yttm_encode_as_ids_spans(core._h, blob, o.ctypes.data_as(_lib.u64p), 3, b, e, 0, 0.0, C.byref(ids), C.byref(off), C.byref(spans), err, _lib.ERRLEN) == 1
        assert err.value.decode() == msg
    assert fetch(3) == 1
    good = dev_spans(core, B, sents)
    assert good[0] == 0
    assert dev_spans(core, B, sents + ["x"], 1, 1, 0)[0] == 1
    P = K.Placed(B, b"ab\nZ\n")
    nl, ni, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    assert L.yttm_spans_text_device(core._h, C.c_void_p(P.ptr), 5, 0, 1, 0, 0.0, C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN) == 1
    assert err.value.decode() == EOS_MSG and (nl.value, ni.value) == (0, 0)
    ids, ioff = D.encode_fetch(core, 3, len(good[2]))
    assert ids.tolist() == good[2].tolist() and take_spans(core, B, 3, len(good[2])).tolist() == good[4].tolist(), "a failed call replaced what was pending"
    assert fetch(2) == 1, "another sentence count"
    # a plain encode afterwards: the ids are its own, the spans are gone
    D.encode_device(core, B, to_bytes(sents))
    assert fetch(3) == 1 and b"no matching result" in err.value
    d_m = B.empty(64, np.int32)
    assert L.yttm_spans_copy_device(core._h, C.c_void_p(B.ptr(d_m)), 3, err, _lib.ERRLEN) == 1
    assert L.yttm_spans_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), 3, 10, None, err, _lib.ERRLEN) == 1
    assert set(B.get(d_m).tolist()) == {-7}
    # an empty batch, also through null pointers
    empty = dev_spans(core, B, [])
    assert empty[0] == 0 and len(empty[2]) == 0 and empty[3].tolist() == [0] and empty[4].shape == (0, 2)
    assert L.yttm_spans_device(core._h, None, None, 0, 0, 0, 0, 0, 0, 0.0, C.byref(ni), C.byref(ms), err, _lib.ERRLEN) == 0 and ni.value == 0
    assert fetch(0) == 0


def check_large(B, name="zipf", n=50_000, width=128, frac=0.01):
    """one larger pass through the property check: n sentences of `width` chars of Zipf text, about 1 % of the chars outside the alphabet"""
    import gen
    M = model(name)
    u = unknown_chars(M.alphabet)
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=23, vocab=20000).replace(b"\n", b" ")[:n * width]
    cps = np.frombuffer(raw, np.uint8).astype("<u4")
    rng = np.random.default_rng(5)
    hit = rng.random(len(cps)) < frac
    cps[hit] = rng.choice(np.array([ord(c) for c in u.values()], "<u4"), size=int(hit.sum()))
    text = cps.tobytes().decode("utf-32-le")
    sents = [text[i * width:(i + 1) * width] for i in range(n)]
    id_rows, _ = check_batch(M, B, sents, 1, 1, 0, what="large", rule=False)
    assert n * 0.5 < sum(1 for row in id_rows if M.unk in row) < n * 0.9
