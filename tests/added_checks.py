"""Checks of the added tokens (yttm_encoder_set_added_tokens, yttm_encoder_added_tokens, yttm_encoder_added_tokens_stats, yttm_added_split_device,
yttm_added_split_fetch, yttm_added_split_copy_device, BPE.set_added_tokens / added_tokens / added_tokens_stats / split_added_tensor,
`yttm ... --added_tokens`), shared by the emulator tests (test_added_device.py, test_added_device_sched.py: numpy arrays are "device" memory
there) and the MI355X tests (test_gpu_added.py: torch tensors).

The yardsticks share no code with the passes:
  (a) the matcher (py_matches, py_split): the loop of the rule in include/yttm_mi355x.h "Added tokens", over bytes;
  (b) the join (want_rows): Python list concatenation over the encode of every segment, one call with the setting off;
  (c) properties: decode of the result is the concatenation of decode(E(g)) and the tokens; every id is below V, a byte id, or A + k of a token
      the matcher found there; setting the tokens twice changes nothing; a text without a match gives the parent's ids and the counters show
      the skip.
Every case that is not trivial asserts from (a) that its input holds a match."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import restrict_checks as RS
import subword_checks as SW
from decode_checks import G, NumpyBuf, TorchBuf, model_args  # noqa: F401  (the buffers are re-exported)
from spans_checks import FLAGS, all_models, model_path, sentences_of, to_bytes  # noqa: F401
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
TOKENS = ["<sep>", "<2en>", "<mask>", "<extra_id_17>", "<", "<2"]  # (a token may be a prefix of another)
NOT_SET = "added_split_device: no added tokens are set"
NO_SPANS = "spans are not defined under added tokens"
NO_SUBWORD = "SUBWORD output under added tokens needs byte fallback"
NO_SPLIT = "added_split: no matching split result"


def tok_bytes(tokens):
    return [t.encode() if isinstance(t, str) else bytes(t) for t in tokens]


# ---- yardstick (a): the matcher ------------------------------------------------------------------------------------------------------------------
def py_matches(sent, toks):
    """[(position, token index)] of one sentence: leftmost first, the longest at a position, non-overlapping"""
    out, p = [], 0
    firsts = {t[0] for t in toks}  # (only to skip the inner loop where it cannot succeed)
    while p < len(sent):
        if sent[p] not in firsts:
            p += 1
            continue
        best = -1
        for k, t in enumerate(toks):
            if sent[p:p + len(t)] == t and (best < 0 or len(t) > len(toks[best])):
                best = k
        if best >= 0:
            out.append((p, best))
            p += len(toks[best])
        else:
            p += 1
    return out


def py_split(sents, toks):
    """-> (sub_first [n + 1], sub_offsets [n_sub + 1] into the packed text, tok [n_sub])"""
    first, off, tok, base = [0], [], [], 0
    for s in sents:
        off.append(base)
        tok.append(-1)
        for p, k in py_matches(s, toks):
            off += [base + p, base + p + len(toks[k])]
            tok += [k, -1]
        base += len(s)
        first.append(len(tok))
    return first, off + [base], tok


def has_match(sents, toks):
    return any(py_matches(s, toks) for s in sents)


# ---- yardstick (b): the join ---------------------------------------------------------------------------------------------------------------------
def packed_rows(core, segs, dropout=0.0):
    """the ids of byte strings as sentences of their own, one host call, bos = eos = reverse = false"""
    blob, off = K.pack(segs)
    ids, o = core.encode_packed(blob, off, False, False, False, dropout)
    return K.rows(ids, o)


def refined(sents, toks):
    """the refined batch: g_0, m_1, g_1, ..., m_j, g_j of every sentence in text order, and per sentence its (kind, ...) list"""
    batch, shape = [], []
    for s in sents:
        cur, p = [], 0
        for q, k in py_matches(s, toks):
            cur += [("g", len(batch)), ("m", k)]
            batch += [s[p:q], toks[k]]
            p = q + len(toks[k])
        cur.append(("g", len(batch)))
        batch.append(s[p:])
        shape.append(cur)
    return batch, shape


def want_rows(plain, sents, toks, A, bos=0, eos=0, rev=0, ids_of_batch=None):
    """`plain`: a core with the setting off and the other settings of the encoder under test.  ids_of_batch: the rows of the refined batch
    where the caller made them himself (dropout)"""
    batch, shape = refined(sents, toks)
    rows = ids_of_batch if ids_of_batch is not None else packed_rows(plain, batch)
    assert len(rows) == len(batch)
    a = model_special(plain)
    out = []
    for cur in shape:
        row = [a["bos"]] if bos else []
        for kind, v in cur:
            row += rows[v] if kind == "g" else [A + v]
        if eos:
            row.append(a["eos"])
        out.append(row[::-1] if rev else row)
    return out


_special = {}


def model_special(core):
    return _special[id(core)]


class Model:
    def __init__(self, name):
        self.name, self.path = name, model_path(name)
        a = model_args(name)
        self.unk, self.args = a["unk"], a
        self.alphabet = SW.alphabet_of(self.path)

    def core(self, tokens=None):
        c = D.core_of(self.path)
        _special[id(c)] = self.args
        _keep_cores.append(c)
        if tokens is not None:
            c.set_added_tokens(tokens)
        return c

    def flags(self):
        return [f for f in FLAGS if (not f[0] or self.args["bos"] != -1) and (not f[1] or self.args["eos"] != -1)]


_keep_cores = []  # (id(core) keys _special: the cores stay alive)


def stats(core):
    return np.array(core.added_tokens_stats(), np.int64)


# ---- the stand-alone split -----------------------------------------------------------------------------------------------------------------------
class PlacedText:
    """bytes at an address = align (mod 16) between guard bytes: `head` ends right in front of the text and `tail` starts right behind it, so
    that a read outside the text completes a token"""

    def __init__(self, B, data, align, head=b"", tail=b""):
        self.B, self.n = B, len(data)
        host = np.full(GUARD + 16 + self.n + GUARD, ord("#"), np.uint8)
        self.buf = B.put(host)
        self.start = GUARD + (align - (B.ptr(self.buf) + GUARD)) % 16
        host[self.start:self.start + self.n] = np.frombuffer(bytes(data), np.uint8)
        host[self.start - len(head):self.start] = np.frombuffer(head, np.uint8)
        host[self.start + self.n:self.start + self.n + len(tail)] = np.frombuffer(tail, np.uint8)
        self.host = host
        if isinstance(self.buf, np.ndarray):
            self.buf[:] = host
        else:
            self.buf.copy_(B.torch.from_numpy(host.copy()))
            B.torch.cuda.synchronize()
        assert self.ptr % 16 == align

    @property
    def ptr(self):
        return self.B.ptr(self.buf) + self.start

    def intact(self):
        return self.B.get(self.buf).tobytes() == self.host.tobytes()


def dev_split(core, B, sents, align=0, head=b"", tail=b""):
    """yttm_added_split_device on text placed at `align` between guard bytes + both exits, which must agree and write nothing behind the arrays"""
    blob, off = K.pack(sents)
    T = PlacedText(B, blob, align, head, tail)
    d_off = B.put(off)
    n = len(sents)
    n_sub, n_m, ms = core.added_split_device_raw(T.ptr, B.ptr(d_off), n, len(blob))
    assert T.intact() and B.get(d_off).view(np.uint64).tolist() == off.tolist(), "an input or its guard bytes were written"
    assert n_sub == n + 2 * n_m and ms >= 0
    first, so, tok = core.fetch_added_split(n, n_sub)
    d_first, d_so, d_tok = B.empty(n + 3, np.uint64), B.empty(n_sub + 3, np.uint64), B.empty(n_sub + 2, np.int32)
    core.copy_added_split(B.ptr(d_first), B.ptr(d_so), B.ptr(d_tok), n, n_sub)
    gf, gs, gt = B.get(d_first).view(np.uint64), B.get(d_so).view(np.uint64), B.get(d_tok)
    assert gf[:n + 1].tolist() == first.tolist() and gs[:n_sub + 1].tolist() == so.tolist() and gt[:n_sub].tolist() == tok.tolist(), "the two exits differ"
    assert gf[n + 1:].view(np.int64).tolist() == [-7, -7] and gs[n_sub + 1:].view(np.int64).tolist() == [-7, -7] and gt[n_sub:].tolist() == [-7, -7], \
        "a copy wrote past its array"
    return first.tolist(), so.tolist(), tok.tolist()


def same_split(core, B, sents, toks, what, aligns=(0,), match=True, head=b"", tail=b""):
    sents = to_bytes(sents)
    want = py_split(sents, toks)
    if match:
        assert has_match(sents, toks), (what, "the input holds no match: the case proves nothing")
    for a in aligns:
        got = dev_split(core, B, sents, a, head, tail)
        for name, g, w in zip(("sub_first", "sub_offsets", "tok"), got, want):
            if g != w:
                k = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
                raise AssertionError("%s align %d: %s differs at %d of %d / %d: got %r want %r" % (what, a, name, k, len(g), len(w), g[k:k + 6], w[k:k + 6]))


def set_tokens(core, toks):
    core.set_added_tokens(toks)
    assert core.added_tokens_raw() == tok_bytes(toks)
    return tok_bytes(toks)


def check_synthetic(B, aligns=(0, 3, 8, 15), name="readme_small"):
    M = Model(name)
    core = M.core()
    pair = tuple(aligns[:2])
    T = set_tokens(core, TOKENS)
    # no sentence, empty sentences, the sizes around a wavefront's group
    assert dev_split(core, B, [], 1) == ([0], [0], [])
    same_split(core, B, ["", "", ""], T, "empty only", match=False)
    for n in (1, 63, 64, 65):
        same_split(core, B, ["ab<sep>cd" if i % 3 == 0 else "" if i % 3 == 1 else "plain" for i in range(n)], T, ("n_sent", n), pair)
    # a match at byte 0, at the last bytes, as the whole sentence; across a sentence boundary it is not taken
    same_split(core, B, ["<sep>ab", "ab<sep>", "<sep>", "ab<se", "p>cd", "<2e", "n>", "<mask"], T, "positions", aligns)
    T = set_tokens(core, ["<sep>"])
    assert py_split(to_bytes(["ab<se", "p>cd"]), T)[2] == [-1, -1]
    same_split(core, B, ["ab<se", "p>cd", "<sep", ">"], T, "across a boundary", aligns, match=False)
    T = set_tokens(core, TOKENS)
    # every shift 0 .. 130 of one tail against the 64-byte step, a match straddling the step
    same_split(core, B, ["a" * k + "<extra_id_17>b<sep><sep>c" for k in range(131)], T, "tail shifts", pair)
    # guard bytes that complete a token if they are read: a token's head in front of the text, a token's tail behind it
    T = set_tokens(core, ["<sep>", "<2en>", "<mask>"])
    same_split(core, B, ["sep>ab<se"], T, "guards", aligns, match=False, head=b"<", tail=b"p>")
    same_split(core, B, ["2en>ab<mask", "x<sep>", "<2e"], T, "guards 2", aligns, head=b"<", tail=b"n>")
    T = set_tokens(core, TOKENS)
    same_split(core, B, ["2en>ab<mask", "x<"], T, "guards 3", aligns, head=b"<", tail=b"2en>")
    # longest wins, no overlap
    T = set_tokens(core, ["ab", "abc", "bc", "abcd"])
    assert py_matches(b"abcdabcbc", T) == [(0, 3), (4, 1), (7, 2)]
    same_split(core, B, ["abcdabcbc", "xbcabx", "abcabcdab"], T, "longest wins", aligns)
    T = set_tokens(core, ["aa"])
    assert py_matches(b"aaaaa", T) == [(0, 0), (2, 0)]
    same_split(core, B, ["aaaaa"] + ["b" * k + "a" * 7 for k in range(60, 68)], T, "aa on aaaaa", pair)
    # adjacent matches with empty segments between them; 300 matches in one sentence; more than 63 matches in one step (one-byte tokens)
    T = set_tokens(core, TOKENS)
    same_split(core, B, ["<sep><sep><2en><sep>", "<sep>" * 300, "x" + "<mask>" * 3 + "y"], T, "adjacent", pair)
    T = set_tokens(core, ["a", "b"])
    same_split(core, B, ["ab" * 100, "a" * 64, "c" + "a" * 129 + "c"], T, "one-byte tokens", pair)
    # token lengths 1, 2, 63, 64, 65 and 255
    lens = {n: ("q%d_" % n + "z" * 300)[:n] for n in (1, 2, 63, 64, 65, 255)}
    T = set_tokens(core, list(lens.values()))
    sents = ["ab" + t + "cd" + t for t in lens.values()] + [t for t in lens.values()] + ["x" * k + lens[255] + lens[65] for k in (0, 1, 63, 64)]
    sents.append(lens[255][:-1] + "!" + lens[64][:-1])  # all but the last byte: no match of those
    same_split(core, B, sents, T, "token lengths", pair)
    # 4096 tokens that share their first three bytes
    many = ["<ex%d>" % k for k in range(4096)]
    T = set_tokens(core, many)
    same_split(core, B, ["a<ex7>b<ex4095><ex40955>", "<ex", "<ex123<ex1234>", "<ex409"], T, "4096 tokens", pair[:1])
    # tokens of 2-, 3- and 4-byte characters, and characters outside the alphabet; invalid bytes in front of and behind a match
    u = SW.unknown_chars(M.alphabet)
    T = set_tokens(core, [u[2], u[3] + u[3], u[4], "<" + u[2] + ">", "Z"])
    sents = ["a" + u[2] + "b" + u[3] + u[3] + u[3], u[4] + "<" + u[2] + ">" + u[4], "aZb", b"\xff" + u[4].encode() + b"\x80\xc3", u[3].encode()[:2] + u[2].encode() + b"\xe2"]
    same_split(core, B, sents, T, "multi-byte tokens", aligns)
    # a 50 000-byte sentence; 1 500 sentences over several workgroups
    T = set_tokens(core, TOKENS)
    rng = np.random.RandomState(7)
    words = ["ab", "cd<sep>", "<2en>", "abcd", "<", "a<mask>b", "dcba", "<extra_id_17>"]
    long_s = " ".join(words[i] for i in rng.randint(0, len(words), 12000))[:50000]
    same_split(core, B, [long_s, "tail<sep>"], T, "a long sentence", pair[:1])
    sents = [" ".join(words[i] for i in rng.randint(0, len(words), 1 + k % 9)) if k % 11 else "" for k in range(1500)]
    same_split(core, B, sents, T, "1500 sentences", pair[:1])


# ---- the wired route -----------------------------------------------------------------------------------------------------------------------------
def spliced(lines, tokens):
    """tokens spliced into lines at word starts, inside words and at line ends"""
    out = []
    for i, s in enumerate(lines):
        t = tokens[i % len(tokens)]
        words = s.split(" ")
        if i % 4 == 0:
            out.append(t + s)
        elif i % 4 == 1 and words:
            w = words[len(words) // 2]
            words[len(words) // 2] = w[:len(w) // 2] + t + w[len(w) // 2:]
            out.append(" ".join(words))
        elif i % 4 == 2:
            out.append(s + t)
        else:
            out.append(s)
    return out + [t for t in tokens[:2]] + [tokens[0] + " \t " + tokens[1], tokens[0] + tokens[0], ""]


def batch_of(name, most=24):
    return spliced(sentences_of(name, most), TOKENS)


def encode_rows(core, B, raw, b, e, r, dropout=0.0):
    return RS.encode_rows(core, B, raw, b, e, r, dropout)


def check_ids(rows, sents, toks, V, A):
    """(c): every id is below V, a byte id, or A + k of a token the matcher found in that sentence"""
    for row, s in zip(rows, sents):
        found = {A + k for _, k in py_matches(s, toks)}
        assert all(0 <= t < A or t in found for t in row) and found <= set(row), (s[:40], row[:20])


def check_routes_model(B, name):
    """yttm_encode_device + both exits under every flag set, with the word cache forced on and off; the counters; decode; clearing"""
    M = Model(name)
    plain, core = M.core(), M.core(TOKENS)
    T = tok_bytes(TOKENS)
    V = core.vocab_size()
    A = V + 256
    raw = to_bytes(batch_of(name))
    assert has_match(raw, T)
    n_sub = len(refined(raw, T)[0])
    for f in M.flags():
        want = want_rows(plain, raw, T, A, *f)
        check_ids(want, raw, T, V, A)
        for cache in (1, 0):
            core.set_cache(cache)
            before = stats(core)
            got, ms = encode_rows(core, B, raw, *f)
            assert got == want, (name, f, cache, next((g, w) for g, w in zip(got, want) if g != w))
            assert ms >= 0 and (stats(core) - before).tolist() == [1, 0, (n_sub - len(raw)) // 2, n_sub]
        core.set_cache(2)
    # (c) decode of the result = the concatenation of decode(E(g)) and the tokens
    batch, shape = refined(raw, T)
    seg_rows = packed_rows(plain, batch)
    rows = encode_rows(core, B, raw, 0, 0, 0)[0]
    flat, off = D.flatten(rows)
    dev, host = D.dev_decode(core, B, flat, off), D.host_decode(core, flat, off)
    assert dev[0] == 0 and host[0] == 0 and dev[2] == host[2] and dev[3].tolist() == host[3].tolist(), (dev[:2], host[:2])
    o = [int(x) for x in dev[3]]

    def unstripped(row):  # the text of a segment's ids where they are not a sentence's first: decode strips only the first piece's space
        if not row:
            return b""
        return D.host_decode(plain, *D.flatten([[row[0]] + row]))[2][len(D.host_decode(plain, *D.flatten([row[:1]]))[2]):]

    for i, cur in enumerate(shape):
        parts = [T[v] if kind == "m" else unstripped(seg_rows[v]) for kind, v in cur]
        if parts[0].startswith(b" "):
            parts[0] = parts[0][1:]
        assert dev[2][o[i]:o[i + 1]] == b"".join(parts), (name, i, dev[2][o[i]:o[i + 1]], parts)
        if len(cur) == 1:
            assert b"".join(parts) == (D.host_decode(plain, *D.flatten([seg_rows[cur[0][1]]]))[2] if seg_rows[cur[0][1]] else b"")
    # setting the same tokens again changes nothing
    core.set_added_tokens(TOKENS)
    assert encode_rows(core, B, raw, 0, 0, 0)[0] == rows
    # a text without a match: the parent's ids, and the counters show the skip
    none = [s for s in to_bytes(sentences_of(name, 12)) if not py_matches(s, T)]
    assert none
    before = stats(core)
    assert encode_rows(core, B, none, 0, 0, 0)[0] == encode_rows(plain, B, none, 0, 0, 0)[0]
    assert (stats(core) - before).tolist() == [1, 1, 0, len(none)]
    # clearing the setting restores the parent's ids exactly, and counts no call
    core.set_added_tokens(None)
    before = stats(core)
    for f in M.flags():
        assert encode_rows(core, B, raw, *f)[0] == encode_rows(plain, B, raw, *f)[0]
    assert (stats(core) - before).tolist() == [0, 0, 0, 0] and core.added_tokens_raw() == []


def check_small_cases(B, name="readme_small"):
    """bos, eos and reverse; a sentence that is only a token; only white space between two tokens; a token inside a word"""
    M = Model(name)
    plain, core = M.core(), M.core(TOKENS)
    T, A = tok_bytes(TOKENS), core.vocab_size() + 256
    raw = [b"<sep>", b"<sep> \t <2en>", b"ab<mask>cd", b" <2en>abcd ab", b"", b"abcd", b"<<2<2en><2e", b"<sep><sep>"]
    a = M.args
    for f in M.flags():
        got = encode_rows(core, B, raw, *f)[0]
        assert got == want_rows(plain, raw, T, A, *f), f
        core_ids = [[t for t in (r[::-1] if f[2] else r) if not (f[0] and t == a["bos"]) and not (f[1] and t == a["eos"])] for r in got]
        assert core_ids[0] == [A] and core_ids[1] == [A, A + 1] and core_ids[7] == [A, A] and core_ids[4] == []
        assert core_ids[6] == [A + 4, A + 5, A + 1, A + 5] + packed_rows(plain, [b"e"])[0]
        assert core_ids[2] == packed_rows(plain, [b"ab"])[0] + [A + 2] + packed_rows(plain, [b"cd"])[0]
        if f[0] and not f[2]:
            assert all(r[0] == a["bos"] for r in got)
        if f[1] and f[2]:
            assert all(r[0] == a["eos"] for r in got)


def check_dropout(B, name="readme_small"):
    """dropout 0.1 and 1 under a pinned salt: the ids are the join of what the setting-off encoder returns for the refined batch"""
    M = Model(name)
    T = tok_bytes(TOKENS)
    raw = to_bytes(batch_of(name))
    assert has_match(raw, T)
    batch, _ = refined(raw, T)
    with DC.env():
        a, b = M.core(), M.core(TOKENS)
    A = a.vocab_size() + 256
    none = want_rows(M.core(), raw, T, A)  # (an encoder of its own: a and b draw alike only call by call)
    assert encode_rows(b, B, raw, 0, 0, 0)[0] == want_rows(a, raw, T, A, ids_of_batch=encode_rows(a, B, batch, 0, 0, 0)[0])
    for p in (0.1, 1.0):
        for f in ((0, 0, 0), (1, 1, 1)):
            ref_rows = encode_rows(a, B, batch, 0, 0, 0, dropout=p)[0]
            want = want_rows(a, raw, T, A, *f, ids_of_batch=ref_rows)
            assert f != (0, 0, 0) or want != none
            assert encode_rows(b, B, raw, *f, dropout=p)[0] == want, (p, f)


def check_with_settings(B, name="readme_small"):
    """with a restricted vocabulary, with the byte fallback (a<sep>é€b, `<` outside the alphabet), and with both, against (b) under the same settings"""
    M = Model(name)
    T = tok_bytes(TOKENS)
    raw = to_bytes(batch_of(name)) + ["a<sep>é€b".encode(), "é<2en>€ <mask>😀".encode()]
    assert ord("<") not in M.alphabet and has_match(raw, T)
    R = RS.Rules(M.path, D.core_of(M.path).vocab_size())
    allowed = R.masks()["odd"]
    for voc, bfb in ((1, 0), (0, 1), (1, 1)):
        plain, core = M.core(), M.core(TOKENS)
        V = core.vocab_size()
        A = V + 256
        for c in (plain, core):
            if voc:
                c.set_vocabulary(allowed)
            c.set_byte_fallback(bool(bfb))
        base = want_rows(M.core(), raw, T, A)
        for f in M.flags():
            want = want_rows(plain, raw, T, A, *f)
            assert f != (0, 0, 0) or want != base, "the other setting changes nothing: the case proves nothing"
            got = encode_rows(core, B, raw, *f)[0]
            assert got == want, (voc, bfb, f, next((g, w) for g, w in zip(got, want) if g != w))
            check_ids(got, raw, T, V, A)
        if bfb:
            i = len(raw) - 2
            row = encode_rows(core, B, raw, 0, 0, 0)[0][i]
            assert A in row and all(V + x in row for x in "é€".encode()) and M.unk not in row
            # (the segment behind the token starts inside a word and gets its own U+2581: decode shows it as a space, and strips only the first one)
            assert D.host_decode(core, *D.flatten([row]))[2] == "a<sep> é€b".encode()


# ---- the other routes ----------------------------------------------------------------------------------------------------------------------------
_keep = []


def _placed(B, raw):
    blob, off = K.pack(raw)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    _keep[:] = [d_b, d_o]  # (alive until the next call)
    return B.ptr(d_b), B.ptr(d_o)


def check_python_routes(B, name="readme_small"):
    """BPE.encode(list), the names, SUBWORD on the host and the device, the decodes, the counts, id text, the spans' refusal"""
    import pytest
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    _special[id(plain.bpe_cython)] = M.args
    V = bpe.vocab_size()
    A, n = V + 256, len(TOKENS)
    T = tok_bytes(TOKENS)
    assert bpe.added_tokens() is None and bpe.added_tokens_stats() == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        bpe.id_to_subword(A)
    assert bpe.subword_to_id("<sep>") == M.unk
    bpe.set_added_tokens(TOKENS)
    assert bpe.added_tokens() == {t: A + k for k, t in enumerate(TOKENS)} and list(bpe.added_tokens()) == TOKENS
    assert bpe.vocab_size() == V and bpe.vocab() == plain.vocab()
    sents = batch_of(name)
    raw = to_bytes(sents)
    assert has_match(raw, T)
    want = want_rows(plain.bpe_cython, raw, T, A, bos=1)
    assert bpe.encode(sents, bos=True) == want
    assert bpe.encode(sents, bos=True, reverse=True) == [r[::-1] for r in want]
    # names
    for k, t in enumerate(TOKENS):
        assert bpe.id_to_subword(A + k) == t and bpe.subword_to_id(t) == A + k
    for bad in (A + n, V, A - 1, -1):
        with pytest.raises(ValueError, match="id must be in the range"):
            bpe.id_to_subword(bad)
    assert bpe.subword_to_id("<sepx>") == M.unk and bpe.subword_to_id("<0x41>") == M.unk
    # decode: on the device = on the host; ignore_ids naming an added id; A + n and -1 with the parent's message; a byte id refused
    core = bpe.bpe_cython
    ids = bpe.encode(sents)
    flat, off = D.flatten(ids)
    dev, host = D.dev_decode(core, B, flat, off), D.host_decode(core, flat, off)
    assert dev[0] == 0 and dev[2] == host[2] and dev[3].tolist() == host[3].tolist() and b"<sep>" in dev[2]
    assert bpe.decode(ids) == [host[2][int(host[3][i]):int(host[3][i + 1])].decode() for i in range(len(ids))]
    drop = [A, A + 1]
    dev, host = D.dev_decode(core, B, flat, off, drop), D.host_decode(core, flat, off, drop)
    kept = D.host_decode(core, *D.flatten([[t for t in r if t not in drop] for r in ids]))
    assert dev[0] == 0 and dev[2] == host[2] == kept[2] and b"<sep>" not in dev[2] and b"<mask>" in dev[2]
    assert bpe.decode([[A + n - 1, 5]]) == [TOKENS[-1] + plain.decode([[5]])[0]], "the last added id is valid, and its piece is not stripped"
    for bad in (A + n, -1, V, A - 1):
        flat1, off1 = D.flatten([[5, bad]])
        off_msg = D.host_decode(plain.bpe_cython, flat1, off1)
        assert off_msg[0] == 1 and D.host_decode(core, flat1, off1)[:2] == off_msg[:2] and D.dev_decode(core, B, flat1, off1)[:2] == off_msg[:2], bad
    # counts: n_bins = 0 is A + n and the counts sum to the ids; id text prints and parses
    n_ids, _ = core.encode_device_raw(*_placed(B, raw), len(raw), sum(map(len, raw)), max(map(len, raw)), True, False, False, 0.0)
    nc, _ = core.id_counts_device_raw(len(raw))
    counts = core.fetch_id_counts()
    assert len(counts) == A + n + 1 and nc == n_ids == int(counts.sum()) and counts[A + n] == 0 and counts[A] > 0
    assert counts.tolist() == np.bincount(np.array([t for r in want for t in r]), minlength=A + n + 1).tolist()
    n_text, _ = core.idtext_device_raw(len(raw))
    text = core.fetch_decode(len(raw), n_text)[0].tobytes()
    assert text == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want)
    d_t = B.put(np.frombuffer(text + b"\0" * 16, np.uint8))
    nl, ni, _ = core.ids_parse_device_raw(B.ptr(d_t), len(text))
    assert (nl, ni) == (len(raw), n_ids) and K.rows(*K.take_encoded(core, B, nl, ni)) == want
    n_ids, _ = core.encode_device_raw(*_placed(B, raw), len(raw), sum(map(len, raw)), max(map(len, raw)), True, False, False, 0.0)
    # spans: refused before any work, everything pending stays
    pending = D.encode_fetch(core, len(raw), n_ids)[0].tolist()
    d_b, d_o = _placed(B, raw)
    L, err, z = _lib.load(), C.create_string_buffer(_lib.ERRLEN), C.c_uint64()
    rc = L.yttm_spans_device(core._h, C.c_void_p(d_b), C.c_void_p(d_o), len(raw), sum(map(len, raw)), max(map(len, raw)), 0, 0, 0, 0.0, C.byref(z), None, err, _lib.ERRLEN)
    assert rc == 1 and NO_SPANS in err.value.decode()
    rc = L.yttm_spans_text_device(core._h, C.c_void_p(d_b), 5, 0, 0, 0, 0.0, C.byref(z), C.byref(z), None, err, _lib.ERRLEN)
    assert rc == 1 and NO_SPANS in err.value.decode()
    with pytest.raises(ValueError, match=NO_SPANS):
        bpe.encode_with_spans(sents)
    # SUBWORD with the byte fallback off: refused before any work, on the host and on the device
    with pytest.raises(ValueError, match=NO_SUBWORD):
        bpe.encode(sents, output_type=yttm.OutputType.SUBWORD)
    rc = L.yttm_subword_device(core._h, C.c_void_p(d_b), C.c_void_p(d_o), len(raw), sum(map(len, raw)), max(map(len, raw)), 0, 0, 0, 0.0, C.byref(z), C.byref(z), None,
                               err, _lib.ERRLEN)
    assert rc == 1 and NO_SUBWORD in err.value.decode()
    assert D.encode_fetch(core, len(raw), n_ids)[0].tolist() == pending and core.fetch_id_counts().tolist() == counts.tolist()
    # SUBWORD with the byte fallback on: the device formatter is the host loop byte for byte, an added id prints as the token and a space
    bpe.set_byte_fallback(True)
    plain.set_byte_fallback(True)
    ids = bpe.encode(sents)
    assert ids == want_rows(plain.bpe_cython, raw, T, A) and M.unk not in [t for r in ids for t in r]
    pieces = bpe.encode(sents, output_type=yttm.OutputType.SUBWORD)
    vocab = bpe.vocab()
    for ps, row in zip(pieces, ids):
        assert ps == [vocab[t] if t < V else "<0x%02X>" % (t - V) if t < A else TOKENS[t - A] for t in row]
    for f in M.flags():
        lines, rows = SW.same(core, B, sents, *f, what=("SUBWORD", f))
        assert rows == want_rows(plain.bpe_cython, raw, T, A, *f)
        assert b"<sep> " in b"".join(lines)
    bpe.set_added_tokens(None)
    bpe.set_byte_fallback(False)
    plain.set_byte_fallback(False)
    assert bpe.encode(sents, bos=True) == plain.encode(sents, bos=True) and len(bpe.encode_with_spans(sents)[0]) == len(sents)


def check_blocks_and_batches(B, name="readme_small"):
    """blocks and batches of the pending result with added ids in it, through their own property checkers"""
    import batches_checks as BA
    import blocks_checks as BL
    M = Model(name)
    plain, core = M.core(), M.core(TOKENS)
    T = tok_bytes(TOKENS)
    raw = to_bytes(batch_of(name))
    want = want_rows(plain, raw, T, core.vocab_size() + 256, 1, 1, 0)
    assert has_match(raw, T)
    p_b, p_o = _placed(B, raw)
    n_ids, _ = core.encode_device_raw(p_b, p_o, len(raw), sum(map(len, raw)), max(map(len, raw)), True, True, False, 0.0)
    assert n_ids == sum(map(len, want))
    longest = max(map(len, want))
    ids, off = BL.pending_same(core, B, len(raw), n_ids, 64, BL.STREAM, BL.PAD, "blocks of added ids, stream")
    assert K.rows(ids, off) == want
    BL.pending_same(core, B, len(raw), n_ids, longest + 1, BL.WHOLE, BL.KEEP, "blocks of added ids, whole")
    BA.pending_same(core, B, len(raw), n_ids, longest + 3, M=5, left=True, what="batches of added ids")


def file_lines(name):
    return [" ".join(s.replace("▁", " ").split()) for s in batch_of(name)]


def check_files(B, tmp_path, name="readme_small"):
    """encode_file as ids, id text and SUBWORD at three piece sizes, count_file, and decode_file of encode_file"""
    import pytest
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    _special[id(plain.bpe_cython)] = M.args
    bpe.set_added_tokens(TOKENS)
    V = bpe.vocab_size()
    A, n = V + 256, len(TOKENS)
    T = tok_bytes(TOKENS)
    lines = file_lines(name)
    data = "".join(s + "\n" for s in lines).encode()
    raw = [s.encode() + b"\n" for s in lines]  # (a file's sentence is the line with its newline, which no token holds)
    assert has_match(raw, T)
    path, out, back = str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), str(tmp_path / "back.txt")
    open(path, "wb").write(data)
    vocab = bpe.vocab()
    with pytest.raises(ValueError, match=NO_SUBWORD):
        bpe.encode_file(path, out, output_type=yttm.OutputType.SUBWORD)
    for bfb in (False, True):
        bpe.set_byte_fallback(bfb)
        plain.set_byte_fallback(bfb)
        for b, e, r in ((0, 0, 0), (1, 1, 1)):
            want = want_rows(plain.bpe_cython, raw, T, A, b, e, r)
            flat = np.array([t for row in want for t in row], np.int64)
            for chunk in (None, max(len(data) // 8, 1), 1):
                g_ids, g_off = bpe.encode_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
                assert K.rows(g_ids, g_off) == want, (b, e, r, chunk)
                nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, id_text=True)
                assert (nl, ni) == (len(want), len(flat))
                assert open(out, "rb").read() == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want), (chunk, "id_text")
                if (b, e, r) == (0, 0, 0):
                    bpe.decode_file(out, back, chunk_bytes=chunk)
                    dec = bpe.decode(want)
                    assert open(back, "rb").read() == "".join(s + "\n" for s in dec).encode(), (chunk, "decode_file of encode_file")
                    assert all(t in "".join(dec) for t in TOKENS[:3])
                counts = bpe.count_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
                assert counts.tolist() == np.bincount(flat, minlength=A + n + 1).tolist(), (chunk, "counts")
                if bfb:
                    nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, output_type=yttm.OutputType.SUBWORD)
                    assert (nl, ni) == (len(want), len(flat))
                    text = b"".join(b"".join((vocab[t] if t < V else "<0x%02X>" % (t - V) if t < A else TOKENS[t - A]).encode() + b" " for t in row) + b"\n"
                                    for row in want)
                    assert open(out, "rb").read() == text, (chunk, "SUBWORD")


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------
def raw_split(core, p_text, p_off, n_sent, n_bytes):
    ns, nm, err = C.c_uint64(7), C.c_uint64(7), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_added_split_device(core._h, C.c_void_p(p_text), C.c_void_p(p_off), n_sent, n_bytes, C.byref(ns), C.byref(nm), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), ns.value, nm.value


def check_errors(B, name="readme_small"):
    import pytest
    M = Model(name)
    core = M.core()
    sents = [b"ab<sep>cd", b"<2en>"]
    # the split without the setting: code 1, nothing is replaced
    p_b, p_o = _placed(B, sents)
    assert raw_split(core, p_b, p_o, 2, 14) == (1, NOT_SET, 0, 0)
    with pytest.raises(ValueError, match=NO_SPLIT):
        core.fetch_added_split(2, 2)
    # every invalid token set leaves the setting as it was
    core.set_added_tokens(TOKENS)
    T = tok_bytes(TOKENS)
    want = py_split(sents, T)
    bad_sets = {
        "empty": ["a", ""], "256 bytes": ["x" * 256], "a space": ["a b"], "a newline": ["a\nb"], "U+2581": ["a▁"], "invalid UTF-8": [b"\xff\xfe"],
        "a duplicate": ["a", "b", "a"], "4097 tokens": ["<t%d>" % k for k in range(4097)], "no token": [], "a tab": ["\t"],
    }
    for what, toks in bad_sets.items():
        with pytest.raises(ValueError, match="set_added_tokens"):
            core.set_added_tokens(toks)
        assert core.added_tokens_raw() == T, what
    assert dev_split(core, B, sents) == want and encode_rows(core, B, sents, 0, 0, 0)[0] == want_rows(M.core(), sents, T, core.vocab_size() + 256)
    with pytest.raises(TypeError):
        core.set_added_tokens("<sep>")
    # wrong counts at the split's exits; null pointers are skipped
    n_sub = len(want[2])
    for n_s, n_q in ((1, n_sub), (2, n_sub + 1), (3, n_sub), (2, 0)):
        with pytest.raises(ValueError, match=NO_SPLIT):
            core.fetch_added_split(n_s, n_q)
        with pytest.raises(ValueError, match=NO_SPLIT):
            core.copy_added_split(0, 0, 0, n_s, n_q)
    L, err = _lib.load(), C.create_string_buffer(_lib.ERRLEN)
    tok = np.full(n_sub, 9, np.int32)
    assert L.yttm_added_split_fetch(core._h, None, None, tok.ctypes.data_as(_lib.i32p), 2, n_sub, err, _lib.ERRLEN) == 0 and tok.tolist() == want[2]
    assert L.yttm_added_split_copy_device(core._h, None, None, None, 2, n_sub, err, _lib.ERRLEN) == 0
    # a later refused split leaves the slot; clearing the setting refuses the split again
    assert raw_split(core, p_b, 0, 2, 14)[0] == 2
    core.set_added_tokens(None)
    assert raw_split(core, p_b, p_o, 2, 14)[:2] == (1, NOT_SET)
    # the setting while a result is pending does not change that result
    plain = M.core()
    n = D.encode_device(plain, B, sents, 0, 0, 0)
    pending = D.encode_fetch(plain, 2, n)[0].tolist()
    plain.set_added_tokens(TOKENS)
    assert D.encode_fetch(plain, 2, n)[0].tolist() == pending


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------
def check_cli(tmp_path, name="readme_small"):
    """--added_tokens on encode, encode_file, count_file, decode and decode_file, a vocabulary file written with the flag, an empty line.  Seven
    processes."""
    import youtokentome_amd as yttm
    M = Model(name)
    plain = yttm.BPE(M.path)
    _special[id(plain.bpe_cython)] = M.args
    V = plain.vocab_size()
    A, n = V + 256, len(TOKENS)
    T = tok_bytes(TOKENS)
    lines = file_lines(name)
    data = "".join(s + "\n" for s in lines).encode()
    path, voc, out, tf = str(tmp_path / "in.txt"), str(tmp_path / "voc.tsv"), str(tmp_path / "out.txt"), str(tmp_path / "tokens.txt")
    open(path, "wb").write(data)
    open(tf, "wb").write(b"".join(t + b"\n" for t in T))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def run(args, stdin=None, ok=True):
        p = subprocess.run(cli + args, capture_output=True, env=env, input=stdin)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout if ok else p.stderr

    raw = to_bytes(lines)
    assert has_match(raw, T)
    want = want_rows(plain.bpe_cython, raw, T, A)
    text = b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want)
    flag = f"--added_tokens={tf}"
    assert run(["encode", f"--model={M.path}", "--output_type=id", flag], stdin=data) == text
    bpe = yttm.BPE(M.path)
    bpe.set_added_tokens(TOKENS)
    decoded = "".join(s + "\n" for s in bpe.decode(want)).encode()
    assert run(["decode", f"--model={M.path}", flag], stdin=text) == decoded and b"<sep>" in decoded
    run(["encode_file", f"--model={M.path}", f"--input={path}", f"--output={out}", "--output_type=id_text", flag])
    assert open(out, "rb").read() == text
    run(["decode_file", f"--model={M.path}", f"--input={out}", f"--output={out}.txt", flag])
    assert open(out + ".txt", "rb").read() == decoded
    run(["count_file", f"--model={M.path}", f"--input={path}", f"--output={voc}", flag])
    rows = [ln.split(b"\t") for ln in open(voc, "rb").read().split(b"\n")[:-1]]
    assert len(rows) == A + n and [int(r[2]) for r in rows] == np.bincount(np.array([t for r in want for t in r]), minlength=A + n).tolist()
    assert [r[1] for r in rows[A:]] == T and all(rows[V + b][1] == b"<0x%02X>" % b for b in range(256))
    # that file as --vocabulary: its rows A .. A + n - 1 must read the tokens and are otherwise ignored
    R = RS.Rules(M.path, V)
    counts = np.array([int(r[2]) for r in rows[:V]])
    restricted = yttm.BPE(M.path)
    restricted.set_vocabulary(counts >= 2)
    _special[id(restricted.bpe_cython)] = M.args
    got = run(["encode", f"--model={M.path}", "--output_type=id", flag, f"--vocabulary={voc}", "--vocabulary_threshold=2"], stdin=data)
    assert got == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want_rows(restricted.bpe_cython, raw, T, A))
    # an empty line is an error
    open(tf, "wb").write(b"<sep>\n\n<2en>\n")
    assert b"an empty line is no token" in run(["encode", f"--model={M.path}", "--output_type=id", flag], stdin=data, ok=False)


# ---- torch tensors (MI355X) ----------------------------------------------------------------------------------------------------------------------
def check_tensor_api(name="readme_small"):
    import pytest
    import torch
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    _special[id(plain.bpe_cython)] = M.args
    with pytest.raises(ValueError, match="no added tokens are set"):
        bpe.split_added_tensor(["<sep>"])
    bpe.set_added_tokens(TOKENS)
    T = tok_bytes(TOKENS)
    A = bpe.vocab_size() + 256
    sents = batch_of(name)
    raw = to_bytes(sents)
    want = py_split(raw, T)
    first, off, tok = bpe.split_added_tensor(sents)
    assert first.is_cuda and (first.dtype, off.dtype, tok.dtype) == (torch.int64, torch.int64, torch.int32)
    assert (first.tolist(), off.tolist(), tok.tolist()) == want
    blob, o = K.pack(raw)
    d_text = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(o.astype(np.int64)).cuda()
    got = bpe.split_added_tensor(d_text, d_off)
    assert tuple(t.tolist() for t in got) == want
    rows = want_rows(plain.bpe_cython, raw, T, A, bos=1)
    ids, lengths = bpe.encode_tensor(sents, bos=True)[:2]
    assert [ids[i, :int(lengths[i])].tolist() for i in range(len(sents))] == rows
    texts = bpe.decode_tensor(ids, lengths=lengths)
    assert list(texts) == bpe.decode(rows)


def check_large(B, name="readme_small", n=50_000, width=128, frac=0.01):
    """one pass of n sentences of `width` chars, a tag in front of every sentence and a token inside `frac` of the words, against (a) and (b)"""
    import gen
    M = Model(name)
    plain, core = M.core(), M.core(TOKENS)
    T = tok_bytes(TOKENS)
    A = core.vocab_size() + 256
    host = gen.abcd_corpus(n * (width + 1), seed=123, line=width, survey_stream=True)
    lines = host.split(b"\n")[:n]
    rng = np.random.RandomState(11)
    sents = []
    for i, ln in enumerate(lines):
        words = ln.split(b" ")
        for j in np.nonzero(rng.rand(len(words)) < frac)[0]:
            w = words[j]
            words[j] = w[:len(w) // 2] + T[2] + w[len(w) // 2:]
        sents.append(T[i % 2] + b" ".join(words))
    want_split = py_split(sents, T)
    got = dev_split(core, B, sents, 5)
    assert all(np.array_equal(np.array(g, np.int64), np.array(w, np.int64)) for g, w in zip(got, want_split))
    assert len(want_split[2]) > 3 * n
    want = want_rows(plain, sents, T, A, 1, 1, 0)
    got, _ = encode_rows(core, B, sents, 1, 1, 0)
    flat_g, off_g = D.flatten(got)
    flat_w, off_w = D.flatten(want)
    assert np.array_equal(np.asarray(off_g), np.asarray(off_w)) and np.array_equal(np.asarray(flat_g), np.asarray(flat_w))
