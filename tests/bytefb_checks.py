"""Checks of the byte fallback (yttm_encoder_set_byte_fallback, yttm_encoder_byte_fallback, yttm_encoder_byte_fallback_stats,
yttm_byte_fallback_ids_device, BPE.set_byte_fallback / byte_fallback / byte_fallback_stats / byte_fallback_tensor, `yttm ... --byte_fallback`),
shared by the emulator tests (test_bytefb_device.py, test_bytefb_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests
(test_gpu_bytefb.py: torch tensors).

Two yardsticks that share no code with the pass or with each other:
  1. the rule of include/yttm_mi355x.h in Python (want_rows): the sentence's code points classified against the alphabet parsed from the model
     file, the runs cut, V + b spliced into the setting-off ids of the same call; every id and offset is compared exactly;
  2. the round trip (check_round_trip): for valid UTF-8 whose words are separated by single ASCII spaces, without leading or trailing white space
     and without U+2581, decode(encode(s)) with the setting on equals s byte for byte, whatever the alphabet (models with the default special
     ids only).
Every case that is not trivial asserts from the rule that at least one unk_id of its input is replaced by two or more ids."""
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
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 64
SEG = 508  # ids a wavefront stages at once (k_restrict.h RST_SEG)
NOT_SET = "byte_fallback_ids_device: byte fallback is not set"
NO_SPANS = "spans are not defined under byte fallback"
PROBES = ["aé€😀b", "😀😀"]  # (U+1F600 is in no golden alphabet)


def probes():
    """the fixed probe words: two of them, and one word each of the Russian and the Japanese training text"""
    out = list(PROBES)
    for name in ("manual_ru", "manual_ja"):
        text = open(os.path.join(G, f"train_{name}.txt"), "rb").read().decode()
        out.append(next(w for w in text.split() if len(w) >= 2))
    return out


# ---- yardstick 1: the rule -----------------------------------------------------------------------------------------------------------------------
def is_space(cp):
    return cp == 0x2581 or cp == 32 or 9 <= cp <= 13


def valid_chars(raw):
    """(code point, its bytes) of every valid char of a byte string; an invalid byte is dropped, one at a time"""
    i, n = 0, len(raw)
    while i < n:
        b0 = raw[i]
        ln = 1 if b0 < 0x80 else 2 if b0 >> 5 == 6 else 3 if b0 >> 4 == 14 else 4 if b0 >> 3 == 30 else 0
        ch = None
        if ln and i + ln <= n:
            try:
                ch = raw[i:i + ln].decode()
            except UnicodeDecodeError:
                ch = None
        if ch is None or len(ch) != 1:
            i += 1
            continue
        yield ord(ch), raw[i:i + ln]
        i += ln


def runs_of(raw, alphabet):
    """the valid bytes of every maximal run of valid non-space code points outside the alphabet; invalid bytes do not end a run"""
    runs, cur = [], b""
    for cp, bs in valid_chars(raw):
        if not is_space(cp) and cp not in alphabet:
            cur += bs
            continue
        if cur:
            runs.append(cur)
        cur = b""
    if cur:
        runs.append(cur)
    return runs


def want_row(row, raw, V, unk, alphabet, rev):
    runs = runs_of(raw, alphabet)
    out, k = [], 0
    for t in (row[::-1] if rev else row):
        if t == unk:
            out.extend(V + b for b in runs[k]) if k < len(runs) else out.append(t)
            k += 1
        else:
            out.append(t)
    return out[::-1] if rev else out


def want_rows(rows, raws, V, unk, alphabet, rev):
    assert len(rows) == len(raws)
    return [want_row(r, s, V, unk, alphabet, rev) for r, s in zip(rows, raws)]


def splits(rows, want):
    """the condition on a non-trivial case: some unk_id became two or more ids (the rule replaces one id by a run's bytes: a longer row shows it)"""
    return any(len(w) > len(r) for r, w in zip(rows, want))


class Model:
    def __init__(self, name):
        self.name, self.path = name, model_path(name)
        self.alphabet = SW.alphabet_of(self.path)
        a = model_args(name) if os.path.sep not in name else {"unk": 1, "bos": 2, "eos": 3, "pad": 0}
        self.unk, self.args = a["unk"], a
        self.default_ids = (a["pad"], a["unk"], a["bos"], a["eos"]) == (0, 1, 2, 3)

    def core(self, on=True):
        c = D.core_of(self.path)
        if on:
            c.set_byte_fallback(True)
        return c

    def flags(self):
        return [f for f in FLAGS if (not f[0] or self.args["bos"] != -1) and (not f[1] or self.args["eos"] != -1)]


# ---- the device path ---------------------------------------------------------------------------------------------------------------------------
class PlacedText:
    """bytes at an address = align (mod 16) inside a larger buffer of guard bytes "Z" (outside every golden alphabet: a guard that is read
    lengthens a run)"""

    def __init__(self, B, data, align):
        self.B, self.n = B, len(data)
        host = np.full(GUARD + 16 + self.n + GUARD, ord("Z"), np.uint8)
        self.buf = B.put(host)
        self.start = GUARD + (align - (B.ptr(self.buf) + GUARD)) % 16
        host[self.start:self.start + self.n] = np.frombuffer(bytes(data), np.uint8)
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


def stats(core):
    return np.array(core.byte_fallback_stats(), np.int64)


def dev_bytefb(core, B, rows, raws, rev=0, shift=0, align=0, guard=1):
    """yttm_byte_fallback_ids_device on ids placed at `shift` between guard ids (unk_id: a guard that is read takes a run) and text at `align`
    between guard bytes: the rows of the pending result, taken by both exits (which check the two ids behind the result against a guard); the
    inputs and their guards stay as they were; the counters move by this call, and the write pass is never skipped on this entry"""
    flat, off = D.flatten(rows)
    blob, soff = K.pack(raws)
    P, T = RS.PlacedIds(B, flat, shift, guard), PlacedText(B, blob, align)
    d_off, d_soff = B.put(off), B.put(soff)
    before = stats(core)
    n_out, ms = core.byte_fallback_ids_device_raw(P.ptr, B.ptr(d_off), T.ptr, B.ptr(d_soff), len(rows), len(flat), len(blob), bool(rev))
    assert P.intact() and T.intact(), "an input or its guard values were written"
    assert B.get(d_off).view(np.uint64).tolist() == off.tolist() and B.get(d_soff).view(np.uint64).tolist() == soff.tolist(), "offsets were written"
    ids, o = K.take_encoded(core, B, len(rows), n_out)
    assert (stats(core) - before).tolist() == [1, 0, len(flat), n_out] and ms >= 0
    return K.rows(ids, o)


def raw_bytefb(core, p_ids, p_off, p_text, p_soff, n_sent, n_ids, n_bytes, rev=0):
    n, err = C.c_uint64(7), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_byte_fallback_ids_device(core._h, C.c_void_p(p_ids), C.c_void_p(p_off), C.c_void_p(p_text), C.c_void_p(p_soff), n_sent, n_ids, n_bytes,
                                                   rev, C.byref(n), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), n.value


def same(M, core, B, rows, sents, what, places=((0, 0),), revs=(0, 1), split=True):
    raws = to_bytes(sents)
    V = core.vocab_size()
    for rev in revs:
        want = want_rows(rows, raws, V, M.unk, M.alphabet, rev)
        if split:
            assert splits(rows, want), (what, "no unk_id becomes two or more ids: the case proves nothing")
        for shift, align in places:
            got = dev_bytefb(core, B, rows, raws, rev, shift, align, M.unk)
            if got != want:
                k = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
                raise AssertionError("%s rev %d shift %d align %d: sentence %d of %d differs: text %r in %r got %r want %r" % (
                    what, rev, shift, align, k, len(rows), raws[k][:40], rows[k][:12], got[k][:24], want[k][:24]))
        assert sum(map(len, want)) >= sum(map(len, rows)), (what, "an id was lost")


# ---- case 1: the pass on synthetic ids and text ------------------------------------------------------------------------------------------------
def check_synthetic(B, shifts=(0, 1, 5, 15), aligns=(0, 3, 8, 15), name="readme_small"):
    M = Model(name)
    core = M.core()
    V, U = core.vocab_size(), M.unk
    u = SW.unknown_chars(M.alphabet)  # {1: "Z", 2: "é", 3: "中", 4: "😀"}
    Kp, Kq = 10, V - 1
    mixed = u[1] + u[2] + u[3] + u[4]
    rng = np.random.RandomState(33)
    pairs = tuple(zip(shifts, aligns))
    # no sentence, empty sentences, one id, the sizes around a step
    assert dev_bytefb(core, B, [], [], 0, 1, 3, U) == [] and dev_bytefb(core, B, [], [], 1, 0, 0, U) == []
    same(M, core, B, [[], [], []], ["", "", ""], "empty only", split=False)
    same(M, core, B, [[], [], [U], [], []], ["", " ", mixed, "a", ""], "empty around one", places=pairs)
    for n in (1, 63, 64, 65):
        row = [Kp] * n
        row[n // 2] = U
        same(M, core, B, [row], ["ab " + u[2] + u[3] + " ba"], ("n", n), places=pairs[:2])
    # unk_ids at lanes 0 and 63 of a step, and on both sides of a step's edge
    for at in ((0,), (63,), (0, 63), (63, 64), (64,), (127, 128)):
        row = [Kp] * 130
        for a in at:
            row[a] = U
        text = " ab ".join(u[1 + (a % 4)] * 2 + u[3] for a in at)
        same(M, core, B, [row], [text], ("lanes", at), places=pairs[:2])
    # sentence boundaries inside a step, next to runs; more than 63 boundaries in one step
    rows = [[U, Kp, U], [U], [Kp] * 58 + [U], [U], [U, Kp] * 35, [], [Kp]]
    sents = [u[2] + " a " + u[4], u[3], "ab " + mixed, u[1], " ".join(u[1 + j % 4] + "a" for j in range(35)), "", "a"]
    same(M, core, B, rows, sents, "boundaries in a step", places=[(s, a) for s in shifts for a in aligns])
    rows = [[U] if i % 3 == 0 else [] if i % 3 == 1 else [Kp] for i in range(400)]
    sents = [u[1 + i % 4] if i % 3 == 0 else "" if i % 3 == 1 else "a" for i in range(400)]
    same(M, core, B, rows, sents, "many boundaries", places=pairs[:2])
    # runs of 1-, 2-, 3- and 4-byte chars, each alone and together
    same(M, core, B, [[Kp, U, Kq]] * 5, ["a " + c * 3 + " b" for c in u.values()] + [mixed], "char widths")
    # a run of ONE ASCII byte as the only unknown of the batch: the total stays, the id does not (dev_bytefb: the write pass ran)
    got = dev_bytefb(core, B, [[Kp, U, Kq], [Kp]], [b"a Z b", b"ab"], 0, 1, 5, U)
    assert got == [[Kp, V + ord("Z"), Kq], [Kp]]
    same(M, core, B, [[Kp, U, Kq], [Kp]], ["a Z b", "ab"], "one ASCII byte", split=False)
    # ... and through the encoder, where the pass may skip its write: it must not, on the strength of an unchanged total
    before = stats(core)
    base = encode_rows(M.core(False), B, [b"ab Z ab", b"ab"], 0, 0, 0)[0]
    got = encode_rows(core, B, [b"ab Z ab", b"ab"], 0, 0, 0)[0]
    n = sum(map(len, base))
    assert got == want_rows(base, [b"ab Z ab", b"ab"], V, U, M.alphabet, 0) and got != base and sum(map(len, got)) == n
    assert (stats(core) - before).tolist() == [1, 0, n, n]
    # invalid bytes in front of, inside and behind a run
    bad = SW.invalid_run_sentences()
    rows = [[Kp] + [U, Kq] * len(runs_of(s, M.alphabet)) for s in bad]
    assert all(len(r) > 1 for r in rows)
    same(M, core, B, rows, bad, "invalid bytes", places=pairs[:2])
    # a run that crosses the 64-byte text step: every shift 0 .. 130 of one tail against the step
    tail = " " + mixed * 3 + "Z a"
    same(M, core, B, [[Kp, U, Kq]] * 131, ["a" * k + tail for k in range(131)], "tail shifts", places=pairs[:2])
    # runs of exactly 64, 65, 508, 509 and 3000 valid bytes, as the lane's copy, the runs of lanes and the wavefront's copy take them
    longs = {64: u[2] * 32, 65: u[2] * 32 + "Z", 508: u[4] * 127, 509: u[4] * 127 + "Z", 3000: u[3] * 1000}
    assert all(len(s.encode()) == n for n, s in longs.items())
    for n, s in longs.items():
        sents = ["ab " + s + " ba", s, s + " " + s, b"Z\x80" + s.encode() + b"\xff " + s.encode()[:-1] + b"\xc3"]
        rows = [[Kp, U, Kq], [U], [U, U], [U, Kp, U]]
        same(M, core, B, rows, sents, ("run bytes", n), places=pairs[1:3])
    same(M, core, B, [[U] * 64, [Kp, U] * 40], [" ".join([u[2] * 8] * 64), " ".join([u[3] * 21 + "Z"] * 40)], "a step beyond a segment")
    same(M, core, B, [[Kp] * 56 + [U] * 8, [U] + [Kp] * 63 + [U]], [" ".join([longs[64]] * 7 + [longs[65]]), longs[3000] + " a " + longs[509]], "long behind a full tile")
    # a 3000-byte run on every wavefront of a workgroup: sentences of more than 256 ids are a group each
    rows = [[U] + [Kp] * 300, [Kp] * 300 + [U], [Kp] * 150 + [U] + [Kq] * 150, [U, Kp] * 3 + [Kp] * 300] * 2
    sents = [longs[3000], "a " + longs[3000], "b " + u[1] * 3000, " ".join([longs[3000], u[4], longs[509]])] * 2
    same(M, core, B, rows, sents, "long runs on every wave", places=pairs[2:3])
    # 300 runs in one sentence: beyond the directory
    same(M, core, B, [[U, Kp] * 300, [Kp] + [U] * 300], [" ".join(u[1 + j % 4] * (1 + j % 3) for j in range(300))] * 2, "300 runs", places=pairs[:2])
    # bos / eos and ids out of range mixed in
    odd = [-1, I32_MIN, I32_MAX, V, V + 7, V + 255, V + 256, -77]
    same(M, core, B, [[2, Kp, U, 3], odd + [U] + odd, [o for x in odd for o in (x, U)], [V]],
         ["a " + mixed, mixed, " ".join(c * 2 for c in mixed * 2), "a"], "special and out of range", places=pairs[:2])
    # an unk_id without a run stays, a run without an unk_id is ignored
    same(M, core, B, [[U, Kp, U, U, Kq, U], [Kp], [U, U], [Kp, U]], [u[3] + " a " + u[2], mixed + " a " + u[1], "ab", u[4] + " " + u[1] + " " + u[2]],
         "more unk_ids than runs and fewer")
    # 1 500 sentences over several workgroups
    pool = ["", "a", "ab " + u[1], u[2] + u[3], "ab", mixed + " ab " + u[4], " ", "b" * 9, "ab" + u[1] + u[3] + " d", u[4] * 20]
    sents = [pool[i] for i in rng.randint(0, len(pool), size=1500)]
    rows = [[int(t) for t in rng.choice([U, Kp, Kq, U, 7], size=n)] for n in rng.randint(0, 40, size=1500)]
    same(M, core, B, rows, sents, "many groups")
    # an encoder that never had the setting on has counted nothing
    assert stats(M.core(False)).tolist() == [0, 0, 0, 0]


# ---- case 2: the wired routes ---------------------------------------------------------------------------------------------------------------------
def encode_rows(core, B, raw, b, e, r, dropout=0.0):
    return RS.encode_rows(core, B, raw, b, e, r, dropout)


def batch_of(name, most=40):
    return sentences_of(name, most) + [" ".join(probes()), "ab " + PROBES[0], PROBES[1] + " " + PROBES[0] + " " + PROBES[1], ""]


def check_routes_model(B, name):
    """yttm_encode_device + both exits under every flag set, with the word cache forced on and off; the counters; the round trip; switching off"""
    M = Model(name)
    plain, core = M.core(False), M.core()
    V = core.vocab_size()
    raw = to_bytes(batch_of(name))
    for f in M.flags():
        base = encode_rows(plain, B, raw, *f)[0]
        want = want_rows(base, raw, V, M.unk, M.alphabet, f[2])
        assert splits(base, want), (name, f)
        assert all(M.unk not in w for w in want), "every unk_id of an encode has its run"
        for cache in (1, 0):
            core.set_cache(cache)
            before = stats(core)
            got, ms = encode_rows(core, B, raw, *f)
            assert got == want, (name, f, cache, next((g, w) for g, w in zip(got, want) if g != w))
            assert ms >= 0 and (stats(core) - before).tolist() == [1, 0, sum(map(len, base)), sum(map(len, want))]
        core.set_cache(2)
    # nothing unknown: the write pass is skipped and the ids are the parent's
    known = [s for s in raw if s and not runs_of(s, M.alphabet)][:20]
    if known:
        base = encode_rows(plain, B, known, 0, 0, 0)[0]
        before = stats(core)
        assert encode_rows(core, B, known, 0, 0, 0)[0] == base and M.unk not in [t for r in base for t in r]
        n = sum(map(len, base))
        assert (stats(core) - before).tolist() == [1, 1, n, n], (name, "the write pass ran for nothing")
    if M.default_ids:
        check_round_trip(core, B, name)
    # switching the setting off restores the parent's ids exactly, and counts no call
    core.set_byte_fallback(False)
    before = stats(core)
    for f in M.flags():
        assert encode_rows(core, B, raw, *f)[0] == encode_rows(plain, B, raw, *f)[0]
    assert (stats(core) - before).tolist() == [0, 0, 0, 0] and not core.byte_fallback()


def normalised(sents):
    """yardstick 2's inputs: valid UTF-8, words separated by single ASCII spaces, no leading or trailing white space, no U+2581"""
    out = []
    for s in sents:
        s = s if isinstance(s, str) else s.decode(errors="ignore")
        out.append(" ".join(s.replace("▁", " ").split()))
    return out


def check_round_trip(core, B, name):
    """decode(encode(s)) == s byte for byte: on the device, on the host, whatever the alphabet"""
    sents = normalised(batch_of(name)) + ["😀", "a😀", "😀a", "Ω 中 é"]
    raw = to_bytes(sents)
    rows = encode_rows(core, B, raw, 0, 0, 0)[0]
    flat, off = D.flatten(rows)
    dev, host = D.dev_decode(core, B, flat, off), D.host_decode(core, flat, off)
    assert dev[0] == 0 and host[0] == 0, (dev[:2], host[:2])
    o = [int(x) for x in dev[3]]
    assert [dev[2][o[i]:o[i + 1]] for i in range(len(raw))] == raw, (name, "device round trip")
    assert host[2] == dev[2] and host[3].tolist() == dev[3].tolist(), (name, "host decode")
    rev = encode_rows(core, B, raw, 0, 0, 1)[0]
    assert [r[::-1] for r in rev] == rows


def check_dropout(B, name="readme_small"):
    """two fresh encoders under one pinned salt draw alike call by call: the one with the setting on gives the rule's ids of the other's"""
    M = Model(name)
    raw = to_bytes(batch_of(name))
    with DC.env():
        a, b = M.core(False), M.core()
    V = a.vocab_size()
    none = encode_rows(a, B, raw, 0, 0, 0)[0]
    assert encode_rows(b, B, raw, 0, 0, 0)[0] == want_rows(none, raw, V, M.unk, M.alphabet, 0)
    for p in (0.1, 1.0):
        for f in ((0, 0, 0), (1, 1, 1)):
            rows = encode_rows(a, B, raw, *f, dropout=p)[0]
            want = want_rows(rows, raw, V, M.unk, M.alphabet, f[2])
            assert splits(rows, want) and (f != (0, 0, 0) or rows != none)
            assert encode_rows(b, B, raw, *f, dropout=p)[0] == want, (p, f)


def check_with_vocabulary(B, name="readme_small"):
    """a restricted vocabulary and the byte fallback together: the result equals both compositions of the two rules"""
    M = Model(name)
    plain, core = M.core(False), M.core()
    V = core.vocab_size()
    R = RS.Rules(M.path, V)
    raw = to_bytes(batch_of(name))
    for mname in ("none", "odd"):
        allowed = R.masks()[mname]
        E = R.table(allowed)
        core.set_vocabulary(allowed)
        for f in M.flags():
            base = encode_rows(plain, B, raw, *f)[0]
            a = want_rows(RS.want_rows(E, base, f[2]), raw, V, M.unk, M.alphabet, f[2])
            b = RS.want_rows(E, want_rows(base, raw, V, M.unk, M.alphabet, f[2]), f[2])
            assert a == b and a != base and splits(base, want_rows(base, raw, V, M.unk, M.alphabet, f[2]))
            assert encode_rows(core, B, raw, *f)[0] == a, (mname, f)


def check_python_routes(B, name="readme_small"):
    """BPE.encode(list) in both output types, the names, yttm_subword_device against the host loop, the decodes, the counts, the spans' refusal"""
    import pytest
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    V = bpe.vocab_size()
    assert bpe.byte_fallback() is None and bpe.byte_fallback_stats() == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        bpe.id_to_subword(V)
    assert bpe.subword_to_id("<0x41>") == M.unk
    bpe.set_byte_fallback()
    assert bpe.byte_fallback() == V and bpe.vocab_size() == V and bpe.vocab() == plain.vocab()
    sents = batch_of(name)
    raw = to_bytes(sents)
    base = plain.encode(sents, bos=True)
    want = want_rows(base, raw, V, M.unk, M.alphabet, 0)
    assert splits(base, want)
    got = bpe.encode(sents, bos=True)
    assert got == want
    assert bpe.encode(sents, bos=True, reverse=True) == [r[::-1] for r in want]
    assert bpe.decode(bpe.encode(normalised(sents))) == normalised(sents)
    # names
    for b in (0, 0x0A, 0x41, 0xE2, 0xFF):
        assert bpe.id_to_subword(V + b) == "<0x%02X>" % b and bpe.subword_to_id("<0x%02X>" % b) == V + b
    assert bpe.subword_to_id("<0xe2>") == M.unk and bpe.subword_to_id("<0x100>") == M.unk
    with pytest.raises(ValueError, match="id must be in the range"):
        bpe.id_to_subword(V + 256)
    # SUBWORD pieces: a byte id prints as <0xNN>, one piece each; the device formatter is the host loop byte for byte
    pieces = bpe.encode(sents, output_type=yttm.OutputType.SUBWORD)
    ids = bpe.encode(sents)
    vocab = bpe.vocab()
    for ps, row in zip(pieces, ids):
        assert ps == [vocab[t] if t < V else "<0x%02X>" % (t - V) for t in row]
    for f in M.flags():
        lines, rows = SW.same(bpe.bpe_cython, B, sents, *f, what=("SUBWORD", f))
        assert rows == want_rows(plain.encode(sents, bos=bool(f[0]), eos=bool(f[1]), reverse=bool(f[2])), raw, V, M.unk, M.alphabet, f[2])
        assert b"<0xF0> <0x9F> <0x98> <0x80> " in b"".join(lines) or f[2]
    # decode: ignore_ids naming byte ids; ids beyond the byte ids keep the message; made-up byte ids come out verbatim
    core = bpe.bpe_cython
    row = [t for r in ids for t in r]
    drop = sorted({t for t in row if t >= V})[:3]
    assert drop
    made_up = [row, [V + 0xC3], [V + 0x41, 5, V + 0xFF]]
    flat, off = D.flatten(made_up)
    dev, host = D.dev_decode(core, B, flat, off, drop), D.host_decode(core, flat, off, drop)
    assert dev[0] == 0 and dev[2] == host[2] and dev[3].tolist() == host[3].tolist()
    kept = D.host_decode(core, *D.flatten([[t for t in r if t not in drop] for r in made_up]))
    assert kept[0] == 0 and dev[2] == kept[2] and dev[2] != D.host_decode(core, flat, off)[2]
    o = [int(x) for x in dev[3]]
    assert dev[2][o[1]:o[2]] == b"\xc3" and dev[2][o[2]:].startswith(b"A") and dev[2].endswith(b"\xff")
    assert bpe.decode([[V + 0xC3]]) == ["\ufffd"]
    for bad in (V + 256, -1):
        flat, off = D.flatten([[5, bad]])
        off_msg = D.host_decode(plain.bpe_cython, flat, off)
        assert off_msg[0] == 1 and D.host_decode(core, flat, off)[:2] == off_msg[:2] and D.dev_decode(core, B, flat, off)[:2] == off_msg[:2]
    flat, off = D.flatten([[5, V]])
    assert D.dev_decode(plain.bpe_cython, B, flat, off)[0] == 1 and D.host_decode(plain.bpe_cython, flat, off)[0] == 1
    # counts: n_bins = 0 is V + 256 and the counts sum to the ids
    n_ids, _ = core.encode_device_raw(*_placed(B, raw), len(raw), sum(map(len, raw)), max(map(len, raw)), True, False, False, 0.0)
    nc, _ = core.id_counts_device_raw(len(raw))
    counts = core.fetch_id_counts()
    assert len(counts) == V + 257 and nc == n_ids == int(counts.sum()) and counts[V + 256] == 0
    assert counts.tolist() == np.bincount(np.array([t for r in want for t in r]), minlength=V + 257).tolist()
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
    assert D.encode_fetch(core, len(raw), n_ids)[0].tolist() == pending and core.fetch_id_counts().tolist() == counts.tolist()
    bpe.set_byte_fallback(False)
    assert bpe.encode(sents, bos=True) == base and len(bpe.encode_with_spans(sents)[0]) == len(sents)


_keep = []


def _placed(B, raw):
    blob, off = K.pack(raw)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    _keep[:] = [d_b, d_o]  # (alive until the next call)
    return B.ptr(d_b), B.ptr(d_o)


def check_blocks_and_batches(B, name="readme_small"):
    """blocks and batches of the pending result with byte ids in it, through their own property checkers"""
    import batches_checks as BA
    import blocks_checks as BL
    M = Model(name)
    core = M.core()
    raw = to_bytes(batch_of(name))
    V = core.vocab_size()
    plain_rows = encode_rows(M.core(False), B, raw, 1, 1, 0)[0]
    want = want_rows(plain_rows, raw, V, M.unk, M.alphabet, 0)
    assert splits(plain_rows, want)
    p_b, p_o = _placed(B, raw)
    n_ids, _ = core.encode_device_raw(p_b, p_o, len(raw), sum(map(len, raw)), max(map(len, raw)), True, True, False, 0.0)
    assert n_ids == sum(map(len, want))
    longest = max(map(len, want))
    ids, off = BL.pending_same(core, B, len(raw), n_ids, 64, BL.STREAM, BL.PAD, "blocks of byte ids, stream")
    assert K.rows(ids, off) == want
    BL.pending_same(core, B, len(raw), n_ids, longest + 1, BL.WHOLE, BL.KEEP, "blocks of byte ids, whole")
    BA.pending_same(core, B, len(raw), n_ids, longest + 3, M=5, left=True, what="batches of byte ids")


def check_files(B, tmp_path, name="readme_small"):
    """encode_file as ids, id text and SUBWORD at three piece sizes, count_file, and decode_file of encode_file = the normalised file"""
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    bpe.set_byte_fallback()
    V = bpe.vocab_size()
    lines = normalised(batch_of(name))
    data = "".join(s + "\n" for s in lines).encode()
    raw = to_bytes(lines)
    path, out, back = str(tmp_path / "in.txt"), str(tmp_path / "out.txt"), str(tmp_path / "back.txt")
    open(path, "wb").write(data)
    vocab = bpe.vocab()
    for b, e, r in ((0, 0, 0), (1, 1, 1)):
        ids, off = plain.encode_file(path, bos=b, eos=e, reverse=r)
        want = want_rows(K.rows(ids, off), raw, V, M.unk, M.alphabet, r)
        assert splits(K.rows(ids, off), want)
        flat = np.array([t for row in want for t in row], np.int64)
        for chunk in (None, max(len(data) // 8, 1), 1):
            g_ids, g_off = bpe.encode_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
            assert K.rows(g_ids, g_off) == want, (b, e, r, chunk)
            nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, id_text=True)
            assert (nl, ni) == (len(want), len(flat))
            assert open(out, "rb").read() == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want), (chunk, "id_text")
            if (b, e, r) == (0, 0, 0):
                bpe.decode_file(out, back, chunk_bytes=chunk)
                assert open(back, "rb").read() == data, (chunk, "decode_file of encode_file")
            nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, output_type=yttm.OutputType.SUBWORD)
            assert (nl, ni) == (len(want), len(flat))
            text = b"".join(b"".join((vocab[t] if t < V else "<0x%02X>" % (t - V)).encode() + b" " for t in row) + b"\n" for row in want)
            assert open(out, "rb").read() == text, (chunk, "SUBWORD")
            counts = bpe.count_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
            assert counts.tolist() == np.bincount(flat, minlength=V + 257).tolist(), (chunk, "counts")


# ---- case 3: errors --------------------------------------------------------------------------------------------------------------------------------
def check_errors(B, name="readme_small"):
    import pytest
    M = Model(name)
    core = M.core(False)
    ids, off = B.put(np.array([5, M.unk, 7], np.int32)), B.put(np.array([0, 3], np.uint64))
    text, soff = B.put(np.frombuffer(b"a Z b" + b"\0" * 16, np.uint8)), B.put(np.array([0, 5], np.uint64))
    args = (B.ptr(ids), B.ptr(off), B.ptr(text), B.ptr(soff), 1, 3, 5)
    # the pass with the setting off: code 1, and what was pending stays
    n = D.encode_device(core, B, [b"ab cd", b"Z"], 0, 0, 0)
    pending = D.encode_fetch(core, 2, n)[0].tolist()
    assert raw_bytefb(core, *args) == (1, NOT_SET, 0)
    assert D.encode_fetch(core, 2, n)[0].tolist() == pending and stats(core).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="byte fallback is not set"):
        core.byte_fallback_ids_device_raw(*args)
    # the setting while a result is pending does not change that result; the pass then replaces it and empties the spans slot
    sents = [b"ab Z cd", b"abcd " * 10]
    blob, so = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(so)
    n_ids, _ = core.spans_device_raw(B.ptr(d_b), B.ptr(d_o), 2, len(blob), max(map(len, sents)))
    before = D.encode_fetch(core, 2, n_ids)[0].tolist()
    core.set_byte_fallback(True)
    assert core.byte_fallback() and D.encode_fetch(core, 2, n_ids)[0].tolist() == before
    assert core.fetch_spans(2, n_ids).shape == (n_ids, 2)
    assert raw_bytefb(core, *args) == (0, "", 3)
    assert D.encode_fetch(core, 1, 3)[0].tolist() == [5, core.vocab_size() + ord("Z"), 7]
    with pytest.raises(ValueError, match="fetch_spans: no matching result"):
        core.fetch_spans(1, 3)
    assert raw_bytefb(core, B.ptr(ids) + 2, *args[1:])[0] == 2  # a misaligned address
    assert raw_bytefb(core, args[0], 0, *args[2:])[0] == 2 and raw_bytefb(core, *args[:3], 0, *args[4:])[0] == 2  # no offsets


# ---- case 4: the command line ---------------------------------------------------------------------------------------------------------------------
def check_cli(tmp_path, name="readme_small"):
    """--byte_fallback on encode, encode_file, count_file, decode and decode_file, and a vocabulary file written with the flag.  Seven processes."""
    import youtokentome_amd as yttm
    M = Model(name)
    plain = yttm.BPE(M.path)
    V = plain.vocab_size()
    lines = normalised(batch_of(name))
    data = "".join(s + "\n" for s in lines).encode()
    path, voc, out = str(tmp_path / "in.txt"), str(tmp_path / "voc.tsv"), str(tmp_path / "out.txt")
    open(path, "wb").write(data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def run(args, stdin=None):
        p = subprocess.run(cli + args, capture_output=True, env=env, input=stdin)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    want = want_rows(plain.encode(lines), to_bytes(lines), V, M.unk, M.alphabet, 0)
    assert splits(plain.encode(lines), want)
    text = b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want)
    assert run(["encode", f"--model={M.path}", "--output_type=id", "--byte_fallback"], stdin=data) == text
    assert run(["decode", f"--model={M.path}", "--byte_fallback"], stdin=text) == data
    sub = run(["encode", f"--model={M.path}", "--output_type=subword", "--byte_fallback"], stdin=data)
    assert b"<0xF0> <0x9F> <0x98> <0x80> " in sub and b"<UNK>" not in sub
    run(["encode_file", f"--model={M.path}", f"--input={path}", f"--output={out}", "--output_type=id_text", "--byte_fallback"])
    assert open(out, "rb").read() == text
    run(["decode_file", f"--model={M.path}", f"--input={out}", f"--output={out}.txt", "--byte_fallback"])
    assert open(out + ".txt", "rb").read() == data
    run(["count_file", f"--model={M.path}", f"--input={path}", f"--output={voc}", "--byte_fallback"])
    rows = [ln.split(b"\t") for ln in open(voc, "rb").read().split(b"\n")[:-1]]
    assert len(rows) == V + 256 and [int(r[2]) for r in rows] == np.bincount(np.array([t for r in want for t in r]), minlength=V + 256).tolist()
    assert all(rows[V + b][1] == b"<0x%02X>" % b for b in range(256))
    # that file as --vocabulary: its byte rows are accepted and otherwise ignored
    R = RS.Rules(M.path, V)
    counts = np.array([int(r[2]) for r in rows[:V]])
    E = R.table(counts >= 2)
    got = run(["encode", f"--model={M.path}", "--output_type=id", "--byte_fallback", f"--vocabulary={voc}", "--vocabulary_threshold=2"], stdin=data)
    assert got == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in RS.want_rows(E, want, 0))


# ---- case 5: torch tensors (MI355X) ---------------------------------------------------------------------------------------------------------------
def check_tensor_api(name="readme_small"):
    import pytest
    import torch
    import youtokentome_amd as yttm
    M = Model(name)
    plain, bpe = yttm.BPE(M.path), yttm.BPE(M.path)
    V = bpe.vocab_size()
    dev = torch.device("cuda", bpe.bpe_cython.device)
    sents = batch_of(name)
    raw = to_bytes(sents)
    p_ids, p_off = plain.encode_tensor(sents, bos=True, padded=False)
    base = K.rows(p_ids.cpu().numpy(), p_off.cpu().numpy())
    with pytest.raises(ValueError, match="byte fallback is not set"):
        bpe.byte_fallback_tensor(p_ids, sents, offsets=p_off)
    bpe.set_byte_fallback()
    want = want_rows(base, raw, V, M.unk, M.alphabet, 0)
    assert splits(base, want)
    ids, off = bpe.encode_tensor(sents, bos=True, padded=False)
    assert ids.dtype == torch.int32 and ids.device == dev and K.rows(ids.cpu().numpy(), off.cpu().numpy()) == want
    m, lengths = bpe.encode_tensor(sents, bos=True, pad_id=V + 300)
    assert m.shape[1] == max(map(len, want))
    for i, row in enumerate(want):
        assert m[i, :int(lengths[i])].tolist() == row and set(m[i, int(lengths[i]):].tolist()) <= {V + 300}
    assert bpe.id_counts_tensor().cpu().numpy().tolist() == np.bincount(np.array([t for r in want for t in r]), minlength=V + 257).tolist()
    # ids this object did not encode: ragged, padded with lengths, reversed; a second pass changes nothing (no unk_id is left)
    r_ids, r_off = bpe.byte_fallback_tensor(p_ids, sents, offsets=p_off)
    assert torch.equal(r_ids, ids) and torch.equal(r_off, off)
    r2, o2 = bpe.byte_fallback_tensor(r_ids, sents, offsets=r_off)
    assert torch.equal(r2, ids) and torch.equal(o2, off)
    pm, pl = plain.encode_tensor(sents, bos=True, pad_id=0)
    rm, rl = bpe.byte_fallback_tensor(pm, sents, lengths=pl, pad_id=V + 300)
    assert torch.equal(rm, m) and torch.equal(rl, lengths)
    q_ids, q_off = plain.encode_tensor(sents, bos=True, reverse=True, padded=False)
    rr, ro = bpe.byte_fallback_tensor(q_ids, sents, offsets=q_off, reverse=True)
    assert K.rows(rr.cpu().numpy(), ro.cpu().numpy()) == [r[::-1] for r in want]
    # the text back, as str and as bytes on the device
    norm = normalised(sents)
    n_ids, n_off = bpe.encode_tensor(norm, padded=False)
    assert bpe.decode_tensor(n_ids, offsets=n_off) == norm
    with pytest.raises(ValueError, match=NO_SPANS):
        bpe.encode_spans_tensor(sents)
    bpe.set_byte_fallback(False)
    assert torch.equal(bpe.encode_tensor(sents, bos=True, padded=False)[0], p_ids)


# ---- case 6: one larger pass (MI355X) ---------------------------------------------------------------------------------------------------------------
def check_large(B, name="zipf", n=50_000, width=128, frac=0.01):
    """50 000 x 128 chars with 1 % of the chars outside the alphabet: the rule as array operations on the setting-off ids of the same text"""
    import gen
    M = Model(name)
    plain, core = M.core(False), M.core()
    V = core.vocab_size()
    u = SW.unknown_chars(M.alphabet)
    rawtext = gen.zipf_corpus_fast(n * width + 4096, seed=23, vocab=20000).replace(b"\n", b" ")[:n * width]
    cps = np.frombuffer(rawtext, np.uint8).astype("<u4")
    rng = np.random.default_rng(5)
    hit = rng.random(len(cps)) < frac
    cps[hit] = rng.choice(np.array([ord(c) for c in u.values()], "<u4"), size=int(hit.sum()))
    text = cps.tobytes().decode("utf-32-le")
    sents = [text[i * width:(i + 1) * width].encode() for i in range(n)]
    blob, soff = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(soff)
    longest = max(map(len, sents))
    # the runs in text order: a run starts at an unknown char that opens its sentence or whose predecessor is not one (all chars are valid)
    known = np.array(sorted(M.alphabet | {32, 9, 10, 11, 12, 13, 0x2581}), "<u4")
    unknown = ~np.isin(cps, known)
    first = unknown & (~np.concatenate(([False], unknown[:-1])) | (np.arange(len(cps)) % width == 0))
    char_bytes = 1 + (cps >= 0x80).astype(np.int64) + (cps >= 0x800) + (cps >= 0x10000)
    run_len = np.bincount((np.cumsum(first) - 1)[unknown], weights=char_bytes[unknown], minlength=int(first.sum())).astype(np.int64)
    run_bytes = np.frombuffer("".join(text[i] for i in np.flatnonzero(unknown)).encode(), np.uint8).astype(np.int64)
    assert len(run_bytes) == int(run_len.sum()) and int(unknown.sum()) > n * width * frac / 2
    for b, e, r in ((0, 0, 0), (1, 1, 1)):
        ni, _ = plain.encode_device_raw(B.ptr(d_b), B.ptr(d_o), n, len(blob), longest, bool(b), bool(e), bool(r), 0.0)
        ids, off = plain.fetch_encode(n, ni)
        is_unk = ids == M.unk
        assert int(is_unk.sum()) == len(run_len), "every unk_id of the encode stands for one run"
        fwd = np.concatenate([ids[int(off[i]):int(off[i + 1])][::-1] for i in range(n)]) if r else ids
        lens = np.ones(len(fwd), np.int64)
        lens[fwd == M.unk] = run_len  # (forward order: the k-th unk_id of the batch is its k-th run)
        start = np.zeros(len(fwd) + 1, np.int64)
        np.cumsum(lens, out=start[1:])
        want = np.repeat(fwd.astype(np.int64), lens)
        want[np.repeat(fwd == M.unk, lens)] = V + run_bytes
        w_off = start[off.astype(np.int64)]
        if r:
            want = np.concatenate([want[int(w_off[i]):int(w_off[i + 1])][::-1] for i in range(n)])
        assert len(want) > len(ids)
        n2, _ = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), n, len(blob), longest, bool(b), bool(e), bool(r), 0.0)
        got, g_off = core.fetch_encode(n, n2)
        assert n2 == len(want) and np.array_equal(got, want.astype(np.int32)), (b, e, r)
        assert np.array_equal(g_off.astype(np.int64), w_off), (b, e, r, "offsets")
        if not r:  # the text back from the device decode
            d_ids, d_off = B.put(got), B.put(g_off)
            nb, _ = core.decode_device_raw(B.ptr(d_ids), B.ptr(d_off), n, n2, (2, 3))
            back = core.fetch_decode(n, nb)
            assert bytes(back[0]) == b"".join(" ".join(s.decode().split()).encode() for s in sents), "round trip"
