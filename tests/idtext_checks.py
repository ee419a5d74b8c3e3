"""Checks of decimal id text on the device -- the parser (yttm_ids_parse_device, yttm_decode_text_device, yttm_decode_file) and the printer
(yttm_idtext_device, yttm_encode_file_idtext) of k_idtext.h -- and of the commands on top, shared by the emulator tests (test_idtext_device.py,
test_idtext_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests (test_gpu_idtext.py: torch tensors).

Yardsticks, none of them the code under test:
  1. ids and offsets: py_parse, a Python parser written from the rule of `while (ss >> x) ids.push_back(x)` in the C locale (WS = 0x20, 0x09 ..
     0x0D; a number is a maximal digit run, negated iff the byte before it is '-'; a line ends at its first fail point: another byte, a sign
     whose next byte in the line is no digit, a number outside int32);
  2. decoded text: yttm_decode_cli through its in_fd / out_fd on the same bytes (the only route before), and BPE.decode;
  3. printed ids: yttm_encode_cli(output_type = "id") on the same text;
  4. on the CPU run, where the compiled reference is present: `yttm_ref decode` (empty ignore set) and `yttm_ref encode ... id` on the same files.
Equality is exact everywhere: ids, offsets, bytes, messages.  Every text sits at a chosen address alignment between guard bytes (lines_checks.Placed)."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import refbin
import subword_checks as S
from decode_checks import G, NumpyBuf, TorchBuf, golden_names, golden_sentences, model_args  # noqa: F401  (the buffers are re-exported)
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = b" \t\n\v\f\r"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ALL = tuple(range(16))


# ---- yardstick 1: the rule --------------------------------------------------------------------------------------------------------------
def py_parse_line(line):
    ids, i, n = [], 0, len(line)
    while i < n:
        b = line[i]
        if b in WS:
            i += 1
        elif 48 <= b <= 57:
            j = i
            while j < n and 48 <= line[j] <= 57:
                j += 1
            digits = line[i:j].lstrip(b"0")
            v = int(digits) if 0 < len(digits) <= 11 else 0 if not digits else 10 ** 11  # (longer than any int32: out of range, whatever it is)
            if i > 0 and line[i - 1] == 0x2D:
                v = -v
            if not I32_MIN <= v <= I32_MAX:
                break
            ids.append(v)
            i = j
        elif b in b"+-" and i + 1 < n and 48 <= line[i + 1] <= 57:
            i += 1
        else:
            break
    return ids


def py_parse(data):
    """-> (rows, flat int32 ids, uint64 offsets[n_lines + 1])"""
    rows = [py_parse_line(ln) for ln in K.py_split(data)]
    flat, off = D.flatten(rows)
    return rows, flat, off


def py_print(rows):
    return b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in rows)


# ---- yardsticks 2 and 3: the command line's loops ------------------------------------------------------------------------------------------
def _through_fds(call, data):
    with tempfile.TemporaryFile() as fi, tempfile.TemporaryFile() as fo:
        fi.write(bytes(data))
        fi.flush()
        os.lseek(fi.fileno(), 0, os.SEEK_SET)
        err = C.create_string_buffer(_lib.ERRLEN)
        rc = call(fi.fileno(), fo.fileno(), err)
        os.lseek(fo.fileno(), 0, os.SEEK_SET)
        out = b""
        while True:
            part = os.read(fo.fileno(), 1 << 24)
            if not part:
                break
            out += part
        return rc, err.value.decode(), out


def cli_decode(core, data, ignore=()):
    """yttm_decode_cli: (code, message, the bytes written before it stopped)"""
    a, ap, an = D._ign(ignore)
    return _through_fds(lambda i, o, err: _lib.load().yttm_decode_cli(core._h, ap, an, i, o, err, _lib.ERRLEN), data)


def cli_encode_ids(core, data, b=0, e=0, r=0):
    rc, msg, out = _through_fds(lambda i, o, err: _lib.load().yttm_encode_cli(core._h, b"id", 0, b, e, r, 0.0, i, o, err, _lib.ERRLEN), data)
    assert rc == 0, msg
    return out


# ---- the device paths ----------------------------------------------------------------------------------------------------------------------
def dev_parse(core, B, data, align=0):
    """yttm_ids_parse_device: (ids, offsets) by both exits; the lines' offsets are pending too; the text and its guard bytes stay"""
    P = K.Placed(B, data, align)
    n, n_ids, _ = core.ids_parse_device_raw(P.ptr, len(data))
    assert n == len(K.py_split(data))
    ids, off = K.take_encoded(core, B, n, n_ids)
    assert core.fetch_lines(n).tolist() == K.py_offsets(data).tolist()
    assert P.intact(), "the text or its guard bytes were written"
    return ids, off


def dev_decode_text(core, B, data, ignore=(), align=0):
    """yttm_decode_text_device: (code, message, text, line_off, n_lines, n_ids)"""
    L = _lib.load()
    P = K.Placed(B, data, align)
    a, ap, an = D._ign(ignore)
    nl, ni, nt, ms, err = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_decode_text_device(core._h, C.c_void_p(P.ptr), len(data), ap, an, C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN)
    assert P.intact(), "the text or its guard bytes were written"
    if rc != 0:
        return rc, err.value.decode(), None, None, nl.value, ni.value
    text, off = D._take_result(core, B, nl.value, nt.value)
    return 0, "", text, off, nl.value, ni.value


def dev_print(core, B, n):
    """yttm_idtext_device on the pending result of n sentences: (text, line_off)"""
    nt, _ = core.idtext_device_raw(n)
    return D._take_result(core, B, n, nt)


def outside(rows, vocab):
    return sorted({t for row in rows for t in row if not 0 <= t < vocab})


def check_one(core, B, data, aligns=ALL, what=""):
    """parse == the rule; decode_text == decode_cli, with every id outside the vocabulary ignored and (where there is one) with none ignored: the
    same message; print(parse) == the rule's text.  Returns the rows."""
    rows, flat, off = py_parse(data)
    vocab = core.vocab_size()
    ign = outside(rows, vocab)
    want_ok = cli_decode(core, data, ign)
    assert want_ok[0] == 0, (what, want_ok[1])
    want_bad = cli_decode(core, data) if ign else None
    assert want_bad is None or want_bad[0] == 1
    for a in aligns:
        ids, o = dev_parse(core, B, data, a)
        assert o.tolist() == off.tolist(), (what, a, K.rows(ids, o)[:5], rows[:5])
        assert ids.tolist() == flat.tolist(), (what, a)
        if a % 5 == 0:
            text, toff = dev_print(core, B, len(rows))
            assert text == py_print(rows), (what, a)
            assert toff.tolist() == np.cumsum([0] + [len(py_print([r])) for r in rows]).tolist()
        got = dev_decode_text(core, B, data, ign, a)
        assert got[:2] == (0, ""), (what, a, got[1])
        assert got[2] == want_ok[2], (what, a)
        lo = got[3].tolist()
        assert all(got[2][lo[i + 1] - 1:lo[i + 1]] == b"\n" for i in range(len(rows))) and (got[4], got[5]) == (len(rows), len(flat))
        if want_bad is not None:
            bad = dev_decode_text(core, B, data, (), a)
            assert bad[:2] == want_bad[:2], (what, a, bad[:2], want_bad[:2])
    return rows


def check_long_piece_lines(B, tmp_path, aligns=ALL):
    """newline mode of the decode's write kernel in front of, between and behind pieces longer than the staging tile, which the wavefront copies
    one by one: empty lines before, between and after such lines, and a last line without a newline == decode_cli, byte for byte"""
    import youtokentome_amd as yttm
    rng = random.Random(4)  # (the model of decode_checks.check_long_pieces, built the same way)
    word = "".join(rng.choice("abcdefgh") for _ in range(2300))
    corpus, model = str(tmp_path / "long.txt"), str(tmp_path / "long.model")
    open(corpus, "w").write((word + " xy ") * 6 + "ab cd\n")
    yttm.BPE.train(corpus, model, 4 + 11 + 2400, 1.0, 1, 0, 1, 2, 3)
    core = yttm.BPE(model).bpe_cython
    whole = core.subword_to_id("▁" + word)
    assert core.id_to_subword(whole) == "▁" + word, "the long word did not become one piece"
    data = b"\n%d\n5 %d %d 6\n\n\n%d 8" % (whole, whole, whole, whole)
    rc, msg, want = cli_decode(core, data)
    assert rc == 0 and want.count(word.encode()) == 4 and want.startswith(b"\n" + word.encode() + b"\n"), msg
    for a in aligns:
        got = dev_decode_text(core, B, data, (), a)
        assert got[:2] == (0, ""), (a, got[1])
        assert got[2] == want, (a, len(got[2]), len(want))
        assert (got[4], got[5]) == (6, 7) and got[3].tolist()[-1] == len(want)


# ---- cases 1 - 4: line structure, signs and glue, fail points, range ------------------------------------------------------------------------
def check_line_structure(B, aligns=ALL, name="readme_small"):
    core = D.core_of(name)
    expect = {b"": [], b"5 6 7\n": [[5, 6, 7]], b"5 6 7": [[5, 6, 7]], b"\n": [[]], b"\n\n\n": [[], [], []], b"5\n\n\n6\n\n": [[5], [], [], [6], []],
              b" \n\t\t\n \v\f\r \n": [[], [], []], b"  \n7": [[], [7]], b"5 6\r\n7\r\n\r\n8\r": [[5, 6], [7], [], [8]],
              b"1 2\t3\v4\f5\r6\n7": [[1, 2, 3, 4, 5, 6], [7]]}
    for data, want in expect.items():
        assert check_one(core, B, data, aligns, data) == want, data
    for sep in WS.replace(b"\n", b""):
        assert check_one(core, B, b"8" + bytes([sep]) + b"9" + bytes([sep]) + b"\n", aligns) == [[8, 9]]


def check_signs(B, aligns=ALL, name="readme_small"):
    core = D.core_of(name)
    expect = {b"+5": [5], b"-0": [0], b"1-2": [1, -2], b"1+2": [1, 2], b"1 - 2": [1], b"+-3": [], b"--3": [], b"5-": [5], b"+": [], b"-": [], b"7 +": [7],
              b"-5 6": [-5, 6], b"6 -5": [6, -5], b"+0012": [12], b"3+": [3], b"++1": [], b"-+1": [], b"1 -": [1], b"4 -\n5": None}
    for line, want in expect.items():
        for tail in (b"", b"\n", b"\n9\n"):
            if want is None:
                assert check_one(core, B, line + tail, aligns, line)[:2] == [[4], [5]]
                continue
            rows = check_one(core, B, line + tail, aligns, line)
            assert rows[0] == want and rows[1:] == ([[9]] if tail == b"\n9\n" else []), (line, tail, rows)
    # -5 ignored: the line decodes; not ignored: the error of the host path, naming -5
    for a in aligns:
        ok = dev_decode_text(core, B, b"6 -5 7\n", (-5,), a)
        assert ok[:3] == (0, "", cli_decode(core, b"6 -5 7\n", (-5,))[2]) and ok[2] == (core.decode([[6, 7]], None)[0] + "\n").encode()
        bad = dev_decode_text(core, B, b"6 -5 7\n", (), a)
        assert bad[0] == 1 and "-5" in bad[1] and bad[:2] == cli_decode(core, b"6 -5 7\n")[:2], bad


def check_fail_points(B, aligns=ALL, name="readme_small"):
    core = D.core_of(name)
    expect = {b"12abc 7": [12], b"abc": [], b"1.5 2": [1], b"0x10": [0], b"3 \x00 4": [3], b"\x00": [], b"3 \x80 4": [3], b"5\xff6": [5],
              "３ 4".encode(): [], "4 ５ 6".encode(): [4], b"7,8": [7], b"9 _": [9], b"1 2 3 x": [1, 2, 3], b"x 1 2 3": []}
    for line, want in expect.items():
        for tail in (b"", b"\n", b"\n8 9\n"):
            rows = check_one(core, B, line + tail, aligns, line)
            assert rows[0] == want and rows[1:] == ([[8, 9]] if tail == b"\n8 9\n" else []), (line, tail, rows)
    # nothing behind a fail point counts: 99999 is outside the vocabulary and raises nothing, the next line is untouched
    assert core.vocab_size() < 99999
    data = b"3 x 99999\n6\n"
    for a in aligns:
        ids, off = dev_parse(core, B, data, a)
        assert (ids.tolist(), off.tolist()) == ([3, 6], [0, 1, 2])
        got = dev_decode_text(core, B, data, (), a)
        assert got[:2] == (0, "") and got[2] == cli_decode(core, data)[2] and got[3].tolist()[0] == 0 and (got[4], got[5]) == (2, 2)


def check_range(B, aligns=ALL, name="readme_small"):
    core = D.core_of(name)
    expect = {b"2147483647 5": [I32_MAX, 5], b"-2147483648 5": [I32_MIN, 5], b"2147483648 5": [], b"-2147483649 5": [], b"4 2147483648 5": [4],
              b"+2147483647": [I32_MAX], b"+2147483648": [], b"4 " + b"9" * 23 + b" 5": [4], b"4 -" + b"9" * 23 + b" 5": [4],
              b"0000000000000000000007 5": [7, 5], b"-0000000000000000000007 5": [-7, 5], b"00000000002147483648": [], b"00000000002147483647": [I32_MAX],
              b"4294967296 1": [], b"4294967301 1": [], b"18446744073709551621 1": [], b"-4294967296": [], b"10000000000": [], b"9999999999": [],
              b"3 " + b"0" * 5000 + b"7 5": [3, 7, 5], b"3 -" + b"0" * 5000 + b"7 5": [3, -7, 5], b"3 " + b"9" * 5000 + b" 5": [3], b"3 -" + b"9" * 5000 + b" 5": [3],
              b"3 " + b"0" * 5000 + b"2147483648 5": [3], b"1" + b"0" * 5000: [], b"0" * 64 + b"5": [5], b"0" * 128: [0]}
    for line, want in expect.items():
        few = aligns if len(line) < 100 else aligns[:3]
        rows = check_one(core, B, line + b"\n6\n", few, line[:24])
        assert rows == [want, [6]], (line[:24], rows)


# ---- case 5: steps ------------------------------------------------------------------------------------------------------------------------------
STEP_LINES = [b"1234567 89", b"-77", b"5 -", b"x 31 32", b"1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29 30", b"+4", b"2147483647-2147483648",
              b"88"]


def step_text(shift, kind):
    """a prefix of `shift` bytes -- spaces of the first line, numbers of it, or a line of its own -- then the lines of STEP_LINES; the last one ends
    with the text"""
    if kind == 0:
        head = b" " * shift
    elif kind == 1:
        head = (b"1 " * shift)[:shift - 1] + b" " if shift else b""
    else:
        head = (b"1 " * shift)[:shift - 1] + b"\n" if shift else b""
    return head + b"\n".join(STEP_LINES)


def check_steps(B, aligns=ALL, shifts=range(131), name="readme_small"):
    """every shift of the lines' starts against the 64-byte step: a digit run, a sign and its digit, a fail point and the numbers behind it on
    either side of a step's end; a number that ends with the text"""
    core = D.core_of(name)
    tail = [[1234567, 89], [-77], [5], [], list(range(1, 31)), [4], [I32_MAX, I32_MIN], [88]]
    for shift in shifts:
        for kind in (0, 1, 2):
            data = step_text(shift, kind)
            rows, flat, off = py_parse(data)
            head_ids = [1] * (shift // 2) if kind else []
            assert rows == ([head_ids] + tail if kind == 2 and shift else [head_ids + tail[0]] + tail[1:]), (shift, kind)
            for a in (aligns if shift in (0, 1, 63, 64, 65) else (aligns[shift % len(aligns)],)):
                ids, o = dev_parse(core, B, data, a)
                assert o.tolist() == off.tolist() and ids.tolist() == flat.tolist(), (shift, kind, a)
    ign = [-77, I32_MAX, I32_MIN, 1234567]
    for shift in (0, 30, 61, 62, 63, 64, 127, 128):
        for kind in (0, 2):
            data = step_text(shift, kind)
            got = dev_decode_text(core, B, data, ign, shift % 16)
            assert got[:3] == cli_decode(core, data, ign), (shift, kind)


def check_groups(B, aligns=ALL, name="readme_small", big=100_000):
    """more than 64 short lines in a group next to one line of `big` ids; lines of 0 ... 5000 ids; thousands of empty lines"""
    core = D.core_of(name)
    vocab = core.vocab_size()
    rng = random.Random(11)
    long_line = b" ".join(b"%d" % rng.randrange(vocab) for _ in range(big))
    shorts = [b"%d" % (i % vocab) for i in range(9000)]
    data = b"\n".join(shorts[:4000] + [long_line] + shorts[4000:]) + b"\n"
    assert len(data) // 9001 < 4096 // 64, "the short lines would not share groups of more than 64 lines"
    rows, flat, off = py_parse(data)
    assert len(rows[4000]) == big
    want = cli_decode(core, data)
    for a in aligns:
        ids, o = dev_parse(core, B, data, a)
        assert o.tolist() == off.tolist() and ids.tolist() == flat.tolist(), a
    got = dev_decode_text(core, B, data, (), aligns[-1])
    assert got[:3] == want
    lens = (0, 1, 2, 63, 64, 65, 511, 512, 513, 5000)
    data = b"".join(b" ".join(b"%d" % rng.randrange(vocab) for _ in range(n)) + b"\n" for n in lens)
    assert [len(r) for r in check_one(core, B, data, aligns[:4], "lengths")] == list(lens)
    check_one(core, B, b"\n" * 3000 + b"5\n" + b"\n" * 70 + b"6", aligns[:4], "empty lines")
    check_one(core, B, b"7\n" * 5000, aligns[:4], "one-id lines")


# ---- case 6: random byte soup --------------------------------------------------------------------------------------------------------------------
SOUP = [b" ", b" ", b" ", b"\t", b"\v", b"\f", b"\r", b"+", b"-", b"a", b".", b"x", b"\x00", b"\x80", b"2147483647", b"2147483648", b"-2147483648", b"-2147483649",
        b"000000000000000000000042", b"9" * 23] + [b"%d" % d for d in range(10)] * 3


def soup_text(n_lines=20_000, seed=5):
    rng = random.Random(seed)
    return b"".join(b"".join(rng.choice(SOUP) for _ in range(rng.randrange(0, 14))) + b"\n" for _ in range(n_lines))


def check_soup(B, aligns=ALL, n_lines=20_000, name="readme_small"):
    core = D.core_of(name)
    data = soup_text(n_lines)
    rows, flat, off = py_parse(data)
    assert sum(1 for r in rows if r) > n_lines // 3 and len(flat) > n_lines // 2
    ign = outside(rows, core.vocab_size())
    want = cli_decode(core, data, ign)
    assert want[0] == 0
    want_bad = cli_decode(core, data)
    for a in aligns:
        ids, o = dev_parse(core, B, data, a)
        assert o.tolist() == off.tolist() and ids.tolist() == flat.tolist(), a
    for a in (aligns[0], aligns[-1]):
        assert dev_decode_text(core, B, data, ign, a)[:3] == want
        assert dev_decode_text(core, B, data, (), a)[:2] == want_bad[:2] and want_bad[0] == 1
    text, _ = dev_print(core, B, len(rows))  # (of the parse that the failed decode left pending)
    assert text == py_print(rows)


# ---- case 7: golden models ---------------------------------------------------------------------------------------------------------------------
def check_golden(B, name, aligns=(0, 5)):
    """encode -> print == encode_cli's id output; decode_text of that == decode_cli of it; parse(print) and print(parse) are identities"""
    a = model_args(name)
    core = D.core_of(name)
    data, _ = K.golden(name)
    n = len(K.py_split(data))
    special = [a[k] for k in ("pad", "unk", "bos", "eos") if a[k] != -1]
    for k, (b, e, r) in enumerate(S.FLAGS):
        if (b and a["bos"] == -1) or (e and a["eos"] == -1):
            continue
        want = cli_encode_ids(core, data, b, e, r)
        P = K.Placed(B, data, aligns[k % len(aligns)])
        nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), bool(b), bool(e), bool(r))
        ids, off = core.fetch_encode(nl, ni)
        text, toff = dev_print(core, B, n)
        assert text == want, (name, b, e, r)
        assert text == py_print(K.rows(ids, off)) and int(toff[-1]) == len(text)
        ids2, off2 = core.fetch_encode(nl, ni)  # the ids stay pending behind the print
        assert ids2.tolist() == ids.tolist() and off2.tolist() == off.tolist()
        # parse(print) == the ids; print(parse(print)) == print
        p_ids, p_off = dev_parse(core, B, text, aligns[(k + 1) % len(aligns)])
        assert p_ids.tolist() == ids.tolist() and p_off.tolist() == off.tolist()
        assert dev_print(core, B, n)[0] == text
        for ign in ((), special):
            got = dev_decode_text(core, B, text, ign, aligns[k % len(aligns)])
            assert got[:3] == cli_decode(core, text, ign), (name, b, e, r, ign)
            o = got[3].tolist()
            assert [got[2][o[i]:o[i + 1] - 1].decode() for i in range(n)] == core.decode(K.rows(ids, off), list(ign))


def check_digit_counts(B, aligns=ALL, name="readme_small"):
    """every digit count on both sides of every power of ten, negatives, both int32 limits: a hand-made result, placed through the parser"""
    core = D.core_of(name)
    vals = [0] + [v for k in range(10) for v in (10 ** k - 1, 10 ** k, 10 ** k + 1)] + [I32_MAX, I32_MAX - 1]
    vals = sorted(set(v for v in vals if v <= I32_MAX))
    rows = [vals, [-v for v in vals] + [I32_MIN], [], [I32_MIN], [0], list(range(0, 130)), [], [-1] * 200 + [I32_MIN] * 200 + [I32_MAX] * 200]
    text = py_print(rows)
    assert py_parse(text)[0] == rows
    for a in aligns:
        ids, off = dev_parse(core, B, text, a)
        assert K.rows(ids, off) == rows, a
        got, toff = dev_print(core, B, len(rows))
        assert got == text and toff.tolist() == np.cumsum([0] + [len(py_print([r])) for r in rows]).tolist(), a
    # and without spaces where the format allows it: the same ids
    glued = b"1-2-3+4 +5\n"
    ids, off = dev_parse(core, B, glued)
    assert dev_print(core, B, 1)[0] == b"1 -2 -3 4 5 \n"


# ---- case 8: pending results ---------------------------------------------------------------------------------------------------------------------
def check_pending(B, name="readme_small"):
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    core = D.core_of(name)
    # a fresh encoder: nothing of one sentence or more is pending
    nt, ms = C.c_uint64(9), C.c_double()
    assert L.yttm_idtext_device(core._h, 3, C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 1 and nt.value == 0
    assert err.value.decode() == "idtext_device: no matching encode result"
    # a decode result survives a parse; a parse result survives a decode and a print
    dec = D.dev_decode(core, B, np.array([5, 6, 7, 8], np.int32), np.array([0, 3, 4], np.uint64))
    assert dec[0] == 0
    ids, off = dev_parse(core, B, b"9 10\n\n11 12 13\n", 7)
    assert D._take_result(core, B, 2, len(dec[2]))[0] == dec[2]
    dec2 = D.dev_decode(core, B, np.array([5, 6], np.int32), np.array([0, 2], np.uint64))
    assert dec2[0] == 0
    i2, o2 = K.take_encoded(core, B, 3, 5)
    assert (i2.tolist(), o2.tolist()) == ([9, 10, 11, 12, 13], [0, 2, 2, 5]) == (ids.tolist(), off.tolist())
    # fetch, copy_padded, encode_longest on a parsed result
    assert core.encode_longest(3) == 3
    d_m, d_l = B.empty(3 * 4, np.int32), B.empty(3, np.int32)
    assert core.copy_encode_padded(B.ptr(d_m), B.ptr(d_l), 3, 4, -100) == 3
    assert B.get(d_m, 12).tolist() == [9, 10, -100, -100] + [-100] * 4 + [11, 12, 13, -100] and B.get(d_l, 3).tolist() == [2, 0, 3]
    # the print replaces the text, not the ids; the wrong n_sent replaces nothing
    text, _ = dev_print(core, B, 3)
    assert text == b"9 10 \n\n11 12 13 \n"
    assert L.yttm_idtext_device(core._h, 2, C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 1
    assert D._take_result(core, B, 3, len(text))[0] == text
    assert L.yttm_decode_fetch(core._h, None, None, 1, err, _lib.ERRLEN) != 0
    # argument errors replace nothing
    nl, ni = C.c_uint64(), C.c_uint64()
    assert L.yttm_ids_parse_device(core._h, None, 5, C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN) == 2
    assert L.yttm_decode_text_device(core._h, None, 5, None, 0, C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 2
    assert K.take_encoded(core, B, 3, 5)[0].tolist() == ids.tolist() and D._take_result(core, B, 3, len(text))[0] == text
    # an invalid id: the parse is pending (it succeeded), no text is
    bad = dev_decode_text(core, B, b"5 6\n7 99999 8\n", (), 3)
    assert bad[0] == 1 and "99999" in bad[1] and (bad[4], bad[5]) == (2, 5)
    assert K.take_encoded(core, B, 2, 5)[0].tolist() == [5, 6, 7, 99999, 8]
    assert L.yttm_decode_fetch(core._h, None, None, 2, err, _lib.ERRLEN) != 0
    # an empty text through null pointers
    assert L.yttm_ids_parse_device(core._h, None, 0, C.byref(nl), C.byref(ni), C.byref(ms), err, _lib.ERRLEN) == 0 and (nl.value, ni.value) == (0, 0)
    assert L.yttm_idtext_device(core._h, 0, C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 0 and nt.value == 0
    assert L.yttm_decode_text_device(core._h, None, 0, None, 0, C.byref(nl), C.byref(ni), C.byref(nt), C.byref(ms), err, _lib.ERRLEN) == 0
    assert (nl.value, ni.value, nt.value) == (0, 0, 0)
    # the lanes work afterwards: an encode, its print, and the SUBWORD route
    data, _ = K.golden(name)
    i3, o3 = K.dev_encode_text(core, B, data, 1, 1, 0, align=2)
    assert dev_print(core, B, len(o3) - 1)[0] == py_print(K.rows(i3, o3))
    S.same(core, B, ["ab Z cd", ""], 0, 0, 0, "after the id text calls")


# ---- case 9: files -----------------------------------------------------------------------------------------------------------------------------
def file_texts(core, name):
    data, _ = K.golden(name)
    ids = cli_encode_ids(core, data, 1, 1, 0)
    rng = random.Random(8)
    vocab = core.vocab_size()
    odd = b"".join(rng.choice([b"5 6 7", b"", b" ", b"12abc 7", b"1-2 x 99999", b"\t8\r", b"+4 -", b"0007"]) + b"\n" for _ in range(300))
    return [ids, ids[:-1], b"", b"\n", b"\n\n\n", b"7", b"5 6\r\n7\r\n\r\n", odd, odd + b" ".join(b"%d" % rng.randrange(vocab) for _ in range(3000)) + b"\n8 9"]


def ref_decode_file(model, path, tmp_path):
    if not refbin.available("prod"):
        return None
    out = str(tmp_path / "ref_dec.txt")
    p = subprocess.run([refbin.path("prod"), "decode", model, path, out], capture_output=True)
    return open(out, "rb").read() if p.returncode == 0 else None


def check_decode_file(tmp_path, name="readme_small", use_ref=False):
    """yttm_decode_file: the same file whatever the piece size and the transfer chunk, equal to decode_cli's output (and, with nothing ignored and
    nothing outside the vocabulary, to the compiled reference's where it is present)"""
    core = D.core_of(name)
    model = S.model_path(name)
    for k, data in enumerate(file_texts(core, name)):
        path = str(tmp_path / f"ids{k}.txt")
        open(path, "wb").write(data)
        rows, flat, _ = py_parse(data)
        ign = outside(rows, core.vocab_size())
        want = cli_decode(core, data, ign)
        assert want[0] == 0
        longest = max([len(ln) for ln in K.py_split(data)] + [0]) + 1
        files = []
        for j, (chunk, io_kb) in enumerate(((None, None), (max(len(data) // 8, 1), 1), (longest - 2 if longest > 2 else 1, 1), (1, None), (len(data) + 9, 1))):
            out = str(tmp_path / f"dec{k}_{j}.txt")
            with DC.env(**({"YTTM_IO_CHUNK_KB": io_kb} if io_kb else {})):
                c2 = D.core_of(name)
                rep = c2.decode_file(path, out, ign, chunk, report=True)
            got = open(out, "rb").read()
            files.append(got)
            assert got == want[2], (k, chunk)
            assert (rep["lines"], rep["ids"], rep["text_bytes"], rep["bytes"]) == (len(rows), len(flat), len(got), len(data))
            assert {"pieces", "piece_bytes", "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_parse", "seconds_decode",
                    "seconds_download_write"} <= set(rep)
            if j == 1 and k == 0:
                assert rep["pieces"] >= 5, rep
            if j in (0, 4) and data:
                assert rep["pieces"] == 1, rep
            if j == 0:
                assert c2.decode_file(path, out, ign, chunk) == (len(rows), len(flat), len(got))
        assert len(set(files)) == 1
        if use_ref and not ign:
            ref = ref_decode_file(model, path, tmp_path)
            assert ref is None or ref == want[2], k


def check_idtext_file(tmp_path, name="readme_small", use_ref=False, picks=None):
    """yttm_encode_file_idtext: the file `yttm encode --output_type id` prints, whatever the piece size"""
    model = S.model_path(name)
    for k, data in enumerate(S.texts(name)):
        if picks is not None and k not in picks:
            continue
        path = str(tmp_path / f"in{k}.txt")
        open(path, "wb").write(data)
        lines = K.py_split(data)
        longest = max([len(ln) for ln in lines] + [0]) + 1
        for b, e, r in S.FLAGS if k == 0 else ((0, 0, 0), (1, 1, 1)):
            core = D.core_of(name)
            want = cli_encode_ids(core, data, b, e, r)
            h_ids, h_off = K.host_encode(core, data, b, e, r)
            assert want == py_print(K.rows(h_ids, h_off))
            files = []
            for j, (chunk, io_kb) in enumerate(((None, None), (max(len(data) // 8, 1), 1), (longest - 2 if longest > 2 else 1, 1), (1, None), (len(data) + 9, 1))):
                out = str(tmp_path / f"out{k}_{j}.txt")
                with DC.env(**({"YTTM_IO_CHUNK_KB": io_kb} if io_kb else {})):
                    c2 = D.core_of(name)
                    rep = c2.encode_file_idtext(path, out, b, e, r, 0.0, chunk, report=True)
                got = open(out, "rb").read()
                files.append(got)
                assert got == want, (k, b, e, r, chunk)
                assert (rep["lines"], rep["ids"], rep["text_bytes"], rep["bytes"]) == (len(lines), len(h_ids), len(got), len(data))
                assert {"pieces", "piece_bytes", "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_format",
                        "seconds_download_write"} <= set(rep)
                if j in (0, 4) and data:
                    assert rep["pieces"] == 1, rep
                if j == 0:
                    assert c2.encode_file_idtext(path, out, b, e, r, 0.0, chunk) == (len(lines), len(h_ids), len(got))
            assert len(set(files)) == 1
            if use_ref and refbin.available("prod") and b"\r" not in data and all(ln.decode(errors="ignore").encode() == ln for ln in lines):
                p = subprocess.run([refbin.path("prod"), "encode", model, path, "-", "1", str(b), str(e), str(r), "0.0", "id"], capture_output=True)
                assert p.returncode != 0 or p.stdout == want, (k, b, e, r)


def check_file_errors(tmp_path, name="readme_small"):
    import pytest
    import youtokentome_amd as yttm
    bpe = S.bpe_of(name)
    core = bpe.bpe_cython
    L, err, z = _lib.load(), C.create_string_buffer(_lib.ERRLEN), C.c_uint64()
    ids_path, txt_path = str(tmp_path / "ids.txt"), str(tmp_path / "in.txt")
    open(ids_path, "wb").write(b"5 6 7\n8\n")
    open(txt_path, "wb").write(b"ab Z\ncd\n")
    want_dec, want_ids = cli_decode(core, b"5 6 7\n8\n")[2], cli_encode_ids(core, b"ab Z\ncd\n")
    routes = ((lambda src, dst: bpe.decode_file(src, dst), ids_path, b"5 6 7\n8\n", want_dec),
              (lambda src, dst: bpe.encode_file(src, dst, id_text=True), txt_path, b"ab Z\ncd\n", want_ids))
    for run, path, content, want in routes:
        with pytest.raises(ValueError, match="Failed to open file: .*no_such_file"):
            run(str(tmp_path / "no_such_file.txt"), str(tmp_path / "o.txt"))
        with pytest.raises(ValueError, match="Failed to open file for writing: .*no_such_dir"):
            run(path, str(tmp_path / "no_such_dir" / "o.txt"))
        with pytest.raises(ValueError, match="Failed to read file: .* is not a regular file"):
            run(str(tmp_path), str(tmp_path / "o.txt"))
        # the input itself as the output, under its own name, a hard link and a symlink: refused before anything is truncated
        same, link = path + ".same", path + ".link"
        os.link(path, same)
        os.symlink(path, link)
        for dst in (path, same, link):
            with pytest.raises(ValueError, match="Failed to open file for writing: .* is the input file"):
                run(path, dst)
            assert open(path, "rb").read() == content
        # an existing, longer output file is replaced, not overwritten in place
        old = path + ".old"
        open(old, "wb").write(b"x" * 1000)
        run(path, old)
        assert open(old, "rb").read() == want
        full = path + ".full"
        os.symlink("/dev/full", full)
        with pytest.raises(ValueError, match="Failed to write file: .*full"):
            run(path, full)
        # the lanes are as good as before
        assert run(path, str(tmp_path / "o.txt"))[0] == 2 and open(str(tmp_path / "o.txt"), "rb").read() == want
    for fn, args in ((L.yttm_decode_file, (None, 0, 0)), (L.yttm_encode_file_idtext, (0, 0, 0, 0.0, 0))):
        src = ids_path if fn is L.yttm_decode_file else txt_path
        for dst in (None, b""):
            assert fn(core._h, os.fsencode(src), dst, *args, C.byref(z), C.byref(z), C.byref(z), None, 0, err, _lib.ERRLEN) == 1
            assert err.value.decode() == "Failed to open file for writing: no output path"
    with pytest.raises(ValueError, match="needs out"):
        bpe.encode_file(txt_path, id_text=True)
    with pytest.raises(ValueError, match="id_text goes with output_type ID"):
        bpe.encode_file(txt_path, str(tmp_path / "o.txt"), output_type=yttm.OutputType.SUBWORD, id_text=True)
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_file(txt_path, str(tmp_path / "o.txt"), dropout_prob=2, id_text=True)
    with pytest.raises(ValueError, match=S.BOS_MSG):
        S.bpe_of("nopad").encode_file(txt_path, str(tmp_path / "o.txt"), bos=True, id_text=True)
    # an invalid id in the third piece: the message of the host path for the first such id in file order, the pieces before it written
    lines = [b"5 6 7"] * 40 + [b"8 x 77777"] + [b"9 10"] * 40 + [b"11 88888 12 99999"] + [b"13"] * 40 + [b"66666"]
    data = b"\n".join(lines) + b"\n"
    bad_path, out = str(tmp_path / "bad.txt"), str(tmp_path / "bad_out.txt")
    open(bad_path, "wb").write(data)
    want = cli_decode(core, data)
    assert want[0] == 1 and "88888" in want[1]
    cut = data.index(b"11 88888")
    for chunk in (cut // 2 + 3, None, 1):
        with pytest.raises(ValueError) as ei:
            core.decode_file(bad_path, out, None, chunk)
        assert str(ei.value) == want[1], chunk
        assert want[2].startswith(open(out, "rb").read())
    assert core.decode_file(bad_path, out, [88888, 99999, 66666], cut // 2 + 3, report=True)["pieces"] == 3
    assert open(out, "rb").read() == cli_decode(core, data, [88888, 99999, 66666])[2]
    # every existing call of encode_file keeps its meaning
    ids, off = bpe.encode_file(txt_path)
    w_ids, w_off = K.host_encode(core, b"ab Z\ncd\n")
    assert ids.tolist() == w_ids.tolist() and off.tolist() == w_off.tolist()
    assert bpe.encode_file(txt_path, str(tmp_path / "pre")) == (2, len(w_ids))
    assert bpe.encode_file(txt_path, str(tmp_path / "sub.txt"), output_type=yttm.OutputType.SUBWORD)[0] == 2
    assert open(str(tmp_path / "sub.txt"), "rb").read() == S.host_text(core, [b"ab Z", b"cd"])[2]


# ---- case 10: the command line ---------------------------------------------------------------------------------------------------------------------
def check_cli(tmp_path, name="readme_small"):
    core = D.core_of(name)
    a = model_args(name)
    data = S.texts(name)[9]
    path, model = str(tmp_path / "in.txt"), S.model_path(name)
    open(path, "wb").write(data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def run(args, stdin=None):
        p = subprocess.run(cli + args, stdin=stdin, capture_output=True, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    for extra in ([], ["--bos", "--eos", "--reverse"]):
        out = str(tmp_path / ("ids" + "".join(extra) + ".txt"))
        run(["encode_file", f"--model={model}", f"--input={path}", f"--output={out}", "--output_type=id_text"] + extra)
        printed = run(["encode", f"--model={model}", "--output_type=id"] + extra, stdin=open(path, "rb"))
        assert open(out, "rb").read() == printed and printed.count(b"\n") == len(K.py_split(data)) > 100
    for ign in ([], [f"--ignore_ids={a['bos']},{a['eos']},{a['unk']}"]):  # (of the file with <BOS> and <EOS> in it)
        dec = str(tmp_path / "dec.txt")
        run(["decode_file", f"--model={model}", f"--input={out}", f"--output={dec}"] + ign)
        assert open(dec, "rb").read() == run(["decode", f"--model={model}"] + ign, stdin=open(out, "rb"))
    # the id and subword choices write what they wrote
    prefix = str(tmp_path / "bin")
    run(["encode_file", f"--model={model}", f"--input={path}", f"--output={prefix}"])
    w_ids, w_off = K.host_encode(core, data)
    f_ids, f_off = K.read_out(prefix)
    assert f_ids.tolist() == w_ids.tolist() and f_off.tolist() == w_off.tolist()
    sub = str(tmp_path / "sub.txt")
    run(["encode_file", f"--model={model}", f"--input={path}", f"--output={sub}", "--output_type=subword"])
    assert open(sub, "rb").read() == S.host_text(core, K.py_split(data))[2]


# ---- case 11: one larger pass ------------------------------------------------------------------------------------------------------------------
def check_large(B, name="zipf", n=50_000, width=128):
    """n sentences of `width` chars of Zipf text: text -> id text -> decoded text, against the host routes"""
    import gen
    core = D.core_of(name)
    a = model_args(name)
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=29, vocab=20000).replace(b"\n", b" ")[:n * width]
    data = b"".join(raw[i * width:(i + 1) * width] + b"\n" for i in range(n))
    want_ids = cli_encode_ids(core, data, 1, 1, 0)
    P = K.Placed(B, data, 9)
    nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
    assert nl == n
    text, _ = dev_print(core, B, n)
    assert text == want_ids
    ign = (a["bos"], a["eos"])
    got = dev_decode_text(core, B, text, ign, 3)
    assert got[:3] == cli_decode(core, text, ign) and (got[4], got[5]) == (n, ni)
