"""Checks of the training blocks made on the device (yttm_blocks_device, yttm_blocks_ids_device, yttm_blocks_flush, yttm_blocks_open / _discard,
yttm_blocks_fetch / _copy_device, yttm_encode_file_blocks, the BPE.*blocks* methods, `yttm blocks_file`), shared by the emulator tests
(test_blocks_device.py, test_blocks_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests (test_gpu_blocks.py).

Two yardsticks that share no code:
  py_blocks   the rule of include/yttm_mi355x.h as plain Python loops over the input lists; every array is compared exactly;
  props       properties computed with numpy array operations: the rows without padding, concatenated, are the ids; seg / pos rebuilt from frags and
              row_frags equal the returned ones; padding only where the rule allows it; in whole mode fragment k is the k-th non-empty sentence
              and the first sentence of row r + 1 added to row r's ids exceeds L.
Every input array sits at a chosen element offset between guard ids, every output array of the device exit has guard words behind it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import spans_checks as SP
from decode_checks import NumpyBuf, TorchBuf  # noqa: F401  (the buffers are re-exported)
from idcount_checks import PlacedIds
from spans_checks import BOS_MSG, EOS_MSG, all_models, model, sentences_of, to_bytes  # noqa: F401
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
STREAM, WHOLE = 0, 1
PAD, KEEP, DROP = 0, 1, 2
PADV = -9  # a pad value no generated id has
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 5000)
NO_BLOCKS = ("fetch_blocks: no matching blocks", "copy_blocks: no matching blocks")
NO_RESULT = "blocks_device: no matching encode result"


class TooLong(Exception):
    pass


# ---- yardstick 1: the rule as loops -------------------------------------------------------------------------------------------------------------
def py_blocks(sents, L, mode, pad, tail, open_row=()):
    """-> (rows, seg, pos, frags, row_frags, new open row as a list of fragments); raises TooLong(index, length) as the rule refuses"""
    rows_f, cur, cur_n = [], [], 0
    n_open = len(open_row)
    for k, s in enumerate(list(open_row) + list(sents)):
        s = [int(v) for v in s]
        if not s:
            continue
        if mode == STREAM:
            i = 0
            while i < len(s):
                take = min(L - cur_n, len(s) - i)
                cur.append(s[i:i + take])
                cur_n += take
                i += take
                if cur_n == L:
                    rows_f.append(cur)
                    cur, cur_n = [], 0
        else:
            if len(s) > L:
                raise TooLong(k - n_open, len(s))
            if cur_n + len(s) > L:
                rows_f.append(cur)
                cur, cur_n = [], 0
            cur.append(s)
            cur_n += len(s)
            if cur_n == L:
                rows_f.append(cur)
                cur, cur_n = [], 0
    new_open = []
    if cur:
        if tail == PAD:
            rows_f.append(cur)
        elif tail == KEEP:
            new_open = cur
    rows, seg, pos, frags, row_frags = [], [], [], [], [0]
    for r, fr in enumerate(rows_f):
        a, b, c = [], [], []
        for o, piece in enumerate(fr):
            frags.append((r * L + len(a), len(piece)))
            for j, v in enumerate(piece):
                a.append(v)
                b.append(o + 1)
                c.append(j)
        while len(a) < L:
            a.append(pad)
            b.append(0)
            c.append(0)
        rows.append(a)
        seg.append(b)
        pos.append(c)
        row_frags.append(len(frags))
    return (np.array(rows, np.int32).reshape(-1, L), np.array(seg, np.int32).reshape(-1, L), np.array(pos, np.int32).reshape(-1, L),
            np.array(frags, np.int32).reshape(-1, 2), np.array(row_frags, np.uint64), new_open)


# ---- yardstick 2: properties, array operations only ---------------------------------------------------------------------------------------------
def props(got, flat, off, L, mode, tail, what=""):
    """got = (rows, seg, pos, frags, row_frags) of ONE call from an empty open row on flat / off"""
    rows, seg, pos, frags, row_frags = got
    flat, off = np.asarray(flat, np.int64), np.asarray(off, np.int64)
    n_rows = rows.shape[0]
    assert rows.shape == seg.shape == pos.shape == (n_rows, L) and len(row_frags) == n_rows + 1, what
    valid = seg > 0
    used = int(valid.sum())
    # the rows without padding, concatenated, are the ids (all of them unless the tail was dropped or kept)
    assert rows[valid].astype(np.int64).tolist() == flat[:used].tolist(), what
    if tail == PAD:
        assert used == len(flat), what
    else:
        assert len(flat) - used < L, what
    # padding: behind the ids of a row only; in stream mode in the last row only
    assert not (valid[:, 1:] & ~valid[:, :-1]).any(), what
    if n_rows:
        assert valid[:, 0].all(), what
    if mode == STREAM and n_rows > 1:
        assert valid[:-1].all(), what
    if tail != PAD and mode == STREAM:
        assert valid.all(), what
    assert (pos[~valid] == 0).all(), what
    # seg / pos rebuilt from frags and row_frags
    rf = row_frags.astype(np.int64)
    assert rf[0] == 0 and rf[-1] == len(frags) and (np.diff(rf) >= (1 if n_rows else 0)).all(), what
    st, ln = frags[:, 0].astype(np.int64), frags[:, 1].astype(np.int64)
    assert (ln > 0).all() and int(ln.sum()) == used, what
    row_of = np.repeat(np.arange(n_rows), np.diff(rf))
    ordinal = np.arange(len(frags)) - rf[row_of] + 1
    seg2, pos2 = np.zeros(n_rows * L, np.int64), np.zeros(n_rows * L, np.int64)
    where = np.repeat(st, ln) + (np.arange(used) - np.repeat(np.cumsum(ln) - ln, ln))
    assert len(np.unique(where)) == used and (st // L == row_of).all() and ((st + ln - 1) // L == row_of).all(), what
    seg2[where] = np.repeat(ordinal, ln)
    pos2[where] = np.arange(used) - np.repeat(np.cumsum(ln) - ln, ln)
    assert (seg2.reshape(n_rows, L) == seg).all() and (pos2.reshape(n_rows, L) == pos).all(), what
    assert (np.diff(st) > 0).all(), what
    lens = np.diff(off)
    if mode == WHOLE:
        ne = lens[lens > 0]
        assert ln.tolist() == ne[:len(ln)].tolist(), what  # fragment k is the k-th non-empty sentence
        fill = valid.sum(axis=1)
        first_next = ln[rf[1:-1]] if n_rows > 1 else np.zeros(0, np.int64)
        assert (fill[:-1] + first_next > L).all(), what
        if tail != PAD and len(ne) > len(ln):  # the row that was kept or dropped did not fit behind the last emitted one either
            assert n_rows == 0 or fill[-1] + ne[len(ln)] > L, what
    else:
        # a fragment ends where its sentence or its row ends
        ends = np.cumsum(lens)
        stream_end = np.cumsum(ln)
        assert (np.isin(stream_end, ends) | ((st + ln) % L == 0)).all(), what


# ---- the device path ----------------------------------------------------------------------------------------------------------------------------
def flatten(sents):
    off = np.zeros(len(sents) + 1, np.uint64)
    if len(sents):
        np.cumsum([len(s) for s in sents], out=off[1:])
    flat = np.concatenate([np.asarray(s, np.int64) for s in sents] + [np.zeros(0, np.int64)]).astype(np.int32)
    return flat, off


def take(core, B, n_rows, n_frags, L):
    """the slot by both exits, which must agree; the device copy writes the arrays and no more"""
    got = core.fetch_blocks(n_rows, n_frags, L)
    n = n_rows * L
    d = [B.empty(n + 3, np.int32) for _ in range(3)] + [B.empty(2 * n_frags + 3, np.int32), B.empty(n_rows + 1 + 3, np.uint64)]
    core.copy_blocks_device(*[B.ptr(x) for x in d], n_rows, n_frags)
    sizes = (n, n, n, 2 * n_frags, n_rows + 1)
    for k, (x, size) in enumerate(zip(d, sizes)):
        dev = B.get(x)
        assert dev[:size].tobytes() == got[k].tobytes(), "the two exits differ in array %d" % k
        assert dev[size:size + 3].view(np.int64 if k == 4 else np.int32).tolist() == [-7] * 3, "the copy wrote past array %d" % k
    return got


def raw_ids(core, ptr, optr, n, n_ids, L, mode, pad, tail):
    nr, nf, err = C.c_uint64(77), C.c_uint64(77), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_blocks_ids_device(core._h, C.c_void_p(ptr), C.c_void_p(optr), n, n_ids, L, mode, pad, tail, C.byref(nr), C.byref(nf), None, err,
                                            _lib.ERRLEN)
    return rc, err.value.decode(), nr.value, nf.value


def dev_blocks(core, B, sents, L, mode, pad=PADV, tail=PAD, shift=0):
    """yttm_blocks_ids_device on the sentences' ids placed at `shift` -> the five arrays; the ids and their guards stay as they were"""
    flat, off = flatten(sents)
    P = PlacedIds(B, flat, shift)
    d_off = B.put(off)
    n_rows, n_frags, _ = core.blocks_ids_device_raw(P.ptr, B.ptr(d_off), len(sents), len(flat), L, mode, pad, tail)
    assert P.intact(), "the ids or their guard values were written"
    assert B.get(d_off).view(np.uint64).tolist() == off.tolist()
    return take(core, B, n_rows, n_frags, L)


def equal(got, want, what):
    for k, name in enumerate(("rows", "seg", "pos", "frags", "row_frags")):
        assert got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.nonzero(got[k].ravel() != want[k].ravel())[0]
            raise AssertionError("%s: %s differs at %d of %d places, first flat %d: got %d want %d" % (
                what, name, len(bad), got[k].size, bad[0], got[k].ravel()[bad[0]], want[k].ravel()[bad[0]]))


def same(core, B, sents, L, mode, pad=PADV, tail=PAD, shift=0, what=""):
    """one call from an empty open row: device == loops, and the properties hold; the open row afterwards is the loops'"""
    what = "%s L %d mode %d tail %d shift %d" % (what, L, mode, tail, shift)
    core.blocks_discard()
    got = dev_blocks(core, B, sents, L, mode, pad, tail, shift)
    want = py_blocks(sents, L, mode, pad, tail)
    equal(got, want[:5], what)
    flat, off = flatten(sents)
    props(got, flat, off, L, mode, tail, what)
    kept = sum(len(f) for f in want[5])
    assert core.blocks_open() == ((kept, L, mode) if kept else (0, 0, 0)), what
    return got


def rand_sents(rng, n, lo, hi, empty=0.1, vocab=30000):
    out = []
    for _ in range(n):
        k = 0 if rng.rand() < empty else int(rng.randint(lo, hi + 1))
        out.append(rng.randint(0, vocab, size=k).astype(np.int32))
    return out


# ---- case 1: every seq_len, both modes, every tail ----------------------------------------------------------------------------------------------
def check_lengths(B, lengths=LENGTHS, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(31)
    for L in lengths:
        ar = np.arange(1, 3 * L + 2, dtype=np.int32)
        sets = [("no sentence", []), ("only empty sentences", [[], [], []])]
        sets += [("one sentence of %d" % k, [ar[:k]]) for k in sorted({1, max(L - 1, 1), L})]
        sets += [("a boundary on every row edge", [ar[:L], [], ar[:L], ar[:L]]), ("sums that hit L", [ar[:L - L // 2], ar[:L // 2], ar[:1], ar[:L - 1], [], ar[:L]])]
        hi = min(L, 40) if L > 2 else L
        sets.append(("random", rand_sents(rng, max(6, min(4 * L, 300) // max(hi // 2, 1)), 1, hi)))
        for mode in (STREAM, WHOLE):
            for what, sents in sets:
                for tail in (PAD, KEEP, DROP):
                    same(core, B, sents, L, mode, tail=tail, shift=(L + tail) % 4, what=what)
        same(core, B, [ar[:L + 1]], L, STREAM, what="one sentence of L + 1")
        same(core, B, [ar[:3 * L + 1]], L, STREAM, what="one sentence of 3 L + 1")
        same(core, B, [ar[:3 * L + 1], ar[:2]], L, STREAM, tail=KEEP, what="one sentence of 3 L + 1, kept")
        same(core, B, [ar[:2], [], ar[:2 * L + 1], ar[:L]], L, STREAM, tail=DROP, what="a sentence across rows")


# ---- case 2: boundaries at chosen lanes, runs of empty sentences, edge values -------------------------------------------------------------------
def check_boundaries(B, name="readme_small"):
    core = D.core_of(name)
    ar = np.arange(100, 5000, dtype=np.int32)
    for L in (1000, 129):
        for cuts in ((1, 4, 252, 253, 255, 256, 257, 260, 511, 512, 516, 2047, 2048, 2049, 2300), (63, 64, 65, 127, 128, 192, 255, 1024, 2050), tuple(range(0, 2200, 4)),
                     tuple(range(3, 2200, 4))):
            edges = [0] + [c for c in cuts if c > 0] + [2304]
            sents = [ar[a:b] for a, b in zip(edges[:-1], edges[1:])]
            for mode in (STREAM, WHOLE):
                if mode == WHOLE and max(len(s) for s in sents) > L:
                    continue
                same(core, B, sents, L, mode, what="cuts %s" % (cuts[:4],))
    # 200 empty sentences in a row inside a step, in front of it and behind the last id
    for L in (64, 1000):
        for mode in (STREAM, WHOLE):
            sents = [ar[:7]] + [[]] * 200 + [ar[:30], ar[:1]] + [[]] * 70 + [ar[:50]] + [[]] * 200
            same(core, B, sents, L, mode, what="200 empty sentences")
            same(core, B, [[]] * 130 + sents, L, mode, tail=KEEP, what="empty sentences first")
    # edge values, and a pad value that is a real id
    odd = np.array([-1, I32_MIN, I32_MAX, 0, 5, -1, I32_MAX, I32_MIN, 7], np.int32)
    for mode in (STREAM, WHOLE):
        for pad in (5, -1, I32_MIN, I32_MAX, 0):
            same(core, B, [odd[:4], odd[4:], odd, odd[:1]], 6 if mode == STREAM else 9, mode, pad=pad, what="edge values, pad %d" % pad)


# ---- case 3: a block of the orbit pass that `next` jumps over -----------------------------------------------------------------------------------
def check_orbit_skip(B, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(32)
    a, b = rand_sents(rng, 1700, 1, 9, empty=0.05), rand_sents(rng, 1800, 1, 9, empty=0.05)
    sents = a + [[]] * 1500 + b
    assert len(sents) == 5000
    for L in (9, 64):
        for mode in (WHOLE, STREAM):
            same(core, B, sents, L, mode, what="1500 empty sentences among 5000")
    same(core, B, [[]] * 2100 + a[:40], 16, WHOLE, tail=KEEP, what="2100 empty sentences first")
    same(core, B, a[:40] + [[]] * 2100, 16, WHOLE, what="2100 empty sentences last")


# ---- case 4: whole mode's fits --------------------------------------------------------------------------------------------------------------------
def check_whole_fits(B, name="readme_small"):
    core = D.core_of(name)
    ar = np.arange(1, 400, dtype=np.int32)
    for L in (5, 64, 130):
        same(core, B, [ar[:L]] * 5, L, WHOLE, what="sentences of exactly L")
        same(core, B, [ar[:L - 2], ar[:2], ar[:1], ar[:L - 1], ar[:L - 1], ar[:1], ar[:L]], L, WHOLE, what="sums that hit L")
        same(core, B, [ar[:L - 2], ar[:3], ar[:L - 3], ar[:3]], L, WHOLE, what="sums of L + 1 and L")
        same(core, B, [ar[:1]] * (3 * L + 1), L, WHOLE, tail=KEEP, what="sentences of one id")


def state_of(core, B, n_rows, n_frags, L):
    return [a.tobytes() for a in take(core, B, n_rows, n_frags, L)], core.blocks_open()


def check_too_long(B, name="readme_small"):
    """a sentence of L + 1 in whole mode: code 1, with the slot, the open row and the pending result unchanged"""
    core = D.core_of(name)
    sents = to_bytes(sentences_of(name))[:20]
    n_ids = D.encode_device(core, B, sents, 0, 0, 0)
    ids, off = D.encode_fetch(core, len(sents), n_ids)
    ar = np.arange(1, 100, dtype=np.int32)
    L = 8
    flat, o = flatten([ar[:5], ar[:6]])
    d_i, d_o = B.put(flat), B.put(o)
    n_rows, n_frags, _ = core.blocks_ids_device_raw(B.ptr(d_i), B.ptr(d_o), 2, len(flat), L, WHOLE, PADV, KEEP)
    assert (n_rows, n_frags) == (1, 1) and core.blocks_open() == (6, L, WHOLE)
    before = state_of(core, B, n_rows, n_frags, L)
    for k, bad in enumerate(([ar[:2], [], ar[:L + 1], ar[:1]], [ar[:L + 1]], [ar[:3]] * 1100 + [ar[:L + 7]])):
        flat2, o2 = flatten(bad)
        d_i2, d_o2 = B.put(flat2), B.put(o2)
        rc, msg, nr, nf = raw_ids(core, B.ptr(d_i2), B.ptr(d_o2), len(bad), len(flat2), L, WHOLE, PADV, (PAD, KEEP, DROP)[k])
        at = [len(s) > L for s in bad].index(True)
        assert rc == 1 and "sentence %d:" % at in msg and "seq_len = %d; length = %d;" % (L, len(bad[at])) in msg and (nr, nf) == (0, 0), msg
        assert state_of(core, B, n_rows, n_frags, L) == before
        try:
            py_blocks(bad, L, WHOLE, PADV, PAD, [ar[:6]])
            raise AssertionError("the loops accept it")
        except TooLong as e:
            assert e.args == (at, len(bad[at]))
    ids2, off2 = K.take_encoded(core, B, len(sents), n_ids)
    assert ids2.tobytes() == ids.tobytes() and off2.tobytes() == off.tobytes()
    # stream mode takes the same sentences
    core.blocks_discard()
    equal(dev_blocks(core, B, [ar[:2], [], ar[:L + 1], ar[:1]], L, STREAM), py_blocks([ar[:2], [], ar[:L + 1], ar[:1]], L, STREAM, PADV, PAD)[:5], "stream")
    # seq_len outside 1 .. 2^24, a bad mode, a bad tail, the size limit, misaligned ids
    for L_bad, mode, tail in ((0, STREAM, PAD), ((1 << 24) + 1, WHOLE, PAD), (8, 2, PAD), (8, STREAM, 3), (8, WHOLE, -1)):
        rc, msg, _, _ = raw_ids(core, B.ptr(d_i), B.ptr(d_o), 2, len(flat), L_bad, mode, PADV, tail)
        assert rc == 1 and msg.startswith("blocks: "), msg
    rc, msg, _, _ = raw_ids(core, B.ptr(d_i) + 2, B.ptr(d_o), 2, len(flat), 8, STREAM, PADV, PAD)
    assert rc != 0 and "4-byte aligned" in msg
    # n_rows L beyond 2^31 - 1: refused from the offsets alone, before any id is read (the one sentence claims 2^31 ids that do not exist)
    d_big = B.put(np.array([0, 1 << 31], np.uint64))
    core.blocks_discard()
    n_rows, n_frags, _ = core.blocks_ids_device_raw(B.ptr(d_i), B.ptr(d_o), 2, len(flat), L, STREAM, PADV, KEEP)
    before = state_of(core, B, n_rows, n_frags, L)
    for L_big, tail in ((1 << 24, PAD), (1 << 24, DROP), (8, KEEP)):
        rc, msg, nr, nf = raw_ids(core, B.ptr(d_i), B.ptr(d_big), 1, 1 << 31, L_big, STREAM, PADV, tail)
        if L_big == 8:
            assert rc == 1 and "exceed 2^31 - 1 elements" in msg and (nr, nf) == (0, 0), msg
        else:
            assert rc == 1 and "the open row holds" in msg, msg
        assert state_of(core, B, n_rows, n_frags, L) == before
    core.blocks_discard()
    for L_big, tail in ((1 << 24, PAD), (1 << 24, DROP), (1, KEEP)):
        rc, msg, nr, nf = raw_ids(core, B.ptr(d_i), B.ptr(d_big), 1, 1 << 31, L_big, STREAM, PADV, tail)
        assert rc == 1 and "exceed 2^31 - 1 elements" in msg and (nr, nf) == (0, 0), msg
    assert [a.tobytes() for a in take(core, B, n_rows, n_frags, L)] == before[0] and core.blocks_open() == (0, 0, 0)


# ---- case 5: alignment ----------------------------------------------------------------------------------------------------------------------------
def check_alignment(B, shifts=(0, 1, 2, 3), name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(33)
    sents = rand_sents(rng, 120, 1, 60)
    for s in shifts:
        for L, mode in ((64, STREAM), (65, STREAM), (127, WHOLE), (1000, STREAM), (3, STREAM)):
            same(core, B, sents if L > 3 else sents[:20], L, mode, shift=s, what="alignment")


# ---- case 6: a batch cut into calls ---------------------------------------------------------------------------------------------------------------
def check_split_calls(B, name="readme_small"):
    """1, 2, 7 and S calls with tail = keep plus a flush == one call, in both modes; the open row between the calls is the loops'"""
    core = D.core_of(name)
    rng = np.random.RandomState(34)
    sents = rand_sents(rng, 45, 1, 30, empty=0.15)
    for L in (7, 30, 64, 200):
        for mode in (STREAM, WHOLE):
            if mode == WHOLE and L < 30:
                continue
            whole = py_blocks(sents, L, mode, PADV, PAD)
            for parts in (1, 2, 7, len(sents)):
                core.blocks_discard()
                cuts = [len(sents) * k // parts for k in range(parts + 1)]
                got, open_row = [], []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    g = dev_blocks(core, B, sents[a:b], L, mode, PADV, KEEP, shift=a % 4)
                    want = py_blocks(sents[a:b], L, mode, PADV, KEEP, open_row)
                    equal(g, want[:5], "call %d..%d of %d parts, L %d mode %d" % (a, b, parts, L, mode))
                    open_row = want[5]
                    kept = sum(len(f) for f in open_row)
                    assert core.blocks_open() == ((kept, L, mode) if kept else (0, 0, 0))
                    got.append(g)
                n_rows, n_frags, _ = core.blocks_flush_raw(PADV)
                assert n_rows == (1 if open_row else 0) and core.blocks_open() == (0, 0, 0)
                got.append(take(core, B, n_rows, n_frags, L))
                assert np.concatenate([g[0] for g in got]).tobytes() == whole[0].tobytes(), (L, mode, parts)
                assert np.concatenate([g[1] for g in got]).tobytes() == whole[1].tobytes(), (L, mode, parts)
                assert np.concatenate([g[2] for g in got]).tobytes() == whole[2].tobytes(), (L, mode, parts)
                assert sum(len(g[3]) for g in got) == len(whole[3])
                assert core.blocks_flush_raw(PADV)[:2] == (0, 0)  # nothing left: a result of no rows
                assert take(core, B, 0, 0, L)[4].tolist() == [0]


# ---- case 7: the open row's binding, the exits ----------------------------------------------------------------------------------------------------
def check_binding_and_exits(B, name="readme_small"):
    core = D.core_of(name)
    L0 = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)

    def raw_take(n_rows, n_frags):
        out = []
        host = np.full(64, 9, np.int32)
        p = host.ctypes.data_as(_lib.i32p)
        out.append((L0.yttm_blocks_fetch(core._h, p, None, None, None, None, n_rows, n_frags, err, _lib.ERRLEN), err.value.decode()))
        assert set(host.tolist()) == {9}
        d = B.empty(64, np.int32)
        out.append((L0.yttm_blocks_copy_device(core._h, C.c_void_p(B.ptr(d)), None, None, None, None, n_rows, n_frags, err, _lib.ERRLEN), err.value.decode()))
        assert set(B.get(d).tolist()) == {-7}
        return out

    refused = [(1, NO_BLOCKS[0]), (1, NO_BLOCKS[1])]
    assert raw_take(0, 0) == refused, "before any blocks call"
    assert core.blocks_open() == (0, 0, 0)
    ar = np.arange(1, 50, dtype=np.int32)
    flat, off = flatten([ar[:5], ar[:4]])
    d_i, d_o = B.put(flat), B.put(off)
    args = (B.ptr(d_i), B.ptr(d_o), 2, len(flat))
    assert core.blocks_ids_device_raw(*args, 6, STREAM, PADV, KEEP)[:2] == (1, 2)
    assert core.blocks_open() == (3, 6, STREAM)
    before = state_of(core, B, 1, 2, 6)
    for L, mode in ((7, STREAM), (6, WHOLE), (5, WHOLE)):  # another L or mode on a non-empty open row
        rc, msg, nr, nf = raw_ids(core, *args, L, mode, PADV, PAD)
        assert rc == 1 and "the open row holds 3 ids for seq_len 6, mode 0" in msg and (nr, nf) == (0, 0), msg
        assert state_of(core, B, 1, 2, 6) == before
    for wrong in ((0, 2), (2, 2), (1, 1), (1, 3)):  # mismatched n_rows / n_frags at the exits
        assert raw_take(*wrong) == refused, wrong
    # null exits are skipped, each array alone equals the full fetch
    full = take(core, B, 1, 2, 6)
    for k in range(5):
        bufs = [B.empty(32, np.uint64 if j == 4 else np.int32) if j == k else None for j in range(5)]
        ptrs = [C.c_void_p(B.ptr(x)) if x is not None else None for x in bufs]
        assert L0.yttm_blocks_copy_device(core._h, *ptrs, 1, 2, err, _lib.ERRLEN) == 0
        size = full[k].size
        assert B.get(bufs[k])[:size].tobytes() == full[k].tobytes()
    # the same (L, mode) goes on; discard empties the open row and another L is fine again
    n_rows, n_frags, _ = core.blocks_ids_device_raw(*args, 6, STREAM, PADV, KEEP)
    equal(take(core, B, n_rows, n_frags, 6), py_blocks([ar[:5], ar[:4]], 6, STREAM, PADV, KEEP, [ar[1:4]])[:5], "the open row goes on")
    assert core.blocks_open() == (0, 0, 0)
    assert core.blocks_ids_device_raw(*args, 6, STREAM, PADV, KEEP)[:2] == (1, 2)
    core.blocks_discard()
    assert core.blocks_open() == (0, 0, 0)
    got = dev_blocks(core, B, [ar[:3], ar[:4]], 4, WHOLE, PADV, DROP)
    equal(got, py_blocks([ar[:3], ar[:4]], 4, WHOLE, PADV, DROP)[:5], "after discard")
    # tail = drop leaves nothing open
    assert core.blocks_open() == (0, 0, 0)


# ---- case 8: pending results ----------------------------------------------------------------------------------------------------------------------
def pending_same(core, B, n, n_ids, L, mode, tail, what):
    """the pending result of n sentences: blocks == the loops on the fetched ids; the result fetches the same bytes afterwards"""
    ids, off = D.encode_fetch(core, n, n_ids)
    o = off.tolist()
    sents = [ids[o[i]:o[i + 1]] for i in range(n)]
    core.blocks_discard()
    n_rows, n_frags, _ = core.blocks_device_raw(n, L, mode, PADV, tail)
    got = take(core, B, n_rows, n_frags, L)
    equal(got, py_blocks(sents, L, mode, PADV, tail)[:5], what)
    props(got, ids, off, L, mode, tail, what)
    ids2, off2 = K.take_encoded(core, B, n, n_ids)
    assert ids2.tobytes() == ids.tobytes() and off2.tobytes() == off.tobytes(), what
    return ids, off


def check_pending_model(B, name):
    """a golden model, the flag sets it allows: yttm_encode_device + yttm_blocks_device"""
    M = model(name)
    core = D.core_of(name)
    sents = to_bytes(sentences_of(name))
    for k, (b, e, r) in enumerate(M.flags()):
        n_ids = D.encode_device(core, B, sents, b, e, r)
        ids, off = D.encode_fetch(core, len(sents), n_ids)
        longest = int(np.diff(off.astype(np.int64)).max())
        pending_same(core, B, len(sents), n_ids, 64 + k, STREAM, (PAD, KEEP, DROP)[k % 3], (name, b, e, r, "stream"))
        pending_same(core, B, len(sents), n_ids, max(longest, 33) + k, WHOLE, (PAD, DROP, KEEP)[k % 3], (name, b, e, r, "whole"))


def raw_pending(core, n_sent, L=8, mode=STREAM, tail=PAD):
    nr, nf, err = C.c_uint64(7), C.c_uint64(7), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_blocks_device(core._h, n_sent, L, mode, PADV, tail, C.byref(nr), C.byref(nf), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), nr.value, nf.value


def check_pending_misc(B, name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    assert raw_pending(core, 0) == (1, NO_RESULT, 0, 0) and raw_pending(core, 3) == (1, NO_RESULT, 0, 0)
    # a parsed id text
    text = b"5 6 -7 7\n\n%d 8 -1 2147483647 -2147483648\n9 9 9 x 4\n1 %d 0\n" % (V, V - 1)
    P = K.Placed(B, text, 3)
    nl, ni, _ = core.ids_parse_device_raw(P.ptr, len(text))
    assert (nl, ni) == (5, 15)
    for L, mode in ((4, STREAM), (5, WHOLE), (64, WHOLE)):
        pending_same(core, B, nl, ni, L, mode, PAD, "parse")
    assert raw_pending(core, nl + 1) == (1, NO_RESULT, 0, 0)
    # an empty batch is a result: no rows
    assert D.encode_device(core, B, [], 0, 0, 0) == 0
    core.blocks_discard()
    assert raw_pending(core, 0) == (0, "", 0, 0) and take(core, B, 0, 0, 8)[4].tolist() == [0]
    # a restricted vocabulary
    sents = to_bytes(sentences_of(name))[:60]
    n_plain = D.encode_device(core, B, sents, 1, 1, 0)
    allowed = np.zeros(V, np.uint8)
    allowed[:V // 2] = 1
    core.set_vocabulary(allowed)
    n_ids = D.encode_device(core, B, sents, 1, 1, 0)
    assert n_ids > n_plain
    pending_same(core, B, len(sents), n_ids, 50, STREAM, PAD, "restricted")
    ids, off = D.encode_fetch(core, len(sents), n_ids)
    pending_same(core, B, len(sents), n_ids, int(np.diff(off.astype(np.int64)).max()), WHOLE, KEEP, "restricted, whole")


def check_dropout(B, name="readme_small"):
    """dropout 0.1 and 1 under a pinned YTTM_DROPOUT_SEED: the blocks are those of the call's own ids"""
    with DC.env():
        core = D.core_of(name)
    sents = to_bytes(sentences_of(name))
    blob, off = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    plain = None
    for p in (0.0, 0.1, 1.0):
        n_ids, _ = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), len(sents), len(blob), max(map(len, sents)), False, False, False, p)
        ids, o = pending_same(core, B, len(sents), n_ids, 100, STREAM, PAD, "dropout %g" % p)
        pending_same(core, B, len(sents), n_ids, int(np.diff(o.astype(np.int64)).max()) + 3, WHOLE, PAD, "dropout %g, whole" % p)
        if p == 0.0:
            plain = n_ids
        else:
            assert n_ids > plain


# ---- case 9: the file route -----------------------------------------------------------------------------------------------------------------------
def read_files(prefix, L):
    rows = np.fromfile(prefix + ".rows", np.int32).reshape(-1, L)
    frags = np.fromfile(prefix + ".frags", np.uint64).reshape(-1, 2)
    return rows, frags


def check_file(B, tmp_path, name="readme_small", picks=None):
    """PREFIX.rows / PREFIX.frags whatever the piece size == the loops on encode_file's ids; lines and ids are encode_file's"""
    texts = [K.golden(name)[0], b"", b"\n", b"no newline Z", b"ab cd\n" * 150 + b"Z" * 50_000 + b"\n" + b"cd ab Z\n" * 150]
    for k, data in enumerate(texts):
        if picks is not None and k not in picks:
            continue
        path = str(tmp_path / f"in{k}.txt")
        open(path, "wb").write(data)
        core = D.core_of(name)
        b, e = (1, 1) if k % 2 == 0 else (0, 0)
        ids, off = core.encode_file(path, None, bool(b), bool(e), False)
        o = off.tolist()
        sents = [ids[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        longest = max([len(s) for s in sents] + [1])
        line_bytes = max([len(ln) for ln in K.py_split(data)] + [0]) + 1
        for mode, L in ((STREAM, 37), (WHOLE, max(longest, 9))):
            for tail in (PAD, DROP):
                want = py_blocks(sents, L, mode, PADV, tail)
                for j, (chunk, io_kb) in enumerate(((None, None), (max(len(data) // 8, 1), 1), (line_bytes - 2 if line_bytes > 2 else 1, 1), (1, None), (len(data) + 9, 1))):
                    old = os.environ.get("YTTM_IO_CHUNK_KB")
                    try:
                        if io_kb:
                            os.environ["YTTM_IO_CHUNK_KB"] = str(io_kb)
                        c2 = D.core_of(name)
                    finally:
                        os.environ.pop("YTTM_IO_CHUNK_KB", None)
                        if old is not None:
                            os.environ["YTTM_IO_CHUNK_KB"] = old
                    prefix = str(tmp_path / f"out{k}_{mode}_{tail}_{j}")
                    rep = c2.encode_file_blocks(path, prefix, L, mode, bool(b), bool(e), False, 0.0, PADV, tail, chunk, report=True)
                    rows, frags = read_files(prefix, L)
                    what = (k, mode, tail, chunk)
                    assert rows.tobytes() == want[0].tobytes(), what
                    assert frags.astype(np.int64).tolist() == want[3].astype(np.int64).tolist(), what
                    assert (rep["rows"], rep["frags"], rep["lines"], rep["ids"], rep["bytes"]) == (len(rows), len(frags), len(sents), len(ids), len(data)), what
                    assert {"pieces", "piece_bytes", "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_blocks",
                            "seconds_download_write"} <= set(rep)
                    if j == 1 and k == 0:
                        assert rep["pieces"] >= 5, rep
                    assert c2.blocks_open() == (0, 0, 0)


def check_file_dropout(tmp_path, name="readme_small"):
    """two fresh encoders under one pinned salt: the stripped PREFIX.rows equal encode_file's ids"""
    data = K.golden(name)[0]
    path = str(tmp_path / "in.txt")
    open(path, "wb").write(data)
    for p in (0.1, 1.0):
        for chunk in (None, max(len(data) // 8, 1)):
            with DC.env():
                a, b = D.core_of(name), D.core_of(name)
            ids, _ = a.encode_file(path, None, False, False, False, p, chunk)
            prefix = str(tmp_path / "out")
            nr, nf, nl, ni = b.encode_file_blocks(path, prefix, 40, STREAM, False, False, False, p, PADV, PAD, chunk)
            rows, frags = read_files(prefix, 40)
            flat = rows.ravel()
            assert ni == len(ids) and flat[:ni].tobytes() == ids.tobytes() and (flat[ni:] == PADV).all() and len(rows) == nr, (p, chunk)


def check_file_errors(B, tmp_path, name="readme_small"):
    import pytest
    bpe = SP.model(name).bpe
    core = bpe.bpe_cython
    txt = str(tmp_path / "in.txt")
    open(txt, "wb").write(b"ab Z\ncd\n\nab ab ab ab ab ab ab cd cd cd cd Z Z Z\ncd\n")
    out = str(tmp_path / "out")
    for run in (lambda p: bpe.encode_file_blocks(p, out, 16), lambda p: bpe.encode_file(p)):  # the same codes and messages as yttm_encode_file
        with pytest.raises(ValueError, match="Failed to open file: .*no_such_file"):
            run(str(tmp_path / "no_such_file.txt"))
        with pytest.raises(ValueError, match="Failed to read file: .* is not a regular file"):
            run(str(tmp_path))
    with pytest.raises(ValueError, match="Failed to open file for writing: .*no_such_dir"):
        bpe.encode_file_blocks(txt, str(tmp_path / "no_such_dir" / "out"), 16)
    nopad = SP.model("nopad").bpe
    with pytest.raises(ValueError, match=BOS_MSG):
        nopad.encode_file_blocks(txt, out, 16, bos=True, pad_id=0)
    with pytest.raises(ValueError, match=EOS_MSG):
        nopad.encode_file_blocks(txt, out, 16, eos=True, pad_id=0)
    with pytest.raises(ValueError, match="without <PAD>"):
        nopad.encode_file_blocks(txt, out, 16)
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_file_blocks(txt, out, 16, dropout_prob=2)
    with pytest.raises(ValueError, match="seq_len must be within"):
        bpe.encode_file_blocks(txt, out, 0)
    with pytest.raises(ValueError, match="mode must be"):
        bpe.encode_file_blocks(txt, out, 16, mode="best")
    err = C.create_string_buffer(_lib.ERRLEN)
    assert _lib.load().yttm_encode_file_blocks(core._h, os.fsencode(txt), os.fsencode(out), 0, 0, 0, 0.0, 0, 16, 0, 0, 1, None, None, None, None, None, 0, err,
                                               _lib.ERRLEN) == 1 and b"tail must be 0 (pad) or 2 (drop)" in err.value
    # a sentence longer than seq_len in whole mode names its line in the file, whatever the pieces
    ids, off = bpe.encode_file(txt)
    lens = np.diff(off.astype(np.int64))
    assert int(lens.argmax()) == 3
    for chunk in (None, 1):
        with pytest.raises(ValueError, match="seq_len is smaller than line 4: .*seq_len = %d; length = %d;" % (lens.max() - 1, lens.max())):
            bpe.encode_file_blocks(txt, out, int(lens.max()) - 1, mode="whole", chunk_bytes=chunk)
        assert bpe.blocks_open() == (0, 0, None)
    empty = str(tmp_path / "empty.txt")
    open(empty, "wb").close()
    rep = bpe.encode_file_blocks(empty, out, 16, report=True)
    assert (rep["rows"], rep["frags"], rep["lines"], rep["ids"], rep["pieces"]) == (0, 0, 0, 0, 0)
    assert os.path.getsize(out + ".rows") == 0 and os.path.getsize(out + ".frags") == 0
    # the lanes are as good as before
    nr, nf, nl, ni = bpe.encode_file_blocks(txt, out, int(lens.max()) + 2, mode="whole", bos=True, eos=True, pad_id=PADV)
    ids2, off2 = bpe.encode_file(txt, bos=True, eos=True)
    o = off2.tolist()
    want = py_blocks([ids2[o[i]:o[i + 1]] for i in range(len(o) - 1)], int(lens.max()) + 2, WHOLE, PADV, PAD)
    rows, frags = read_files(out, int(lens.max()) + 2)
    assert rows.tobytes() == want[0].tobytes() and (nr, nf, nl, ni) == (len(want[0]), len(want[3]), len(o) - 1, len(ids2))


# ---- case 10: Python and the command line ---------------------------------------------------------------------------------------------------------
def check_python_and_cli(tmp_path, name="readme_small"):
    """BPE.encode_file_blocks == the loops on encode_file's ids; `yttm blocks_file` writes the same files.  Three processes."""
    bpe = SP.model(name).bpe
    data = K.golden(name)[0]
    path, model_file = str(tmp_path / "in.txt"), SP.model_path(name)
    open(path, "wb").write(data)
    pad = bpe.subword_to_id("<PAD>")
    ids, off = bpe.encode_file(path, bos=True, eos=True)
    o = off.tolist()
    sents = [ids[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    longest = max(len(s) for s in sents)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli", "blocks_file", f"--model={model_file}", f"--input={path}"]
    runs = (("stream", 48, False, ["--seq_len=48"]), ("whole", longest + 1, True, [f"--seq_len={longest + 1}", "--mode=whole", "--drop_last"]),
            ("whole", longest, False, [f"--seq_len={longest}", "--mode", "whole"]))
    for k, (mode, L, drop, args) in enumerate(runs):
        want = py_blocks(sents, L, WHOLE if mode == "whole" else STREAM, pad, DROP if drop else PAD)
        out = str(tmp_path / f"py{k}")
        got = bpe.encode_file_blocks(path, out, L, mode=mode, bos=True, eos=True, drop_last=drop, chunk_bytes=len(data) // 4)
        assert got == (len(want[0]), len(want[3]), len(sents), len(ids))
        rows, frags = read_files(out, L)
        assert rows.tobytes() == want[0].tobytes() and frags.astype(np.int64).tolist() == want[3].astype(np.int64).tolist()
        cli_out = str(tmp_path / f"cli{k}")
        p = subprocess.run(cli + [f"--output={cli_out}", "--bos", "--eos"] + args, capture_output=True, env=env)
        assert p.returncode == 0, p.stderr.decode()
        for ext in (".rows", ".frags"):
            assert open(cli_out + ext, "rb").read() == open(out + ext, "rb").read(), (k, ext)


def check_tensor_api(name="readme_small"):
    """the BPE.*blocks*_tensor methods against the loops on encode_tensor's ids"""
    import pytest
    import torch
    import youtokentome_amd as yttm
    bpe = yttm.BPE(SP.model_path(name))
    dev = torch.device("cuda", bpe.bpe_cython.device)
    pad = bpe.subword_to_id("<PAD>")
    sents = sentences_of(name)[:50] + ["", "ab Z cd", "é中 ab", " "]
    ids, off = bpe.encode_tensor(sents, bos=True, padded=False)
    o = off.cpu().tolist()
    flat = ids.cpu().numpy()
    lists = [flat[o[i]:o[i + 1]] for i in range(len(sents))]
    longest = max(len(s) for s in lists)

    def host(b):
        assert all(t.device == dev for t in b) and [t.dtype for t in b] == [torch.int32] * 4 + [torch.int64]
        return tuple(t.cpu().numpy() for t in b[:4]) + (b.row_frags.cpu().numpy().view(np.uint64),)

    for mode, m, L in (("stream", STREAM, 33), ("whole", WHOLE, longest + 2)):
        want = py_blocks(lists, L, m, pad, PAD)
        b = bpe.encode_blocks_tensor(sents, L, mode=mode, bos=True)
        assert tuple(b.rows.shape) == want[0].shape and tuple(b.frags.shape) == want[3].shape
        equal(host(b), want[:5], "encode_blocks_tensor " + mode)
        props(host(b), flat, np.array(o), L, m, PAD, mode)
        equal(host(bpe.blocks_tensor(seq_len=L, mode=mode)), want[:5], "the pending result")
        equal(host(bpe.blocks_tensor(ids, offsets=off, seq_len=L, mode=mode)), want[:5], "a ragged tensor")
        matrix, lengths = bpe.encode_tensor(sents, bos=True)
        equal(host(bpe.blocks_tensor(matrix, lengths=lengths, seq_len=L, mode=mode, pad_id=pad)), want[:5], "a padded matrix")
        text = "\n".join(s.replace("\n", " ") for s in sents) + "\n"
        ids_t, off_t = bpe.encode_text_tensor(text.encode(), bos=True, padded=False)
        ot = off_t.cpu().tolist()
        ft = ids_t.cpu().numpy()
        want_t = py_blocks([ft[ot[i]:ot[i + 1]] for i in range(len(ot) - 1)], L, m, pad, DROP)
        equal(host(bpe.encode_text_blocks_tensor(text.encode(), L, mode=mode, bos=True, tail="drop")), want_t[:5], "text")
        # keep, then flush
        half = len(sents) // 2
        a = bpe.encode_blocks_tensor(sents[:half], L, mode=mode, bos=True, tail="keep")
        f_open = bpe.blocks_open()
        assert f_open[1:] == (L, mode) or f_open == (0, 0, None)
        with pytest.raises(ValueError, match="the open row holds"):
            if f_open[0]:
                bpe.encode_blocks_tensor(sents, L + 1, mode=mode)
            else:
                raise ValueError("the open row holds nothing")
        c = bpe.encode_blocks_tensor(sents[half:], L, mode=mode, bos=True, tail="keep")
        z = bpe.blocks_flush_tensor()
        assert bpe.blocks_open() == (0, 0, None)
        assert torch.equal(torch.cat([a.rows, c.rows, z.rows]), torch.from_numpy(want[0]).to(dev))
        assert torch.equal(torch.cat([a.seg, c.seg, z.seg]), torch.from_numpy(want[1]).to(dev))
    with pytest.raises(ValueError, match="seq_len is smaller than sentence"):
        bpe.encode_blocks_tensor(sents, longest - 1, mode="whole", bos=True)
    with pytest.raises(ValueError, match="mode must be"):
        bpe.encode_blocks_tensor(sents, 8, mode="best")
    with pytest.raises(ValueError, match="int32"):
        bpe.blocks_tensor(ids.to(torch.int64), offsets=off, seq_len=8)


# ---- case 11: one larger pass (MI355X) ------------------------------------------------------------------------------------------------------------
def check_large(B, name="zipf", n=50_000, width=128):
    """50 000 x 128-char sentences at L = 512 and 2048 in both modes through the property check: arrays only, no loop per token"""
    import gen
    core = D.core_of(name)
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=29, vocab=20000).replace(b"\n", b" ")[:n * width]
    data = b"".join(raw[i * width:(i + 1) * width] + b"\n" for i in range(n))
    P = K.Placed(B, data, 9)
    nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
    assert nl == n
    ids, off = core.fetch_encode(nl, ni)
    for L in (512, 2048):
        for mode in (STREAM, WHOLE):
            for tail in (PAD, DROP):
                core.blocks_discard()
                n_rows, n_frags, _ = core.blocks_device_raw(nl, L, mode, PADV, tail)
                got = core.fetch_blocks(n_rows, n_frags, L)
                props(got, ids, off, L, mode, tail, (L, mode, tail))
                assert (got[0][got[1] == 0] == PADV).all()
    assert core.fetch_encode(nl, ni)[0].tobytes() == ids.tobytes()
