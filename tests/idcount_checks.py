"""Checks of the token frequencies made on the device (yttm_id_counts_device, yttm_id_counts_ids_device, yttm_id_counts_fetch / _copy_device,
yttm_encode_file_counts, BPE.id_counts_tensor, BPE.count_file, `yttm count_file`), shared by the emulator tests (test_idcount_device.py,
test_idcount_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests (test_gpu_idcount.py: torch tensors).

The yardstick everywhere is numpy.bincount -- of the synthetic array itself, or of the ids the EXISTING routes return (yttm_encode_fetch,
encode_file) --, with the out-of-range tally computed in numpy from the rule of include/yttm_mi355x.h: counts[n_bins] = the ids outside
[0, n_bins).  Every comparison is exact.  Every synthetic array sits at a chosen element offset between guard values that would be counted
(they are valid ids) if the kernel read past either end."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import spans_checks as SP
from decode_checks import G, NumpyBuf, TorchBuf, golden_names  # noqa: F401  (the buffers are re-exported)
from spans_checks import BOS_MSG, EOS_MSG, FLAGS, all_models, model, sentences_of, to_bytes  # noqa: F401
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
HOOK = "YTTM_IDCOUNT_WINDOW"
STRIDE = 8192  # ids a workgroup takes per step: 16 wavefronts x 128 units of 16 bytes (idcount_plan.h)
GUARD = 64     # guard ids on either side
GUARD_ID = 5
BINS = 600
NO_COUNTS = ("fetch_id_counts: no matching counts", "copy_id_counts: no matching counts")
NO_RESULT = "id_counts_device: no matching encode result"


def built_window():
    """the largest window the kernel is built with: the default of its hook in the library's table"""
    L = _lib.load()
    L.yttm_config_table.restype = C.c_char_p
    for row in L.yttm_config_table().decode().splitlines():
        cols = [c.strip() for c in row.strip().strip("|").split("|")]
        if cols and cols[0] == "`%s`" % HOOK:
            return int(cols[1])
    raise AssertionError(HOOK + " is no row of the hook table")


@contextlib.contextmanager
def window(value):
    """the hook for the encoders made inside (None: unset); whatever stood before comes back"""
    old = os.environ.get(HOOK)
    try:
        os.environ.pop(HOOK, None)
        if value is not None:
            os.environ[HOOK] = str(value)
        yield
    finally:
        os.environ.pop(HOOK, None)
        if old is not None:
            os.environ[HOOK] = old


def np_counts(ids, n_bins):
    """the rule: bincount of the ids inside [0, n_bins), the rest tallied in the last slot"""
    ids = np.asarray(ids, np.int64).ravel()
    inside = (ids >= 0) & (ids < n_bins)
    out = np.zeros(n_bins + 1, np.uint64)
    out[:n_bins] = np.bincount(ids[inside], minlength=n_bins)
    out[n_bins] = len(ids) - int(inside.sum())
    assert int(out.sum()) == len(ids)
    return out


class PlacedIds:
    """int32 ids starting `shift` elements (0 .. 15) behind a 64-byte boundary inside a larger buffer of guard ids"""

    def __init__(self, B, ids, shift=0):
        ids = np.asarray(ids, np.int32)
        self.B, self.n = B, len(ids)
        host = np.full(GUARD + 16 + self.n + GUARD, GUARD_ID, np.int32)
        self.buf = B.put(host)
        base = B.ptr(self.buf)
        assert base % 4 == 0
        self.start = GUARD + ((4 * shift - (base + 4 * GUARD)) % 64) // 4
        host[self.start:self.start + self.n] = ids
        self.host = host
        if isinstance(self.buf, np.ndarray):
            self.buf[:] = host
        else:
            self.buf.copy_(B.torch.from_numpy(host.copy()))
            B.torch.cuda.synchronize()
        assert self.ptr % 64 == 4 * shift

    @property
    def ptr(self):
        return self.B.ptr(self.buf) + 4 * self.start

    def intact(self):
        return self.B.get(self.buf).tobytes() == self.host.tobytes()


def take_counts(core, B, n_bins, n_arg=None):
    """the counts by both exits, which must agree; the device copy writes n_bins + 1 values and no more"""
    n_arg = n_bins if n_arg is None else n_arg
    got = core.fetch_id_counts(n_arg)
    assert got.dtype == np.uint64 and len(got) == n_bins + 1
    d = B.empty(n_bins + 3, np.uint64)
    core.copy_id_counts_device(B.ptr(d), n_arg)
    dev = B.get(d).view(np.uint64)
    assert dev[:n_bins + 1].tolist() == got.tolist(), "the two exits differ"
    assert dev[n_bins + 1:].view(np.int64).tolist() == [-7, -7], "the copy wrote past the counts"
    return got


def dev_count(core, B, ids, n_bins, shift=0, accumulate=False):
    """yttm_id_counts_ids_device on ids placed at `shift`: the counts; the ids and their guards stay as they were"""
    P = PlacedIds(B, ids, shift)
    core.id_counts_ids_device_raw(P.ptr, P.n, n_bins, accumulate)
    assert P.intact(), "the ids or their guard values were written"
    return take_counts(core, B, n_bins)


def same(core, B, ids, n_bins, shift=0, what=""):
    got, want = dev_count(core, B, ids, n_bins, shift), np_counts(ids, n_bins)
    if got.tolist() != want.tolist():
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s n_ids %d n_bins %d shift %d: %d bins differ, first %d: got %d want %d" % (
            what, len(ids), n_bins, shift, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    assert int(got.sum()) == len(ids)


def random_ids(rng, n, n_bins, outside=0.05):
    """uniform over the bins, a share of them outside on both sides"""
    ids = rng.randint(0, n_bins, size=n).astype(np.int64)
    out = rng.rand(n) < outside
    ids[out] = rng.choice([-1, -77, n_bins, n_bins + 3, I32_MIN, I32_MAX], size=int(out.sum()))
    return ids.astype(np.int32)


def zipf_ids(rng, n, n_bins):
    """a Zipf draw, exponent 1: id k with probability ~ 1 / (k + 1)"""
    p = 1.0 / np.arange(1, n_bins + 1)
    return rng.choice(n_bins, size=n, p=p / p.sum()).astype(np.int32)


# ---- case 1: sizes and alignment ------------------------------------------------------------------------------------------------------------
def check_sizes(B, shifts=(0, 1, 2, 3), big=200_000, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(11)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1):
        ids = random_ids(rng, n, BINS)
        for s in shifts:
            same(core, B, ids, BINS, s, "sizes")
    ids = random_ids(rng, big + 3, BINS)
    for s in shifts[:2] + shifts[-1:]:
        same(core, B, ids, BINS, s, "sizes, large")
    # a head and a tail with nothing between them: fewer ids than reach the first boundary, and just past it
    for n in (1, 2, 3, 4, 5, 6, 7):
        for s in (1, 2, 3, 13, 14, 15):
            if s in shifts:
                same(core, B, random_ids(rng, n, BINS), BINS, s, "head and tail")


# ---- case 2: edge values ---------------------------------------------------------------------------------------------------------------------
def check_edge_values(B, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(12)
    edges = [0, BINS - 1, BINS, -1, I32_MIN, I32_MAX]
    for v in edges:
        same(core, B, [v], BINS, 1, "edge value alone")
        same(core, B, [v] * 130, BINS, 2, "edge value repeated")
    ids = random_ids(rng, 5000, BINS, outside=0.0)
    ids[rng.choice(5000, size=600, replace=False)] = np.resize(np.array(edges, np.int64), 600).astype(np.int32)
    same(core, B, ids, BINS, 3, "edge values mixed in")
    same(core, B, np.array(edges * 50, np.int64).astype(np.int32), BINS, 0, "edge values only")
    # every id outside: only the tally counts
    got = dev_count(core, B, np.full(3000, -5, np.int32), BINS)
    assert got[BINS] == 3000 and int(got[:BINS].sum()) == 0


# ---- case 3: hot bins ------------------------------------------------------------------------------------------------------------------------
def check_hot_bins(B, big=200_000, wide=40_000, name="readme_small"):
    W = built_window()
    rng = np.random.RandomState(13)
    with window(64):  # a window edge inside 600 bins
        core = D.core_of(name)
        for v in (0, 63, 64, BINS - 1):
            same(core, B, np.full(big, v, np.int32), BINS, 1, "one id %d, window 64" % v)
    core = D.core_of(name)
    assert wide > W
    for v in (0, W - 1, W, wide - 1):
        same(core, B, np.full(big, v, np.int32), wide, 3, "one id %d" % v)
    same(core, B, np.resize(np.array([7, 7, 3], np.int32), big), BINS, 0, "two ids, uneven")
    same(core, B, np.resize(np.array([2, 590], np.int32), big), BINS, 2, "two alternating ids")
    same(core, B, np.resize(np.array([W - 1, W], np.int32), big // 4), wide, 2, "two alternating ids across the window's edge")
    same(core, B, np.resize(np.arange(64, dtype=np.int32) * 9, big), BINS, 1, "64 distinct ids repeating")
    same(core, B, np.resize(np.arange(64, dtype=np.int32) * 9, big)[::-1].copy(), BINS, 1, "64 distinct ids repeating, backwards")
    same(core, B, zipf_ids(rng, big, BINS), BINS, 0, "Zipf over 600")
    same(core, B, zipf_ids(rng, big, wide), wide, 1, "Zipf over 40 000")


# ---- case 4: window edges --------------------------------------------------------------------------------------------------------------------
def check_window_hook(B, n=30_000, name="readme_small"):
    rng = np.random.RandomState(14)
    ids = random_ids(rng, n, BINS)
    ids[:3] = [BINS - 1, 0, BINS]
    want = np_counts(ids, BINS).tolist()
    for w in (0, 1, 64, 599, 600, 601, None):
        with window(w):
            core = D.core_of(name)
        assert dev_count(core, B, ids, BINS, 1).tolist() == want, "window %s" % w


def check_window_built(B, n=50_000, name="readme_small"):
    W = built_window()
    assert W >= 1024
    core = D.core_of(name)
    rng = np.random.RandomState(15)
    for n_bins in (W - 1, W, W + 1, 2 * W + 1, 100_000):
        ids = random_ids(rng, n, n_bins)
        ids[:8] = [0, W - 2, W - 1, min(W, n_bins - 1), n_bins - 1, n_bins, -1, I32_MAX]
        same(core, B, ids, n_bins, 2, "built window")


# ---- case 5: accumulate ----------------------------------------------------------------------------------------------------------------------
def raw_ids(core, ptr, n, n_bins, acc):
    err = C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_id_counts_ids_device(core._h, C.c_void_p(ptr), n, n_bins, acc, None, err, _lib.ERRLEN)
    return rc, err.value.decode()


def raw_take(core, B, n_bins):
    """(code, message) of both exits for a request that must fail"""
    L, err, out = _lib.load(), C.create_string_buffer(_lib.ERRLEN), []
    host = np.full(max(n_bins, 1) + 1 if n_bins < (1 << 20) else 8, 9, np.uint64)
    rc = L.yttm_id_counts_fetch(core._h, host.ctypes.data_as(_lib.u64p), n_bins, err, _lib.ERRLEN)
    out.append((rc, err.value.decode()))
    assert set(host.tolist()) == {9}
    d = B.empty(len(host), np.uint64)
    rc = L.yttm_id_counts_copy_device(core._h, C.c_void_p(B.ptr(d)), n_bins, err, _lib.ERRLEN)
    out.append((rc, err.value.decode()))
    assert set(B.get(d).view(np.int64).tolist()) == {-7}
    return out


def check_accumulate(B, name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    assert raw_take(core, B, BINS) == [(1, NO_COUNTS[0]), (1, NO_COUNTS[1])], "before any count"
    assert raw_take(core, B, 0) == [(1, NO_COUNTS[0]), (1, NO_COUNTS[1])]
    rng = np.random.RandomState(16)
    a, b = random_ids(rng, 7000, BINS), random_ids(rng, 901, BINS)
    once = np_counts(a, BINS)
    assert dev_count(core, B, a, BINS, 1).tolist() == once.tolist()
    assert dev_count(core, B, a, BINS, 2, accumulate=True).tolist() == (2 * once).tolist()
    assert dev_count(core, B, b, BINS, 3, accumulate=True).tolist() == (2 * once + np_counts(b, BINS)).tolist()
    # another n_bins on top: code 1, and the slot is as it was
    P = PlacedIds(B, a, 0)
    rc, msg = raw_ids(core, P.ptr, P.n, BINS + 1, 1)
    assert rc == 1 and "accumulate needs the n_bins of the counts so far (600, not 601)" in msg, msg
    rc, msg = raw_ids(core, P.ptr, P.n, 7, 1)
    assert rc == 1 and "(600, not 7)" in msg
    assert take_counts(core, B, BINS).tolist() == (2 * once + np_counts(b, BINS)).tolist()
    for wrong in (BINS - 1, BINS + 1, 7):
        assert raw_take(core, B, wrong) == [(1, NO_COUNTS[0]), (1, NO_COUNTS[1])], wrong
    # accumulate == 0 resets, the last slot included
    out = np.full(50, -3, np.int32)
    assert dev_count(core, B, out, BINS).tolist() == np_counts(out, BINS).tolist()
    assert dev_count(core, B, b, BINS).tolist() == np_counts(b, BINS).tolist()
    # no ids at all: zeroes, or the counts so far
    assert dev_count(core, B, [], BINS, accumulate=True).tolist() == np_counts(b, BINS).tolist()
    assert dev_count(core, B, [], BINS).tolist() == [0] * (BINS + 1)
    # n_bins == 0 is the vocabulary's size, for the count and for both exits
    ids = random_ids(rng, 3000, V)
    P = PlacedIds(B, ids, 1)
    assert raw_ids(core, P.ptr, P.n, 0, 0) == (0, "")
    assert take_counts(core, B, V, 0).tolist() == take_counts(core, B, V, V).tolist() == np_counts(ids, V).tolist()
    # accumulate on an encoder that has not counted yet starts from zero
    fresh = D.core_of(name)
    assert dev_count(fresh, B, b, BINS, accumulate=True).tolist() == np_counts(b, BINS).tolist()
    # n_bins beyond 2^31, a misaligned address
    rc, msg = raw_ids(core, P.ptr, P.n, (1 << 31) + 1, 0)
    assert rc == 1 and "n_bins" in msg
    rc, msg = raw_ids(core, P.ptr + 2, 4, BINS, 0)
    assert rc != 0 and "4-byte aligned" in msg
    assert take_counts(core, B, V).tolist() == np_counts(ids, V).tolist()


# ---- case 6: pending results -----------------------------------------------------------------------------------------------------------------
def raw_pending(core, n_sent, n_bins=0, acc=0):
    nc, err = C.c_uint64(7), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_id_counts_device(core._h, n_sent, n_bins, acc, C.byref(nc), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), nc.value


def count_pending_same(core, B, n, n_ids, what):
    """the pending result of n sentences: counts == bincount of the fetched ids, and the result fetches the same bytes afterwards"""
    V = core.vocab_size()
    ids, off = D.encode_fetch(core, n, n_ids)
    n_counted, _ = core.id_counts_device_raw(n)
    assert n_counted == n_ids, what
    got = take_counts(core, B, V)
    assert got.tolist() == np_counts(ids, V).tolist(), what
    ids2, off2 = K.take_encoded(core, B, n, n_ids)
    assert ids2.tobytes() == ids.tobytes() and off2.tobytes() == off.tobytes(), what
    return ids, got


def check_pending_model(B, name):
    """a golden model, the flag sets it allows, both encode entries"""
    M = model(name)
    core = D.core_of(name)
    sents = to_bytes(sentences_of(name))
    data = b"\n".join(s.replace(b"\n", b" ") for s in sents) + b"\n"
    for b, e, r in M.flags():
        n_ids = D.encode_device(core, B, sents, b, e, r)
        ids_a, _ = count_pending_same(core, B, len(sents), n_ids, (name, b, e, r, "encode_device"))
        assert n_ids > 0 and int(ids_a.min()) >= 0
        P = K.Placed(B, data, 5)
        nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), bool(b), bool(e), bool(r))
        count_pending_same(core, B, nl, ni, (name, b, e, r, "encode_text_device"))
        assert P.intact()


def check_pending_misc(B, name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    # no pending result at all
    assert raw_pending(core, 0) == (1, NO_RESULT, 0) and raw_pending(core, 3) == (1, NO_RESULT, 0)
    assert raw_take(core, B, 0)[0] == (1, NO_COUNTS[0])
    # a parse: negative and oversized numbers land in the last slot
    text = b"5 6 -7 7\n\n%d 8 -1 2147483647 -2147483648\n9 9 9 x 4\n1 %d 0\n" % (V, V - 1)
    P = K.Placed(B, text, 3)
    nl, ni, _ = core.ids_parse_device_raw(P.ptr, len(text))
    assert (nl, ni) == (5, 15)
    ids, got = count_pending_same(core, B, nl, ni, "parse")
    assert got[V] == 5 and sorted(ids.tolist())[:2] == [I32_MIN, -7]
    # a wrong n_sent: code 1, counts and result as they were
    assert raw_pending(core, nl + 1) == (1, NO_RESULT, 0) and raw_pending(core, 0) == (1, NO_RESULT, 0)
    assert take_counts(core, B, V).tolist() == got.tolist()
    assert K.take_encoded(core, B, nl, ni)[0].tolist() == ids.tolist()
    # spans stay pending beside the ids
    sents = [b"ab Z cd", b"", "é中 ab".encode(), b"abcd " * 40]
    blob, off = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    n_ids, _ = core.spans_device_raw(B.ptr(d_b), B.ptr(d_o), len(sents), len(blob), max(map(len, sents)))
    spans = core.fetch_spans(len(sents), n_ids)
    count_pending_same(core, B, len(sents), n_ids, "spans")
    assert core.fetch_spans(len(sents), n_ids).tolist() == spans.tolist()
    # other bins, and an encode after a count leaves the counts fetchable
    ids, _ = D.encode_fetch(core, len(sents), n_ids)
    core.id_counts_device_raw(len(sents), 7)
    want7 = np_counts(ids, 7)
    assert take_counts(core, B, 7).tolist() == want7.tolist() and want7[7] > 0
    n2 = D.encode_device(core, B, [b"cd ab", b"Z"], 0, 0, 0)
    assert take_counts(core, B, 7).tolist() == want7.tolist()
    core.id_counts_device_raw(2, 7, True)
    assert take_counts(core, B, 7).tolist() == (want7 + np_counts(D.encode_fetch(core, 2, n2)[0], 7)).tolist()
    # an empty batch is a result: zero ids counted
    assert D.encode_device(core, B, [], 0, 0, 0) == 0
    assert raw_pending(core, 0) == (0, "", 0) and take_counts(core, B, V).tolist() == [0] * (V + 1)


# ---- case 7: dropout -------------------------------------------------------------------------------------------------------------------------
def check_dropout(B, name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    sents = to_bytes(sentences_of(name))
    blob, off = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    plain = None
    for p in (0.0, 0.1, 1.0):
        n_ids, _ = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), len(sents), len(blob), max(map(len, sents)), False, False, False, p)
        _, got = count_pending_same(core, B, len(sents), n_ids, "dropout %g" % p)  # (exact: it counts what this very call produced)
        assert got[V] == 0
        if p == 0.0:
            plain = n_ids
        else:
            assert n_ids > plain  # (dropped merges leave more tokens)


# ---- case 8: the file route ------------------------------------------------------------------------------------------------------------------
def file_counts(core, path, b=0, e=0, r=0, dropout=0.0, chunk=None):
    """yttm_encode_file_counts: (counts, report)"""
    return core.encode_file_counts(path, bool(b), bool(e), bool(r), dropout, chunk, report=True)


def check_file(B, tmp_path, name="readme_small", picks=None):
    """the counts of a file whatever the piece size == bincount of encode_file's ids; lines and ids are encode_file's"""
    texts = [K.golden(name)[0], b"", b"\n", b"no newline Z", b"ab cd\n" * 150 + b"Z" * 50_000 + b"\n" + b"cd ab Z\n" * 150]
    for k, data in enumerate(texts):
        if picks is not None and k not in picks:
            continue
        path = str(tmp_path / f"in{k}.txt")
        open(path, "wb").write(data)
        longest = max([len(ln) for ln in K.py_split(data)] + [0]) + 1
        for b, e, r in FLAGS if k == 0 else ((0, 0, 0), (1, 1, 1)):
            core = D.core_of(name)
            V = core.vocab_size()
            ids, off = core.encode_file(path, None, bool(b), bool(e), bool(r))
            want = np_counts(ids, V)
            assert want[V] == 0
            for j, (chunk, io_kb) in enumerate(((None, None), (max(len(data) // 8, 1), 1), (longest - 2 if longest > 2 else 1, 1), (1, None), (len(data) + 9, 1))):
                old = os.environ.get("YTTM_IO_CHUNK_KB")
                try:
                    if io_kb:
                        os.environ["YTTM_IO_CHUNK_KB"] = str(io_kb)
                    c2 = D.core_of(name)
                finally:
                    os.environ.pop("YTTM_IO_CHUNK_KB", None)
                    if old is not None:
                        os.environ["YTTM_IO_CHUNK_KB"] = old
                got, rep = file_counts(c2, path, b, e, r, 0.0, chunk)
                assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (k, b, e, r, chunk)
                assert (rep["lines"], rep["ids"], rep["bytes"]) == (len(off) - 1, len(ids), len(data))
                assert {"pieces", "piece_bytes", "seconds_total", "seconds_read_upload", "seconds_split", "seconds_encode", "seconds_count",
                        "seconds_download_write"} <= set(rep)
                if j == 1 and k == 0:
                    assert rep["pieces"] >= 5, rep
                if j in (0, 4) and data:
                    assert rep["pieces"] == 1, rep
                assert take_counts(c2, B, V).tolist() == want.tolist()  # the slot holds the file's counts afterwards
                assert c2.encode_file_counts(path, bool(b), bool(e), bool(r), 0.0, chunk).tolist() == want.tolist()  # ... and a second call starts from zero


def check_file_dropout(tmp_path, name="readme_small"):
    data = K.golden(name)[0]
    path = str(tmp_path / "in.txt")
    open(path, "wb").write(data)
    core = D.core_of(name)
    V = core.vocab_size()
    plain, rep0 = file_counts(core, path)
    for p in (0.1, 1.0):
        for chunk in (None, max(len(data) // 8, 1)):
            got, rep = file_counts(core, path, 0, 0, 0, p, chunk)
            assert int(got.sum()) == rep["ids"] and got[V] == 0 and rep["lines"] == rep0["lines"] and rep["ids"] > rep0["ids"]
    # Two fresh encoders under one pinned salt (YTTM_DROPOUT_SEED, dropout_checks.env) cut the file alike and key piece k's draws alike -- by the
    # salt and the encoder's call number --, so there the counts ARE the bincount of encode_file's ids
    for p in (0.1, 1.0):
        for chunk in (None, max(len(data) // 8, 1)):
            with DC.env():
                a, b = D.core_of(name), D.core_of(name)
            ids, _ = a.encode_file(path, None, False, False, False, p, chunk)
            got, rep = file_counts(b, path, 0, 0, 0, p, chunk)
            assert got.tolist() == np_counts(ids, V).tolist() and rep["ids"] == len(ids), (p, chunk)


def check_file_errors(B, tmp_path, name="readme_small"):
    import pytest
    bpe = SP.model(name).bpe
    core = bpe.bpe_cython
    V = core.vocab_size()
    txt = str(tmp_path / "in.txt")
    open(txt, "wb").write(b"ab Z\ncd\n")
    want = np_counts(bpe.encode_file(txt)[0], V)
    assert bpe.count_file(txt).tolist() == want.tolist()
    for run in (bpe.count_file, lambda p: bpe.encode_file(p)):  # the same codes and messages as yttm_encode_file
        with pytest.raises(ValueError, match="Failed to open file: .*no_such_file"):
            run(str(tmp_path / "no_such_file.txt"))
        with pytest.raises(ValueError, match="Failed to read file: .* is not a regular file"):
            run(str(tmp_path))
    locked = str(tmp_path / "locked.txt")
    open(locked, "wb").write(b"ab\n")
    os.chmod(locked, 0)
    if not os.access(locked, os.R_OK):  # (root reads anything)
        for run in (bpe.count_file, lambda p: bpe.encode_file(p)):
            with pytest.raises(ValueError, match="Failed to open file: .*locked.txt .*Permission denied"):
                run(locked)
    # a failed call leaves the counts that were there
    assert take_counts(core, B, V).tolist() == want.tolist()
    nopad = SP.model("nopad").bpe
    with pytest.raises(ValueError, match=BOS_MSG):
        nopad.count_file(txt, bos=True)
    with pytest.raises(ValueError, match=EOS_MSG):
        nopad.count_file(txt, eos=True)
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.count_file(txt, dropout_prob=2)
    empty = str(tmp_path / "empty.txt")
    open(empty, "wb").close()
    got, rep = bpe.count_file(empty, report=True)
    assert got.tolist() == [0] * (V + 1) and (rep["lines"], rep["ids"], rep["pieces"]) == (0, 0, 0)
    L, err, z = _lib.load(), C.create_string_buffer(_lib.ERRLEN), C.c_uint64()
    assert L.yttm_encode_file_counts(core._h, os.fsencode(txt), 0, 0, 0, 0.0, 0, None, C.byref(z), C.byref(z), None, 0, err, _lib.ERRLEN) == 2
    # the lanes are as good as before
    assert bpe.count_file(txt, bos=True, eos=True).tolist() == np_counts(bpe.encode_file(txt, bos=True, eos=True)[0], V).tolist()


# ---- case 9: Python and the command line -----------------------------------------------------------------------------------------------------
def check_count_file_and_cli(tmp_path, name="readme_small"):
    """BPE.count_file == the C route == bincount of encode_file; `yttm count_file`: the columns of `yttm vocab` and the counts.  Three processes."""
    bpe = SP.model(name).bpe
    core = bpe.bpe_cython
    V = bpe.vocab_size()
    data = K.golden(name)[0]
    path, model_file = str(tmp_path / "in.txt"), SP.model_path(name)
    open(path, "wb").write(data)
    for b, e in ((False, False), (True, True)):
        want = np_counts(bpe.encode_file(path, bos=b, eos=e)[0], V)
        got = bpe.count_file(path, bos=b, eos=e)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and got.shape == (V + 1,) and got.tolist() == want.tolist()
        assert file_counts(core, path, b, e)[0].tolist() == want.tolist()
        got2, rep = bpe.count_file(path, bos=b, eos=e, chunk_bytes=len(data) // 4, report=True)
        assert got2.tolist() == want.tolist() and rep["pieces"] >= 3 and rep["ids"] == int(want.sum())
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def run(args):
        p = subprocess.run(cli + args, capture_output=True, env=env)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout

    vocab_lines = run(["vocab", f"--model={model_file}"]).split(b"\n")[:-1]
    assert len(vocab_lines) == V
    out = str(tmp_path / "counts.tsv")
    assert run(["count_file", f"--model={model_file}", f"--input={path}", f"--output={out}", "--bos", "--eos"]) == b""
    printed = run(["count_file", f"--model={model_file}", f"--input={path}", "--bos", "--eos"])
    assert open(out, "rb").read() == printed
    lines = printed.split(b"\n")
    assert lines[-1] == b"" and len(lines) == V + 1
    for i, (ln, vl) in enumerate(zip(lines, vocab_lines)):
        assert ln == vl + b"\t%d" % int(want[i]), (i, ln, vl)
        assert ln.split(b"\t")[0] == b"%d" % i


def check_tensor_api(name="readme_small"):
    """BPE.id_counts_tensor: the pending result of the *_tensor calls, a slice of a padded matrix, a ragged tensor"""
    import pytest
    import torch
    bpe = SP.model(name).bpe
    V = bpe.vocab_size()
    sents = sentences_of(name)[:50] + ["", "ab Z cd", "é中 ab", " "]
    dev = torch.device("cuda", bpe.bpe_cython.device)
    import youtokentome_amd as yttm
    fresh = yttm.BPE(SP.model_path(name))
    with pytest.raises(ValueError, match="no \\*_tensor encode or parse call"):
        fresh.id_counts_tensor()
    ids, off = bpe.encode_tensor(sents, bos=True, padded=False)
    got = bpe.id_counts_tensor()
    assert got.dtype == torch.int64 and got.device == dev and tuple(got.shape) == (V + 1,)
    assert got.cpu().numpy().view(np.uint64).tolist() == np_counts(ids.cpu().numpy(), V).tolist()
    assert torch.equal(bpe.id_counts_tensor(ids), got)  # a ragged tensor
    assert torch.equal(bpe.id_counts_tensor(ids, accumulate=True), 2 * got)
    m, lengths = bpe.encode_tensor(sents, eos=True, pad_id=V + 5)
    assert torch.equal(bpe.id_counts_tensor(n_bins=V).cpu(), torch.from_numpy(np_counts(np.concatenate([m[i, :int(lengths[i])].cpu().numpy() for i in range(len(sents))]), V).view(np.int64)))
    for rows in (slice(0, len(sents)), slice(3, 17), slice(1, 2)):  # a slice of rows starts anywhere and is contiguous: the pad values are ids like any other
        part = m[rows]
        got = bpe.id_counts_tensor(part, n_bins=V)
        assert got.cpu().numpy().view(np.uint64).tolist() == np_counts(part.cpu().numpy(), V).tolist()
        assert int(got[V]) == int((part == V + 5).sum())
    got = bpe.id_counts_tensor(m[:, 1:3].contiguous(), n_bins=11)
    assert tuple(got.shape) == (12,) and got.cpu().numpy().view(np.uint64).tolist() == np_counts(m[:, 1:3].cpu().numpy(), 11).tolist()
    with pytest.raises(ValueError, match="contiguous"):
        bpe.id_counts_tensor(m[:, 1:3])
    with pytest.raises(ValueError, match="int32"):
        bpe.id_counts_tensor(m.to(torch.int64))
    with pytest.raises(ValueError, match="is on cpu"):
        bpe.id_counts_tensor(m.cpu())
    with pytest.raises(ValueError, match="accumulate needs the n_bins"):
        bpe.id_counts_tensor(ids, n_bins=V + 1, accumulate=True)
    text = b"5 6 -7\n8\n"
    p_ids, p_off = bpe.parse_ids_tensor(text)
    assert bpe.id_counts_tensor().cpu().numpy().view(np.uint64).tolist() == np_counts([5, 6, -7, 8], V).tolist()
    assert torch.equal(bpe.parse_ids_tensor(text)[0], p_ids)


# ---- case 10: one larger pass (MI355X) -------------------------------------------------------------------------------------------------------
def check_large_pending(B, name="zipf", n=50_000, width=128):
    """the large shape of the sibling checks through the pending route"""
    import gen
    core = D.core_of(name)
    V = core.vocab_size()
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=29, vocab=20000).replace(b"\n", b" ")[:n * width]
    data = b"".join(raw[i * width:(i + 1) * width] + b"\n" for i in range(n))
    P = K.Placed(B, data, 9)
    nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
    assert nl == n
    ids, _ = core.fetch_encode(nl, ni)
    n_counted, _ = core.id_counts_device_raw(nl)
    assert n_counted == ni
    assert core.fetch_id_counts().tolist() == np_counts(ids, V).tolist()
    assert core.fetch_encode(nl, ni)[0].tobytes() == ids.tobytes()


def check_large_array(n=1 << 24, n_bins=40_000):
    """2^24 Zipf ids at 40 000 bins through the array route, against torch.bincount moved to the host"""
    import torch
    import youtokentome_amd as yttm
    bpe = yttm.BPE(SP.model_path("readme_small"))
    dev = torch.device("cuda", bpe.bpe_cython.device)
    g = torch.Generator(device="cpu").manual_seed(17)
    p = 1.0 / torch.arange(1, n_bins + 1, dtype=torch.float64)
    ids = torch.multinomial(p, n, replacement=True, generator=g).to(torch.int32)
    ids[::1001] = -1
    ids[5::4001] = n_bins
    d_ids = ids.to(dev)
    got = bpe.id_counts_tensor(d_ids[3:], n_bins=n_bins).cpu()
    inside = d_ids[3:][(d_ids[3:] >= 0) & (d_ids[3:] < n_bins)]
    want = torch.bincount(inside.to(torch.int64), minlength=n_bins).cpu()
    assert torch.equal(got[:n_bins], want) and int(got[n_bins]) == n - 3 - inside.numel() and int(got.sum()) == n - 3
