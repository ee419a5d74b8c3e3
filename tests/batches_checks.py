"""Checks of the batches by length under a token budget made on the device (yttm_batches_plan_device, yttm_batches_plan_lengths_device,
yttm_batches_gather_device, yttm_batches_gather_ids_device, yttm_batches_fetch / _copy_device, the BPE.*batches*_tensor methods), shared by the
emulator tests (test_batches_device.py, test_batches_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests
(test_gpu_batches.py).

Two yardsticks that share no code:
  py_plan / py_gather   the rule of include/yttm_mi355x.h as plain Python loops: sorted() over the kept sentences, the greedy cut, the matrices
                        built row by row; every array is compared exactly;
  props / props_gather  properties computed with numpy array operations: order is a permutation whose kept prefix does not decrease in length
                        (ties by ascending index) and whose left-out tail ascends; every batch is within both limits and every batch but the
                        last is maximal; every element of every matrix is the id the rule puts there or pad_value, the padding on the side
                        asked for; widths is the row maximum.
Every case that is meant to exercise something asserts from the Python rule that it does.  The input lengths and ids sit at a chosen element
offset between guard values, every output array of the device exit has guard words behind it."""
import ctypes as C
import os

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import spans_checks as SP
from decode_checks import NumpyBuf, TorchBuf  # noqa: F401  (the buffers are re-exported)
from idcount_checks import PlacedIds
from spans_checks import all_models, model, sentences_of, to_bytes  # noqa: F401
from youtokentome_amd import _lib

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PADV = -9  # a pad value no generated id has
TILE, ORBIT, CHUNK = 4096, 8192, 2048  # BAT_TILE, BAT_ORBIT, BAT_CHUNK of yttm_kernels.h
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5000)
NO_BATCHES = ("fetch_batches: no matching batches", "copy_batches: no matching batches")
ORBIT_HOOK = "YTTM_BATCHES_ORBIT"


class Refused(Exception):
    pass


# ---- yardstick 1: the rule as loops -------------------------------------------------------------------------------------------------------------
def py_plan(lens, T, M=0, min_len=0, max_len=0):
    """-> (order, batch_first, n_kept); raises Refused(index, length) for the first sentence the rule refuses"""
    lens = [int(v) for v in lens]
    kept = []
    for i, ln in enumerate(lens):
        if ln < 0:
            raise Refused(i, ln)
        if min_len <= ln and (max_len == 0 or ln <= max_len):
            if ln > T:
                raise Refused(i, ln)
            kept.append(i)
    order = sorted(kept, key=lambda i: (lens[i], i))
    n_kept = len(order)
    first, a = [], 0
    while a < n_kept:
        b = a + 1
        while b < n_kept and (M == 0 or b + 1 - a <= M) and (b + 1 - a) * lens[order[b]] <= T:
            b += 1
        first.append(a)
        a = b
    first.append(n_kept)
    inside = set(kept)
    order += [i for i in range(len(lens)) if i not in inside]
    return np.array(order, np.uint32), np.array(first, np.uint64), n_kept


def py_gather(sents, order, first, pad, left):
    """-> (widths, batch_off, out), the matrices built row by row"""
    widths, off, out = [], [0], []
    for b in range(len(first) - 1):
        rows = [[int(v) for v in sents[int(order[p])]] for p in range(int(first[b]), int(first[b + 1]))]
        w = max(len(r) for r in rows)
        for r in rows:
            fill = [pad] * (w - len(r))
            out += fill + r if left else r + fill
        widths.append(w)
        off.append(len(out))
    return np.array(widths, np.uint32), np.array(off, np.uint64), np.array(out, np.int64).astype(np.int32)


# ---- yardstick 2: properties, array operations only ---------------------------------------------------------------------------------------------
def props(lens, T, M, min_len, max_len, order, first, n_kept, what=""):
    lens, order, first = np.asarray(lens, np.int64), order.astype(np.int64), first.astype(np.int64)
    n = len(lens)
    assert len(order) == n and np.array_equal(np.sort(order), np.arange(n)), what
    kept = (lens >= min_len) & ((lens <= max_len) if max_len else np.ones(n, bool))
    assert n_kept == int(kept.sum()), what
    kp, tail = order[:n_kept], order[n_kept:]
    assert kept[kp].all() and not kept[tail].any() and (np.diff(tail) > 0).all(), what
    lk = lens[kp]
    assert (np.diff(lk) >= 0).all() and (np.diff(kp)[np.diff(lk) == 0] > 0).all(), what
    assert first[-1] == n_kept and (first[0] == 0) and (np.diff(first) >= 1).all() and (len(first) > 1) == (n_kept > 0), what
    if n_kept:
        rows = np.diff(first)
        assert (rows * lk[first[1:] - 1] <= T).all() and (M == 0 or (rows <= M).all()), what
        more = rows[:-1] + 1
        assert (((more * lk[first[1:-1]]) > T) | ((more > M) if M else False)).all(), what


def props_gather(flat, off, order, first, widths, batch_off, out, pad, left, what=""):
    flat, off, order, first = np.asarray(flat, np.int64), np.asarray(off, np.int64), order.astype(np.int64), first.astype(np.int64)
    widths, batch_off, out = widths.astype(np.int64), batch_off.astype(np.int64), out.astype(np.int64)
    B, side = len(first) - 1, np.diff(off)
    rows = np.diff(first)
    assert len(widths) == B and len(batch_off) == B + 1, what
    if B:
        assert np.array_equal(widths, np.maximum.reduceat(side[order[:first[-1]]], first[:-1])), what
    assert np.array_equal(batch_off, np.concatenate([[0], np.cumsum(rows * widths)])) and len(out) == batch_off[-1], what
    E = len(out)
    b_of = np.repeat(np.arange(B), rows * widths)
    rel = np.arange(E) - batch_off[b_of]
    w = widths[b_of]
    r, c = rel // np.maximum(w, 1), rel % np.maximum(w, 1)
    s = order[first[b_of] + r]
    ln = side[s]
    shift = (w - ln) if left else np.zeros(E, np.int64)
    is_id = (c >= shift) & (c < shift + ln)
    assert int(is_id.sum()) == int((side[order[:first[-1]]]).sum()), what  # every id of every kept sentence, once
    assert np.array_equal(out[is_id], flat[(off[s] + c - shift)[is_id]]), what
    assert (out[~is_id] == pad).all(), what


# ---- the device path ----------------------------------------------------------------------------------------------------------------------------
def flatten(sents):
    off = np.zeros(len(sents) + 1, np.uint64)
    if len(sents):
        np.cumsum([len(s) for s in sents], out=off[1:])
    flat = np.concatenate([np.asarray(s, np.int64) for s in sents] + [np.zeros(0, np.int64)]).astype(np.int32)
    return flat, off


def take(core, B, n, n_batches, n_elems=None):
    """the slot by both exits, which must agree; the device copy writes the arrays and no more"""
    got = core.fetch_batches(n, n_batches, n_elems)
    sizes = [(n, np.uint32), (n_batches + 1, np.uint64)]
    if n_elems is not None:
        sizes += [(n_batches, np.uint32), (n_batches + 1, np.uint64), (n_elems, np.int32)]
    d = [B.empty(size + 3, np.int32 if dt == np.uint32 else dt) for size, dt in sizes]
    ptrs = [B.ptr(x) for x in d] + [None] * (5 - len(d))
    core.copy_batches_device(*ptrs, n, n_batches, n_elems or 0)
    for k, (x, (size, dt)) in enumerate(zip(d, sizes)):
        dev = B.get(x)
        assert dev[:size].tobytes() == got[k].tobytes(), "the two exits differ in array %d" % k
        assert dev[size:size + 3].view(np.int64 if dt == np.uint64 else np.int32).tolist() == [-7] * 3, "the copy wrote past array %d" % k
    return got


def raw_plan_lengths(core, ptr, n, T, M=0, min_len=0, max_len=0):
    nk, nb, err = C.c_uint64(77), C.c_uint64(77), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_batches_plan_lengths_device(core._h, C.c_void_p(ptr), n, T, M, min_len, max_len, C.byref(nk), C.byref(nb), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), nk.value, nb.value


def raw_plan(core, n, T, M=0, min_len=0, max_len=0):
    nk, nb, err = C.c_uint64(77), C.c_uint64(77), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_batches_plan_device(core._h, n, T, M, min_len, max_len, C.byref(nk), C.byref(nb), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), nk.value, nb.value


def raw_gather_ids(core, ptr, optr, n, n_ids, pad=PADV, left=0):
    ne, err = C.c_uint64(77), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_batches_gather_ids_device(core._h, C.c_void_p(ptr), C.c_void_p(optr), n, n_ids, pad, left, C.byref(ne), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), ne.value


def raw_gather(core, n, pad=PADV, left=0):
    ne, err = C.c_uint64(77), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_batches_gather_device(core._h, n, pad, left, C.byref(ne), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), ne.value


def equal(got, want, names, what):
    for g, w, name in zip(got, want, names):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g.ravel() != w.ravel())[0]
            raise AssertionError("%s: %s differs at %d of %d places, first %d: got %d want %d" % (what, name, len(bad), g.size, bad[0], g.ravel()[bad[0]],
                                                                                                  w.ravel()[bad[0]]))


def plan_same(core, B, lens, T, M=0, min_len=0, max_len=0, shift=0, what=""):
    """yttm_batches_plan_lengths_device on lengths placed at `shift`: device == loops, and the properties hold -> (order, batch_first, n_kept)"""
    what = "%s n %d T %d M %d min %d max %d" % (what, len(lens), T, M, min_len, max_len)
    lens = np.asarray(lens, np.int64)
    P = PlacedIds(B, lens.astype(np.int32), shift)
    n_kept, n_batches, _ = core.batches_plan_lengths_device_raw(P.ptr, len(lens), T, M, min_len, max_len)
    assert P.intact(), "the lengths or their guard values were written"
    order, first = take(core, B, len(lens), n_batches)
    want = py_plan(lens, T, M, min_len, max_len)
    assert n_kept == want[2], what
    equal((order, first), want[:2], ("order", "batch_first"), what)
    props(lens, T, M, min_len, max_len, order, first, n_kept, what)
    return order, first, n_kept


def gather_same(core, B, sents, plan, pad=PADV, left=False, shift=0, what=""):
    """yttm_batches_gather_ids_device of the side `sents` under the slot's plan: device == loops, and the properties hold"""
    order, first, _ = plan
    flat, off = flatten(sents)
    P = PlacedIds(B, flat, shift)
    d_off = B.put(off)
    n_elems, _ = core.batches_gather_ids_device_raw(P.ptr, B.ptr(d_off), len(sents), len(flat), pad, left)
    assert P.intact(), "the ids or their guard values were written"
    assert B.get(d_off).view(np.uint64).tolist() == off.tolist()
    got = take(core, B, len(sents), len(first) - 1, n_elems)
    equal(got[:2], (order, first), ("order", "batch_first"), what)
    equal(got[2:], py_gather(sents, order, first, pad, left), ("widths", "batch_off", "out"), what)
    props_gather(flat, off, *got, pad, left, what)
    return got


def ids_for(rng, lens, vocab=30000):
    return [rng.randint(0, vocab, size=int(k)).astype(np.int32) for k in lens]


def passes_of(T, max_len=0):
    cap = min(T, max_len) if max_len else T
    return ((cap + 1).bit_length() + 7) // 8


def tie_group(lens):
    return int(np.bincount(np.asarray(lens, np.int64)).max())


# ---- case 1: sizes ------------------------------------------------------------------------------------------------------------------------------
def check_sizes(B, sizes=SIZES, name="readme_small"):
    """random lengths in 0 .. 40 at T = 256; the small sizes and 5 000 also through the gather"""
    core = D.core_of(name)
    rng = np.random.RandomState(41)
    for n in sizes:
        lens = rng.randint(0, 41, size=n)
        plan = plan_same(core, B, lens, 256, shift=n % 4, what="sizes")
        if n >= 63:
            assert len(plan[1]) - 1 >= 2 and tie_group(lens) >= 3
        if n <= 257 or n == 5000:
            sents = ids_for(rng, lens)
            gather_same(core, B, sents, plan, left=bool(n & 1), shift=(n + 1) % 4, what="sizes, n %d" % n)


# ---- case 2: stability and hot digits -------------------------------------------------------------------------------------------------------------
def stability_cases():
    rng = np.random.RandomState(42)
    hot = rng.randint(0, 41, size=6000)
    hot[rng.permutation(6000)[:3000]] = 23
    return (("all equal", np.full(3000, 7), 256), ("strictly descending", np.arange(300, 0, -1), 512),
            ("descending in runs of 70", np.repeat(np.arange(40, 0, -1), 70), 256), ("two alternating", np.tile([3, 17], 1500), 256),
            ("64 distinct a wavefront", np.concatenate([rng.permutation(64) for _ in range(40)]), 256), ("one length 3000 times", hot, 256))


def check_stability(B, name="readme_small"):
    core = D.core_of(name)
    for what, lens, T in stability_cases():
        assert what == "strictly descending" or tie_group(lens) >= 3
        order, first, n_kept = plan_same(core, B, lens, T, what=what)
        assert len(first) - 1 >= 2
    lens = stability_cases()[5][1]
    assert int((lens == 23).sum()) >= 3000
    rng = np.random.RandomState(43)
    gather_same(core, B, ids_for(rng, lens[:700]), plan_same(core, B, lens[:700], 256, M=33), what="one length many times")


# ---- case 3: digit edges and pass counts (the lengths entry only) ---------------------------------------------------------------------------------
def check_digits(B, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(44)
    seen = set()
    for T, max_len in ((254, 0), (255, 0), (1000, 254), (1000, 255), (65534, 0), (65535, 0), (1 << 20, 65535), ((1 << 24) - 2, 0), ((1 << 24) - 1, 0),
                       ((1 << 24) + 1, 0), (I32_MAX, 0), (I32_MAX, 1 << 24)):
        edges = [v for e in (255, 256, 65535, 65536, 1 << 24) for v in (e - 1, e, e + 1)] + [I32_MAX - 1, I32_MAX]
        pool = np.array([v for v in edges if v <= T] + [0, 1, 2, 3], np.int64)
        lens = np.concatenate([pool, pool, rng.choice(pool, size=300), rng.randint(0, 50, size=200), np.minimum(rng.randint(0, 1 << 31, size=100), T)])
        rng.shuffle(lens)
        plan_same(core, B, lens, T, max_len=max_len, what="digits")
        plan_same(core, B, lens, T, M=5, min_len=2, max_len=max_len, what="digits")
        seen.add(passes_of(T, max_len))
    assert seen == {1, 2, 3, 4} and passes_of(255) == 2 and passes_of(254) == 1 and passes_of(65535) == 3 and passes_of(1000, 255) == 2
    # the largest T: a length of 2^31 - 1 is alone in its batch
    lens = np.array([5, I32_MAX, 0, 7, I32_MAX, 1 << 30, 1 << 30], np.int64)
    order, first, n_kept = plan_same(core, B, lens, I32_MAX, what="the largest T")
    assert order.tolist()[-2:] == [1, 4] and first.tolist()[-3:] == [5, 6, 7]


# ---- case 4: budget edges -------------------------------------------------------------------------------------------------------------------------
def state_of(core, B, n, n_batches, n_elems):
    return [a.tobytes() for a in take(core, B, n, n_batches, n_elems)]


def check_budget(B, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(45)
    order, first, _ = plan_same(core, B, [4] * 10, 12, what="exactly T")
    assert np.diff(first.astype(np.int64)).tolist() == [3, 3, 3, 1]  # 3 * 4 == T
    order, first, _ = plan_same(core, B, [4] * 10, 11, what="one more than T")
    assert np.diff(first.astype(np.int64)).tolist() == [2] * 5  # 3 * 4 == T + 1
    order, first, _ = plan_same(core, B, [5, 1, 1], 5, what="a sentence of exactly T")
    assert first.tolist() == [0, 2, 3] and order.tolist() == [1, 2, 0]
    order, first, _ = plan_same(core, B, [0, 1, 1, 0, 1], 1, what="T = 1")
    assert first.tolist() == [0, 2, 3, 4, 5]
    lens = np.concatenate([np.full(10, 1), np.full(10, 50), rng.randint(0, 20, size=200)])
    for M in (1, 2, 0, 4):
        order, first, _ = plan_same(core, B, lens, 100, M=M, what="M")
    rows = np.diff(first.astype(np.int64))
    last = lens[order.astype(np.int64)][first.astype(np.int64)[1:] - 1]
    assert ((rows == 4) & ((rows + 1) * last <= 100)).any() and ((rows < 4) & (last == 50)).any()  # M binds before T, and T before M
    for M, want in ((0, 1), (7, 3)):
        order, first, _ = plan_same(core, B, [0] * 20, 9, M=M, what="only empty sentences")
        assert len(first) - 1 == want
        got = gather_same(core, B, [[]] * 20, (order, first, 20), what="only empty sentences")
        assert got[2].tolist() == [0] * want and len(got[4]) == 0
    # a kept sentence of T + 1 ids: code 1 naming index and length; plan, gathered arrays and pending result unchanged
    sents = to_bytes(sentences_of(name))[:20]
    n_ids = D.encode_device(core, B, sents, 0, 0, 0)
    ids, off = D.encode_fetch(core, len(sents), n_ids)
    lens = rng.randint(0, 9, size=50)
    side = ids_for(rng, lens)
    plan = plan_same(core, B, lens, 16, what="before the refusal")
    got = gather_same(core, B, side, plan, what="before the refusal")
    before = state_of(core, B, 50, len(plan[1]) - 1, len(got[4]))
    T = 16
    for bad in ([3, 0, T + 1, 2, T + 5], [T + 1], [1] * 4500 + [T + 2, 1, T + 1]):
        d_l = B.put(np.array(bad, np.int32))
        rc, msg, nk, nb = raw_plan_lengths(core, B.ptr(d_l), len(bad), T)
        at = [v > T for v in bad].index(True)
        assert rc == 1 and "sentence %d:" % at in msg and "max_tokens = %d; length = %d;" % (T, bad[at]) in msg and (nk, nb) == (0, 0), msg
        assert state_of(core, B, 50, len(plan[1]) - 1, len(got[4])) == before
        try:
            py_plan(bad, T)
            raise AssertionError("the loops accept it")
        except Refused as e:
            assert e.args == (at, bad[at])
        plan_same(core, B, bad, T, max_len=T, what="left out by max_len")  # the same sentence left out: no error
        plan_same(core, B, lens, 16)
        gather_same(core, B, side, plan)
    ids2, off2 = K.take_encoded(core, B, len(sents), n_ids)
    assert ids2.tobytes() == ids.tobytes() and off2.tobytes() == off.tobytes()
    # the pending result's own sentence longer than T
    longest = int(np.diff(off.astype(np.int64)).max())
    at = int(np.diff(off.astype(np.int64)).argmax())
    rc, msg, _, _ = raw_plan(core, len(sents), longest - 1)
    assert rc == 1 and "sentence %d:" % at in msg and "length = %d;" % longest in msg, msg
    assert state_of(core, B, 50, len(plan[1]) - 1, len(got[4])) == before
    # a negative length names its index
    for bad in ([3, 4, -1, 5, -2], [1] * 300 + [I32_MIN]):
        d_l = B.put(np.array(bad, np.int32))
        rc, msg, nk, nb = raw_plan_lengths(core, B.ptr(d_l), len(bad), T)
        at = [v < 0 for v in bad].index(True)
        assert rc == 1 and "sentence %d has a negative length (%d)" % (at, bad[at]) in msg, msg
        assert state_of(core, B, 50, len(plan[1]) - 1, len(got[4])) == before
    # parameters outside their ranges, a misaligned pointer
    d_l = B.put(np.array([1, 2, 3, 4], np.int32))
    for T_bad, M_bad in ((0, 0), (1 << 31, 0), (8, 1 << 31)):
        rc, msg, _, _ = raw_plan_lengths(core, B.ptr(d_l), 4, T_bad, M_bad)
        assert rc == 1 and msg.startswith("batches: "), msg
    rc, msg, _, _ = raw_plan_lengths(core, B.ptr(d_l) + 2, 3, 8)
    assert rc != 0 and "4-byte aligned" in msg
    assert state_of(core, B, 50, len(plan[1]) - 1, len(got[4])) == before


# ---- case 5: the filter ---------------------------------------------------------------------------------------------------------------------------
def check_filter(B, name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(46)
    lens = rng.randint(0, 30, size=400)
    T = 20
    for min_len in (0, 1, 5):
        for max_len in (7, T, 0):
            _, _, n_kept = plan_same(core, B, np.minimum(lens, T) if max_len == 0 else lens, T, min_len=min_len, max_len=max_len, what="filter")
            assert 0 < n_kept < 400 or (min_len, max_len) == (0, 0)
    _, _, n_kept = plan_same(core, B, lens, 64, max_len=40, what="max_len above every length")
    assert n_kept == 400
    plan_same(core, B, lens, T, max_len=25, min_len=26, what="max_len above T, nothing kept")
    order, first, n_kept = plan_same(core, B, lens, T, min_len=31, what="everything left out")
    assert n_kept == 0 and first.tolist() == [0] and order.tolist() == list(range(400))
    got = gather_same(core, B, ids_for(rng, lens), (order, first, 0), what="everything left out")
    assert len(got[2]) == 0 and got[3].tolist() == [0]
    for what, lens in (("left out in front", [99] * 70 + [3] * 70), ("in the middle", [3] * 70 + [99] * 70 + [4] * 70), ("at the end", [3] * 70 + [99] * 70)):
        order, first, n_kept = plan_same(core, B, lens, 50, max_len=50, what=what)
        assert n_kept == lens.count(3) + lens.count(4)
        gather_same(core, B, ids_for(rng, lens), (order, first, n_kept), what=what)


# ---- case 6: the orbit ----------------------------------------------------------------------------------------------------------------------------
def core_with_orbit(name, orbit):
    old = os.environ.get(ORBIT_HOOK)
    try:
        if orbit:
            os.environ[ORBIT_HOOK] = str(orbit)
        else:
            os.environ.pop(ORBIT_HOOK, None)
        return D.core_of(name)
    finally:
        os.environ.pop(ORBIT_HOOK, None)
        if old is not None:
            os.environ[ORBIT_HOOK] = old


def jumps_a_block(first, orbit):
    f = first.astype(np.int64)
    return bool((f[1:] // orbit > f[:-1] // orbit + 1).any())


def check_orbit(B, name="readme_small", big=True):
    """a batch of 1 500 one-id sentences among 5 000: with blocks of 256 or 64 positions (the hook) `next` jumps over blocks; with the built block
    of 8 192 positions the same with 17 000 among 20 000"""
    rng = np.random.RandomState(47)
    lens = np.concatenate([np.full(1500, 1), rng.randint(2, 10, size=3500)])
    rng.shuffle(lens)
    want = None
    for orbit in (256, 64, 1000, 0):
        core = core_with_orbit(name, orbit)
        order, first, n_kept = plan_same(core, B, lens, 1600, what="1500 one-id sentences among 5000, orbit %d" % orbit)
        assert first.tolist()[:2] == [0, 1500]
        assert orbit in (0, 1000) or jumps_a_block(first, orbit)  # (1000: the hook rounds down to a multiple of 64)
        want = want or (order.tobytes(), first.tobytes())
        assert (order.tobytes(), first.tobytes()) == want
        # M = 1: as many batches as sentences; the last batch holds one sentence
        order, first, _ = plan_same(core, B, lens[:700], 1600, M=1, what="M = 1, orbit %d" % orbit)
        assert len(first) - 1 == 700
        order, first, _ = plan_same(core, B, [1] * 300 + [200], 300, what="a last batch of one sentence")
        assert first.tolist() == [0, 300, 301]
        order, first, _ = plan_same(core, B, lens[:900], 1 << 20, what="one batch")
        assert first.tolist() == [0, 900]
    if big:
        core = core_with_orbit(name, 0)
        lens = np.concatenate([np.full(17000, 1), rng.randint(2, 10, size=3000)])
        rng.shuffle(lens)
        order, first, _ = plan_same(core, B, lens, 17001, what="17000 one-id sentences among 20000")
        assert first.tolist()[:2] == [0, 17000] and jumps_a_block(first, ORBIT)
        order, first, _ = plan_same(core, B, lens, 40, what="20000 sentences, small batches")
        assert int(first[-2]) // ORBIT == 2  # the orbit visits every block


# ---- case 7: the gather ---------------------------------------------------------------------------------------------------------------------------
def check_gather(B, shifts=(0, 1, 2, 3), name="readme_small"):
    core = D.core_of(name)
    rng = np.random.RandomState(48)
    V = core.vocab_size()
    # widths, one batch of three rows each; every pad value, both sides
    widths = (0, 1, 3, 4, 5, 63, 64, 65, 1000)
    lens = np.repeat(widths, 3)
    lens[1::3] = np.maximum(lens[1::3] - 1, 0)  # (a shorter row in every batch: padding)
    rng.shuffle(lens)
    plan = plan_same(core, B, lens, 3000, M=3, what="widths")
    sents = ids_for(rng, lens)
    sents[0][:3] = [-1, I32_MIN, I32_MAX][:len(sents[0][:3])]
    sents[5] = np.array(([-1, I32_MIN, I32_MAX, 7] * 300)[:len(sents[5])], np.int32)
    for k, pad in enumerate((0, -1, 7, I32_MIN)):
        for left in (False, True):
            got = gather_same(core, B, sents, plan, pad=pad, left=left, shift=shifts[(k + left) % len(shifts)], what="widths, pad %d left %d" % (pad, left))
            assert sorted(set(got[2].tolist())) == sorted(widths)
    for s in shifts:  # the input ids at every element offset
        gather_same(core, B, sents, plan, left=bool(s & 1), shift=s, what="alignment %d" % s)
    # batches of one row and of 1000 rows
    lens = rng.randint(0, 9, size=150)
    gather_same(core, B, ids_for(rng, lens), plan_same(core, B, lens, 64, M=1, what="one row"), what="one row")
    lens = np.concatenate([np.full(1000, 2), [3, 3]])
    plan = plan_same(core, B, lens, 2000, what="1000 rows")
    assert np.diff(plan[1].astype(np.int64)).tolist() == [1000, 2]
    gather_same(core, B, ids_for(rng, lens), plan, left=True, what="1000 rows")
    # a chunk boundary on a batch's end (32 rows of 64), on a row's end inside a batch (40 rows of 64), inside a row (rows of 1000)
    for rows, w in ((32, 64), (40, 64), (5, 1000)):
        lens = np.full(3 * rows, w)
        plan = plan_same(core, B, lens, rows * w, what="chunk boundary")
        off = plan[1].astype(np.int64) * w
        assert ((rows * w) % CHUNK == 0) == (CHUNK in off.tolist()) and (CHUNK % w == 0) == (w == 64) and off[-1] > CHUNK
        for left in (False, True):
            gather_same(core, B, ids_for(rng, lens), plan, left=left, shift=3, what="chunk boundary %d x %d" % (rows, w))
    # many batches of width 0 in a row: on the planned side in front, on a second side anywhere
    lens = np.concatenate([np.zeros(300, np.int64), rng.randint(1, 9, size=200)])
    rng.shuffle(lens)
    plan = plan_same(core, B, lens, 32, M=2, what="width 0")
    got = gather_same(core, B, ids_for(rng, lens), plan, what="width 0")
    assert (got[2][:150] == 0).all()
    second = lens.copy()
    second[:7] += 40
    second[plan[0].astype(np.int64)[340:420]] = 0
    second[plan[0].astype(np.int64)[421]] = 0  # an empty sentence of this side in a batch that holds ids
    got = gather_same(core, B, ids_for(rng, second), plan, left=True, what="a second side")
    assert (got[2][170:210] == 0).all() and got[2][210] > 0 and got[2].max() > 40
    # more than 2^31 - 1 elements: refused from the offsets alone (the ids do not exist), and the gathered part stays
    before = state_of(core, B, 500, len(plan[1]) - 1, len(got[4]))
    huge = np.zeros(501, np.uint64)
    huge[1:] = 1 << 31
    d_i, d_o = B.put(np.zeros(4, np.int32)), B.put(huge)
    rc, msg, ne = raw_gather_ids(core, B.ptr(d_i), B.ptr(d_o), 500, 1 << 31)
    assert rc == 1 and "exceed 2^31 - 1 elements" in msg and ne == 0, msg
    assert state_of(core, B, 500, len(plan[1]) - 1, len(got[4])) == before
    plan = plan_same(core, B, [1 << 30] * 3 + [5], I32_MAX, what="3 x 2^30")
    huge = np.array([0, 1 << 30, 2 << 30, 3 << 30, (3 << 30) + 5], np.uint64)
    d_o = B.put(huge)
    rc, msg, ne = raw_gather_ids(core, B.ptr(d_i), B.ptr(d_o), 4, int(huge[-1]))
    assert rc == 1 and "exceed 2^31 - 1 elements (%d)" % ((3 << 30) + 5) in msg, msg
    assert [a.tobytes() for a in take(core, B, 4, 4)] == [plan[0].tobytes(), plan[1].tobytes()]


# ---- case 8: the slot and the exits ---------------------------------------------------------------------------------------------------------------
def check_slot(B, name="readme_small"):
    core = D.core_of(name)
    L0 = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    rng = np.random.RandomState(49)

    def raw_take(n, n_batches, n_elems, which=0):
        """both exits asked for one array: [(code, message)]; nothing is written where they refuse"""
        out = []
        host = np.full(256, 9, np.int32)
        args = [None] * 5
        args[which] = host.ctypes.data_as(C.c_void_p)
        out.append((L0.yttm_batches_fetch(core._h, *args, n, n_batches, n_elems, err, _lib.ERRLEN), err.value.decode()))
        d = B.empty(256, np.int32)
        args[which] = C.c_void_p(B.ptr(d))
        out.append((L0.yttm_batches_copy_device(core._h, *args, n, n_batches, n_elems, err, _lib.ERRLEN), err.value.decode()))
        if out[0][0]:
            assert set(host.tolist()) == {9} and set(B.get(d).tolist()) == {-7}
        return out

    refused = [(1, NO_BATCHES[0]), (1, NO_BATCHES[1])]
    assert raw_take(0, 0, 0) == refused, "before any plan"
    lens = rng.randint(0, 9, size=40)
    sents = ids_for(rng, lens)
    flat, off = flatten(sents)
    d_i, d_o = B.put(flat), B.put(off)
    rc, msg, ne = raw_gather_ids(core, B.ptr(d_i), B.ptr(d_o), 40, len(flat))
    assert rc == 1 and "no plan" in msg and ne == 0, msg
    order, first, n_kept = plan_same(core, B, lens, 16, what="slot")
    nb = len(first) - 1
    for n_wrong in (39, 41, 0):
        rc, msg, ne = raw_gather_ids(core, B.ptr(d_i), B.ptr(d_o), n_wrong, len(flat))
        assert rc == 1 and "the plan is of 40 sentences" in msg, msg
    rc, msg, ne = raw_gather_ids(core, B.ptr(d_i) + 2, B.ptr(d_o), 40, len(flat))
    assert rc != 0 and "4-byte aligned" in msg
    # nothing gathered yet: the plan alone leaves by the exits; the gathered arrays do not, and n_elems is 0
    assert raw_take(40, nb, 0, which=4) == refused and raw_take(40, nb, 0, which=2) == refused and raw_take(40, nb, 5) == refused
    got = gather_same(core, B, sents, (order, first, n_kept), what="slot")
    ne = len(got[4])
    for wrong in ((39, nb, ne), (40, nb + 1, ne), (40, nb, ne + 1), (40, nb, 0), (0, 0, 0)):  # wrong counts at the exits
        assert raw_take(*wrong) == refused, wrong
    for k in range(5):  # null pointers are skipped: each array alone equals the full fetch
        assert [rc for rc, _ in raw_take(40, nb, ne, which=k)] == [0, 0]
        buf = B.empty(got[k].size + 8, np.int64 if got[k].dtype == np.uint64 else np.int32)
        args = [None] * 5
        args[k] = B.ptr(buf)
        core.copy_batches_device(*args, 40, nb, ne)
        assert B.get(buf)[:got[k].size].tobytes() == got[k].tobytes(), k
    # the plan and the gathered part survive an encode, a blocks call, an id-count call and a decode
    before = state_of(core, B, 40, nb, ne)
    bs = to_bytes(sentences_of(name))[:10]
    n_ids = D.encode_device(core, B, bs, 1, 1, 0)
    core.blocks_device_raw(len(bs), 16, 0, PADV, 0)
    core.blocks_discard()
    core.id_counts_device_raw(len(bs), core.vocab_size())
    assert state_of(core, B, 40, nb, ne) == before
    # the pending result is not the plan's: the gather of the pending result is refused by n_sent, the plan's own side still goes
    rc, msg, _ = raw_gather(core, len(bs))
    assert rc == 1 and "the plan is of 40 sentences" in msg, msg
    rc, msg, _ = raw_gather(core, 40)
    assert rc == 1 and "no matching encode result" in msg, msg
    assert state_of(core, B, 40, nb, ne) == before
    # a second gather replaces the gathered part only; a new plan empties it
    got2 = gather_same(core, B, sents, (order, first, n_kept), pad=3, left=True, what="a second gather")
    assert got2[4].tobytes() != got[4].tobytes()
    plan_same(core, B, lens, 16, M=2, what="a new plan")
    nb2 = core.batches_last_plan[2]
    assert raw_take(40, nb2, len(got2[4]), which=4) == refused and raw_take(40, nb2, 0, which=4) == refused
    assert [rc for rc, _ in raw_take(40, nb2, 0, which=0)] == [0, 0]


# ---- case 9: pending results ----------------------------------------------------------------------------------------------------------------------
def pending_same(core, B, n, n_ids, T, M=0, min_len=0, max_len=0, left=False, what=""):
    """the pending result of n sentences: plan + gather == the loops on the fetched ids; the result fetches the same bytes afterwards"""
    ids, off = D.encode_fetch(core, n, n_ids)
    o = off.tolist()
    sents = [ids[o[i]:o[i + 1]] for i in range(n)]
    lens = np.diff(off.astype(np.int64)) if n else np.zeros(0, np.int64)
    n_kept, n_batches, _ = core.batches_plan_device_raw(n, T, M, min_len, max_len)
    n_elems, _ = core.batches_gather_device_raw(n, PADV, left)
    got = take(core, B, n, n_batches, n_elems)
    want = py_plan(lens, T, M, min_len, max_len)
    assert n_kept == want[2], what
    equal(got[:2], want[:2], ("order", "batch_first"), what)
    equal(got[2:], py_gather(sents, want[0], want[1], PADV, left), ("widths", "batch_off", "out"), what)
    props(lens, T, M, min_len, max_len, got[0], got[1], n_kept, what)
    props_gather(ids, off, *got, PADV, left, what)
    ids2, off2 = K.take_encoded(core, B, n, n_ids)
    assert ids2.tobytes() == ids.tobytes() and off2.tobytes() == off.tobytes(), what
    return got


def check_pending_model(B, name):
    """a golden model, the flag sets it allows: yttm_encode_device + yttm_batches_plan_device + yttm_batches_gather_device"""
    M = model(name)
    core = D.core_of(name)
    sents = to_bytes(sentences_of(name))
    for k, (b, e, r) in enumerate(M.flags()):
        n_ids = D.encode_device(core, B, sents, b, e, r)
        _, off = D.encode_fetch(core, len(sents), n_ids)
        longest = int(np.diff(off.astype(np.int64)).max())
        got = pending_same(core, B, len(sents), n_ids, longest + k, M=(0, 5)[k % 2], left=bool(k & 1), what=(name, b, e, r))
        assert len(got[1]) - 1 >= 2 or n_ids <= longest + k  # (ids beyond the budget: more than one batch)
        pending_same(core, B, len(sents), n_ids, longest, min_len=2, max_len=longest - 1, what=(name, b, e, r, "filter"))


def check_pending_misc(B, name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    no = "batches_plan_device: no matching encode result"
    assert raw_plan(core, 0, 8) == (1, no, 0, 0) and raw_plan(core, 3, 8) == (1, no, 0, 0)
    # a parsed id text
    text = b"5 6 -7 7\n\n%d 8 -1 2147483647 -2147483648\n9 9 9 x 4\n1 %d 0\n" % (V, V - 1)
    P = K.Placed(B, text, 3)
    nl, ni, _ = core.ids_parse_device_raw(P.ptr, len(text))
    assert (nl, ni) == (5, 15)
    for T, Mx in ((5, 0), (8, 2), (64, 0)):
        pending_same(core, B, nl, ni, T, M=Mx, what="parse")
    assert raw_plan(core, nl + 1, 8) == (1, no, 0, 0)
    # an empty batch is a result: a plan of no sentences
    assert D.encode_device(core, B, [], 0, 0, 0) == 0
    assert raw_plan(core, 0, 8) == (0, "", 0, 0) and raw_gather(core, 0) == (0, "", 0)
    got = take(core, B, 0, 0, 0)
    assert got[1].tolist() == [0] and got[3].tolist() == [0]
    # a restricted vocabulary
    sents = to_bytes(sentences_of(name))[:60]
    n_plain = D.encode_device(core, B, sents, 1, 1, 0)
    allowed = np.zeros(V, np.uint8)
    allowed[:V // 2] = 1
    core.set_vocabulary(allowed)
    n_ids = D.encode_device(core, B, sents, 1, 1, 0)
    assert n_ids > n_plain
    pending_same(core, B, len(sents), n_ids, 400, left=True, what="restricted")


def check_dropout(B, name="readme_small"):
    """dropout 0.1 and 1 under a pinned YTTM_DROPOUT_SEED: the batches are those of the call's own ids"""
    with DC.env():
        core = D.core_of(name)
    sents = to_bytes(sentences_of(name))
    blob, off = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    plain = None
    for p in (0.0, 0.1, 1.0):
        n_ids, _ = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), len(sents), len(blob), max(map(len, sents)), False, False, False, p)
        pending_same(core, B, len(sents), n_ids, 2000, M=7, what="dropout %g" % p)
        if p == 0.0:
            plain = n_ids
        else:
            assert n_ids > plain


# ---- MI355X only ----------------------------------------------------------------------------------------------------------------------------------
def check_tensor_api(name="readme_small"):
    """the BPE.*batches*_tensor methods against the loops on encode_tensor's ids"""
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
    lens = np.diff(np.array(o))
    T = 3 * int(lens.max())

    def check(b, want_plan, left, pad_value, side=lists):
        assert all(t.device == dev for t in (b.order, b.batch_first, b.widths, b.batch_off, b.ids))
        assert [t.dtype for t in (b.order, b.batch_first, b.widths, b.batch_off, b.ids)] == [torch.int32, torch.int64, torch.int32, torch.int64, torch.int32]
        assert b.order.cpu().numpy().view(np.uint32).tolist() == want_plan[0].tolist() and b.batch_first.cpu().tolist() == want_plan[1].tolist()
        assert b.n_kept == want_plan[2] and len(b) == len(want_plan[1]) - 1
        w, bo, out = py_gather(side, want_plan[0], want_plan[1], pad_value, left)
        assert b.widths.cpu().tolist() == w.tolist() and b.batch_off.cpu().tolist() == bo.tolist() and b.ids.cpu().numpy().tobytes() == out.tobytes()
        base = b.ids.data_ptr()
        for k, (idx, m) in enumerate(b):
            a, e = int(want_plan[1][k]), int(want_plan[1][k + 1])
            assert idx.cpu().tolist() == want_plan[0][a:e].astype(np.int64).tolist() and tuple(m.shape) == (e - a, int(w[k]))
            assert m.numel() == 0 or m.data_ptr() == base + 4 * int(bo[k])  # a view, not a copy
            assert m.cpu().numpy().tobytes() == out[int(bo[k]):int(bo[k + 1])].tobytes()
        assert len(b) == 0 or (b[-1][1].shape == b[len(b) - 1][1].shape)
        with pytest.raises(IndexError):
            b[len(b)]

    want = py_plan(lens, T, 6, 1, 0)
    b = bpe.encode_batches_tensor(sents, T, max_sentences=6, min_len=1, bos=True)
    check(b, want, False, pad)  # pad_id defaults to the model's <PAD>
    check(bpe.encode_batches_tensor(sents, T, max_sentences=6, min_len=1, bos=True, left_pad=True, pad_id=-5), want, True, -5)
    text = "\n".join(s.replace("\n", " ") for s in sents) + "\n"
    ids_t, off_t = bpe.encode_text_tensor(text.encode(), bos=True, padded=False)
    ot, ft = off_t.cpu().tolist(), ids_t.cpu().numpy()
    lists_t = [ft[ot[i]:ot[i + 1]] for i in range(len(ot) - 1)]
    check(bpe.encode_text_batches_tensor(text.encode(), T, bos=True), py_plan(np.diff(np.array(ot)), T), False, pad, lists_t)
    # the plan alone, then each of two sides under it
    tgt = [lst[::2] for lst in lists]
    both = np.maximum(lens, [len(t) for t in tgt]).astype(np.int32)
    plan = bpe.batches_plan_tensor(torch.from_numpy(both).to(dev), T, max_sentences=9)
    want = py_plan(both, T, 9)
    assert plan.ids is None and plan.order.cpu().numpy().view(np.uint32).tolist() == want[0].tolist() and len(plan) == len(want[1]) - 1
    assert plan[0][1] is None and plan[0][0].cpu().tolist() == want[0][:int(want[1][1])].astype(np.int64).tolist()
    check(bpe.batches_gather_tensor(ids, offsets=off, pad_id=pad), want, False, pad)
    tflat, toff = flatten(tgt)
    check(bpe.batches_gather_tensor(torch.from_numpy(tflat).to(dev), offsets=torch.from_numpy(toff.astype(np.int64)).to(dev), left_pad=True), want, True, pad, tgt)
    matrix, lengths = bpe.encode_tensor(sents, bos=True)
    check(bpe.batches_gather_tensor(matrix, lengths=lengths), want, False, pad)
    with pytest.raises(ValueError, match="max_tokens is smaller than sentence"):
        bpe.encode_batches_tensor(sents, int(lens.max()) - 1, bos=True)
    with pytest.raises(ValueError, match="int32"):
        bpe.batches_plan_tensor(torch.from_numpy(both.astype(np.int64)).to(dev), T)
    with pytest.raises(ValueError, match="without <PAD>"):
        yttm.BPE(SP.model_path("nopad")).encode_batches_tensor(["ab"], 8)


def check_large(B, name="zipf", n=50_000, width=128):
    """50 000 x 128-char sentences at T = 4 096 and 16 384 through the property checks: arrays only, no loop per sentence"""
    import gen
    core = D.core_of(name)
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=29, vocab=20000).replace(b"\n", b" ")[:n * width]
    data = b"".join(raw[i * width:(i + 1) * width] + b"\n" for i in range(n))
    P = K.Placed(B, data, 9)
    nl, ni, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
    assert nl == n
    ids, off = core.fetch_encode(nl, ni)
    lens = np.diff(off.astype(np.int64))
    for T, M, min_len, left in ((4096, 0, 0, False), (16384, 0, 0, True), (4096, 64, int(np.median(lens)), True)):
        n_kept, n_batches, _ = core.batches_plan_device_raw(nl, T, M, min_len, 0)
        n_elems, _ = core.batches_gather_device_raw(nl, PADV, left)
        got = core.fetch_batches(nl, n_batches, n_elems)
        props(lens, T, M, min_len, 0, got[0], got[1], n_kept, (T, M))
        props_gather(ids, off, *got, PADV, left, (T, M))
        assert n_batches >= 100
    assert core.fetch_encode(nl, ni)[0].tobytes() == ids.tobytes()
