"""Checks of the encode under a restricted vocabulary (yttm_encoder_set_vocabulary, yttm_encoder_vocabulary_stats, yttm_restrict_ids_device,
BPE.set_vocabulary / vocabulary_info / vocabulary_stats / restrict_tensor, `yttm ... --vocabulary`), shared by the emulator tests
(test_restrict_device.py, test_restrict_device_sched.py: numpy arrays are "device" memory there) and the MI355X tests (test_gpu_restrict.py:
torch tensors).

Two yardsticks that share no code:
  1. the rule of include/yttm_mi355x.h as a Python recursion over z -> (x, y), the rules parsed from the model file behind its char section
     (Rules.table, want_rows) -- applied to the UNRESTRICTED ids of the same call; every comparison is exact;
  2. properties (check_props): BPE.decode of the result == BPE.decode of the unrestricted ids, byte for byte; every output id is allowed, a leaf
     or out of range; restricting the result again changes nothing.
Every case that is not the identity asserts from the oracle that at least one id of its input splits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import decode_checks as D
import dropout_checks as DC
import lines_checks as K
import spans_checks as SP
import subword_checks as SW
from decode_checks import G, NumpyBuf, TorchBuf  # noqa: F401  (the buffers are re-exported)
from spans_checks import FLAGS, all_models, model_path, sentences_of, to_bytes  # noqa: F401
from youtokentome_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 64
SEG = 508  # ids a wavefront stages at once (k_restrict.h RST_SEG)
NO_VOCAB = "restrict_ids_device: no vocabulary is set"


# ---- yardstick 1: the rule ---------------------------------------------------------------------------------------------------------------------
class Rules:
    """the rules (x, y, z) of a model file: "n_chars n_rules", n_chars pairs, then n_rules triples"""

    def __init__(self, path, V):
        tok = open(path).read().split()
        n, m = int(tok[0]), int(tok[1])
        at = 2 + 2 * n
        self.rules = [tuple(int(t) for t in tok[at + 3 * i:at + 3 * i + 3]) for i in range(m)]
        self.by_z = {z: (x, y) for x, y, z in self.rules}
        assert len(self.by_z) == m, "the rules' z are distinct"
        self.V = V

    def table(self, allowed):
        """{v: E(v)} for v of [0, V): the recursion E(z) = E(x) ++ E(y), unrolled on a stack (a chain of merges is deeper than Python's)"""
        V, by_z, E = self.V, self.by_z, {}
        assert len(allowed) == V
        for v in range(V):
            out, stack = [], [v]
            while stack:
                t = stack.pop()
                if t in E:
                    out.extend(E[t])
                elif allowed[t] or t not in by_z:
                    out.append(t)
                else:
                    stack.append(by_z[t][1])
                    stack.append(by_z[t][0])
            E[v] = out
        return E

    def info(self, allowed):
        E = self.table(allowed)
        return (int(np.count_nonzero(allowed)), sum(1 for e in E.values() if len(e) > 1), max(len(e) for e in E.values()))

    def masks(self, counts=None, threshold=2):
        """the masks every case uses: name -> bool [V]"""
        V, m = self.V, {}
        m["all"] = np.ones(V, bool)
        m["none"] = np.zeros(V, bool)
        m["odd"] = np.ones(V, bool)
        for i, (_, _, z) in enumerate(self.rules):
            if i % 2 == 1:
                m["odd"][z] = False
        m["low"] = np.arange(V) < self.rules[len(self.rules) // 2][2]
        if counts is not None:
            m["counts"] = np.asarray(counts[:V]) >= threshold
        return m


def want_rows(E, rows, rev):
    """a sentence's restricted ids: the concatenation of E(id) in forward order; of a sentence stored back to front the reverse of that"""
    out = []
    for r in rows:
        fwd = r[::-1] if rev else r
        e = [u for t in fwd for u in E.get(t, (t,))]  # (an id outside [0, V) is in no table: it stays)
        out.append(e[::-1] if rev else e)
    return out


def want_flat(E, V, ids, rev):
    """the same for one flat array whose sentences need no telling apart (the expansion of an id does not depend on its neighbours), in numpy"""
    L = np.array([len(E[v]) for v in range(V)], np.int64)
    src = np.zeros(V + 1, np.int64)
    np.cumsum(L, out=src[1:])
    flat = np.array([u for v in range(V) for u in (E[v][::-1] if rev else E[v])], np.int64)
    ids = np.asarray(ids, np.int64)
    inside = (ids >= 0) & (ids < V)
    safe = np.where(inside, ids, 0)
    lens = np.where(inside, L[safe], 1)
    start = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(lens, out=start[1:])
    k = np.arange(int(start[-1])) - np.repeat(start[:-1], lens)
    out = flat[np.repeat(src[safe], lens) + k]
    out[np.repeat(~inside, lens)] = ids[~inside]
    return out.astype(np.int32), start


# ---- the device path ---------------------------------------------------------------------------------------------------------------------------
class PlacedIds:
    """int32 ids starting `shift` elements (0 .. 15) behind a 64-byte boundary inside a larger buffer of guard ids"""

    def __init__(self, B, ids, shift, guard):
        ids = np.asarray(ids, np.int32)
        self.B, self.n = B, len(ids)
        host = np.full(GUARD + 16 + self.n + GUARD, guard, np.int32)
        self.buf = B.put(host)
        base = B.ptr(self.buf)
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


def stats(core):
    return np.array(core.vocabulary_stats(), np.int64)


def dev_restrict(core, B, rows, rev=0, shift=0, guard=5):
    """yttm_restrict_ids_device on ids placed at `shift` between guards: the rows of the pending result, taken by both exits (which check the two
    ids behind the result against a guard); the input and its guards stay as they were; the counters move by this call"""
    flat, off = D.flatten(rows)
    P = PlacedIds(B, flat, shift, guard)
    d_off = B.put(off)
    before = stats(core)
    n_out, _ = core.restrict_ids_device_raw(P.ptr, B.ptr(d_off), len(rows), len(flat), bool(rev))
    assert P.intact(), "the ids or their guard values were written"
    assert B.get(d_off).view(np.uint64).tolist() == off.tolist(), "the offsets were written"
    ids, o = K.take_encoded(core, B, len(rows), n_out)
    got = K.rows(ids, o)
    moved = stats(core) - before
    assert moved.tolist() == [1, 1 if n_out == len(flat) else 0, len(flat), n_out], moved
    return got


def raw_restrict(core, p_ids, p_off, n_sent, n_ids, rev=0):
    n, err = C.c_uint64(7), C.create_string_buffer(_lib.ERRLEN)
    rc = _lib.load().yttm_restrict_ids_device(core._h, C.c_void_p(p_ids), C.c_void_p(p_off), n_sent, n_ids, rev, C.byref(n), None, err, _lib.ERRLEN)
    return rc, err.value.decode(), n.value


# ---- yardstick 2: properties -------------------------------------------------------------------------------------------------------------------
def check_props(core, B, R, allowed, in_rows, out_rows, rev, what=""):
    V = R.V
    valid = [k for k, r in enumerate(in_rows) if all(0 <= t < V for t in r)]
    if valid:
        step = -1 if rev else 1  # (the text of a sentence stored back to front is that of its ids read back to front)
        a = core.decode([in_rows[k][::step] for k in valid], None)
        b = core.decode([out_rows[k][::step] for k in valid], None)
        assert a == b, (what, "the restricted ids decode to other text")
    for r in out_rows:
        for t in r:
            assert t < 0 or t >= V or allowed[t] or t not in R.by_z, (what, "an id that should have split", t)
    assert dev_restrict(core, B, out_rows, rev, 3) == out_rows, (what, "restricting twice is not restricting once")


def same(core, B, R, E, allowed, rows, what, shifts=(0,), revs=(0, 1), guard=5, splits=True, props=True):
    for rev in revs:
        want = want_rows(E, rows, rev)
        if splits:
            assert want != rows, (what, "nothing splits: the case proves nothing")
        for s in shifts:
            got = dev_restrict(core, B, rows, rev, s, guard)
            if got != want:
                k = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
                raise AssertionError("%s rev %d shift %d: sentence %d of %d differs: in %r got %r want %r" % (
                    what, rev, s, k, len(rows), rows[k][:12], got[k][:24], want[k][:24]))
        if props:
            check_props(core, B, R, allowed, rows, want, rev, what)


def split_ids(R, E, k=4):
    """ids that split, longest expansion first, and ids that stay"""
    by_len = sorted((v for v in E if len(E[v]) > 1), key=lambda v: -len(E[v]))
    stay = [v for v in E if len(E[v]) == 1]
    assert by_len and stay
    return by_len[:k], stay


# ---- case 1: the pass on synthetic ids ------------------------------------------------------------------------------------------------------------
def check_synthetic(B, shifts=(0, 1, 5, 15), name="readme_small"):
    core = D.core_of(name)
    V = core.vocab_size()
    R = Rules(model_path(name), V)
    rng = np.random.RandomState(21)
    for mname, allowed in R.masks().items():
        if mname == "all":
            continue
        E = R.table(allowed)
        info = core.set_vocabulary(allowed)
        assert info == R.info(allowed) == core.vocabulary_info(), (mname, info)
        (S, S2, S3, _), stay = split_ids(R, E)
        Kp = stay[-1]
        guard = S  # (a guard id that is read shows: it splits)
        args = dict(shifts=shifts if mname == "none" else shifts[:2], guard=guard)
        # no sentence, empty sentences, one id, the sizes around a step
        assert dev_restrict(core, B, [], 0, 1, guard) == [] and dev_restrict(core, B, [], 1, 0, guard) == []
        same(core, B, R, E, allowed, [[], [], []], (mname, "empty only"), splits=False, **args)
        same(core, B, R, E, allowed, [[], [], [S], [], []], (mname, "empty around one"), **args)
        for n in (1, 63, 64, 65):
            row = rng.randint(0, V, size=n).tolist()
            row[n // 2] = S
            same(core, B, R, E, allowed, [row], (mname, "n", n), **args)
        # the splitting id at lanes 0 and 63 of a step, and on both sides of a step's edge
        for at in ((0,), (63,), (0, 63), (63, 64), (64,), (127, 128)):
            row = [Kp] * 130
            for a in at:
                row[a] = S if a % 2 else S2
            same(core, B, R, E, allowed, [row], (mname, "lanes", at), props=False, **args)
        # sentence boundaries inside a step, next to expansions
        same(core, B, R, E, allowed, [[S, Kp, S2], [S], [Kp] * 58 + [S3], [S2], [S, S2] * 35, [], [Kp]], (mname, "boundaries in a step"), **args)
        # more than 63 boundaries in one step
        rows = [[S] if i % 3 == 0 else [] if i % 3 == 1 else [Kp] for i in range(400)]
        same(core, B, R, E, allowed, rows, (mname, "many boundaries"), **args)
        rows = [[S2, Kp][i % 2:] for i in range(300)]
        same(core, B, R, E, allowed, rows, (mname, "many short sentences"), props=False, **args)
        # ids out of range pass through and split nothing around them
        odd = [-1, I32_MIN, I32_MAX, V, V + 7, -77]
        same(core, B, R, E, allowed, [odd, [S] + odd + [S2], [o for x in odd for o in (x, S)], [V]], (mname, "out of range"), **args)
        # several groups and workgroups: many sentences of uneven length, and sentences long enough to be a group each
        rows = [rng.randint(0, V, size=n).tolist() for n in rng.randint(0, 40, size=1500)]
        same(core, B, R, E, allowed, rows, (mname, "many groups"), shifts=shifts[:1], guard=guard, props=(mname == "none"))
        rows = [rng.randint(-3, V + 3, size=n).tolist() for n in (300, 257, 1000, 256, 64, 700, 2, 513)]
        same(core, B, R, E, allowed, rows, (mname, "long sentences"), shifts=shifts[:1], guard=guard)
    # every id allowed: the identity, whatever the input
    core.set_vocabulary(R.masks()["all"])
    E = R.table(R.masks()["all"])
    rows = [rng.randint(-3, V + 3, size=n).tolist() for n in (0, 1, 64, 65, 300)]
    same(core, B, R, E, R.masks()["all"], rows, "all allowed", shifts=shifts[:2], splits=False)


# ---- case 2: expansions longer than the tile ------------------------------------------------------------------------------------------------------
def check_long(B, tmp_path, shifts=(0, 3)):
    """the model of decode_checks.check_long_pieces: one piece is a word of 2 300 chars, and the prefixes it was merged from have every length"""
    bpe, word, _ = SW.long_model(tmp_path)
    core = bpe.bpe_cython
    V = core.vocab_size()
    R = Rules(bpe.model, V)
    for mname in ("none", "lowest tenth"):  # (the second one: only the first tenth of the merges allowed, so that long expansions hold merged ids)
        allowed = R.masks()["none"] if mname == "none" else np.arange(V) < R.rules[len(R.rules) // 10][2]
        E = R.table(allowed)
        assert core.set_vocabulary(allowed) == R.info(allowed)
        whole = core.subword_to_id("▁" + word)
        if mname == "none":
            assert len(E[whole]) == 2301 and core.vocabulary_info()[2] == 2301
        by_len = {}
        for v in range(V):
            by_len.setdefault(len(E[v]), v)
        near = lambda n: by_len[min(by_len, key=lambda ln: (abs(ln - n), ln))]  # noqa: E731
        big = max(by_len)
        assert big > 2 * SEG
        W = by_len[big]
        stay = by_len[1]
        m20, m9, m500 = near(20), near(9), by_len[max(ln for ln in by_len if ln <= SEG)]
        m509 = m600 = by_len[min(ln for ln in by_len if ln > SEG)]  # (the shortest expansion that no segment holds)
        assert 64 * len(E[m20]) > SEG and 2 * len(E[m500]) > SEG
        cases = {
            "a step whose expansions exceed the tile": [[m20] * 64, [m9] * 200, [m20, stay, m9] * 50],
            "one expansion of a step longer than a segment": [[stay] * 10 + [m600] + [stay] * 80, [m9] * 30 + [m509] + [m9] * 40, [m500, m500, stay, m509]],
            "the longest alone": [[W]],
            "the longest behind a full tile": [[m9] * 56 + [stay] * 4 + [W], [m500] + [W], [stay] * 64 + [W] + [stay], [m20] * 63 + [W, W]],
            "the longest between short sentences": [[stay, stay], [W], [stay], [], [m9, W, stay], [stay]],
            "the longest on every wave": [[W] + [stay] * 300, [stay] * 300 + [W], [m20] * 300, [W, stay] * 3 + [stay] * 300] * 2,
        }
        for what, rows in cases.items():
            same(core, B, R, E, allowed, rows, (mname, what), shifts=shifts, guard=W, props=(what == "the longest between short sentences"))
    # the wired route: the long word through the encoder
    sents = [word + " xy", "ab " + word + " " + word, "", "xy"]
    plain = bpe.encode(sents)
    allowed = R.masks()["none"]
    core.set_vocabulary(allowed)
    got = bpe.encode(sents)
    assert got == want_rows(R.table(allowed), plain, 0) and got != plain
    assert bpe.decode(got) == bpe.decode(plain)
    assert bpe.encode(sents, reverse=True) == [r[::-1] for r in got]


# ---- case 3: the wired routes ---------------------------------------------------------------------------------------------------------------------
def encode_rows(core, B, raw, b, e, r, dropout=0.0):
    blob, off = K.pack(raw)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    n_ids, ms = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), len(raw), len(blob), max(map(len, raw)), bool(b), bool(e), bool(r), dropout)
    ids, o = K.take_encoded(core, B, len(raw), n_ids)
    return K.rows(ids, o), ms


def check_routes_model(B, name):
    """yttm_encode_device + both exits under every mask and flag set, with the word cache forced on and off; the counters; clearing"""
    plain, core = D.core_of(name), D.core_of(name)
    V = core.vocab_size()
    M = SP.model(name)
    R = Rules(model_path(name), V)
    raw = to_bytes(sentences_of(name))
    base = {f: encode_rows(plain, B, raw, *f)[0] for f in M.flags()}
    counts = np.bincount(np.array([t for r in base[M.flags()[0]] for t in r]), minlength=V)
    # the threshold: one above the count of the batch's rarest merged token, so that at least that token splits
    masks = R.masks(counts, min(int(counts[z]) for z in R.by_z if counts[z]) + 1)
    for mname, allowed in masks.items():
        E = R.table(allowed)
        assert core.set_vocabulary(allowed) == R.info(allowed)
        for f in M.flags():
            want = want_rows(E, base[f], f[2])
            assert (want != base[f]) == (mname != "all"), (name, mname, f, "the mask splits nothing of this batch")
            for cache in (2, 1, 0) if mname in ("none", "counts") else (2,):
                core.set_cache(cache)
                before = stats(core)
                got, ms = encode_rows(core, B, raw, *f)
                assert got == want, (name, mname, f, cache)
                assert ms >= 0
                moved = stats(core) - before
                n_in, n_out = sum(map(len, base[f])), sum(map(len, want))
                assert moved.tolist() == [1, 1 if mname == "all" else 0, n_in, n_out], (name, mname, f, moved)
            core.set_cache(2)
        if mname in ("none", "counts"):
            f = M.flags()[-1]
            check_props(core, B, R, allowed, base[f], want_rows(E, base[f], f[2]), f[2], (name, mname))
            blob, off = K.pack(raw)  # the host-to-host route
            ids, o = core.encode_packed(blob, off, bool(f[0]), bool(f[1]), bool(f[2]), 0.0)
            assert K.rows(ids, o) == want_rows(E, base[f], f[2])
    # clearing restores the unrestricted ids exactly, and counts no call
    assert core.set_vocabulary(None) == (0, 0, 0) == core.vocabulary_info()
    before = stats(core)
    for f in M.flags():
        assert encode_rows(core, B, raw, *f)[0] == base[f]
    assert (stats(core) - before).tolist() == [0, 0, 0, 0]


def check_dropout(B, name="readme_small"):
    """two fresh encoders under one pinned salt draw alike call by call: the restricted one's ids are the oracle's of the other's"""
    raw = to_bytes(sentences_of(name))
    with DC.env():
        a, b = D.core_of(name), D.core_of(name)
    R = Rules(model_path(name), a.vocab_size())
    allowed = R.masks()["none"]
    E = R.table(allowed)
    b.set_vocabulary(allowed)
    none = encode_rows(a, B, raw, 0, 0, 0)[0]
    assert encode_rows(b, B, raw, 0, 0, 0)[0] == want_rows(E, none, 0)
    for p in (0.1, 1.0):
        for f in ((0, 0, 0), (1, 1, 1)):
            rows = encode_rows(a, B, raw, *f, dropout=p)[0]
            want = want_rows(E, rows, f[2])
            assert encode_rows(b, B, raw, *f, dropout=p)[0] == want, (p, f)
            if p < 1:
                assert want != rows and rows != none
            else:  # (every merge dropped: chars only, nothing is left to split)
                assert want == rows


def check_python_routes(B, name="readme_small"):
    """BPE.encode(list) in both output types, set_vocabulary from counts, the spans and the SUBWORD text of restricted ids"""
    import youtokentome_amd as yttm
    plain, bpe = yttm.BPE(model_path(name)), yttm.BPE(model_path(name))
    V = bpe.vocab_size()
    R = Rules(model_path(name), V)
    sents = sentences_of(name)[:40] + ["", "ab Z cd", "é中 ab", " "]
    base = plain.encode(sents, bos=True)
    counts = np.zeros(V + 1, np.uint64)
    counts[:V] = np.bincount(np.array([t for r in base for t in r]), minlength=V)
    allowed = counts[:V] >= 4
    E = R.table(allowed)
    assert bpe.set_vocabulary(counts=counts, threshold=4) == R.info(allowed) == bpe.vocabulary_info()
    got = bpe.encode(sents, bos=True)
    assert got == want_rows(E, base, 0) and got != base
    assert bpe.encode(sents, bos=True, reverse=True) == want_rows(E, plain.encode(sents, bos=True, reverse=True), 1)
    assert bpe.decode(got) == plain.decode(base)
    pieces = bpe.encode(sents, output_type=yttm.OutputType.SUBWORD)
    ids = bpe.encode(sents)
    vocab, unk = bpe.vocab(), bpe.subword_to_id("<UNK>")
    for s, ps, row in zip(sents, pieces, ids):
        assert len(ps) == len(row) and all(p == vocab[t] for p, t in zip(ps, row) if t != unk), s
    assert bpe.vocabulary_stats()[0] >= 3
    assert bpe.set_vocabulary(allowed=allowed) == R.info(allowed)
    assert bpe.encode(sents, bos=True) == got
    # spans and SUBWORD text of the restricted ids: the siblings' own checkers, on an encoder with the vocabulary set
    M = SP.Model(name)
    M.bpe.set_vocabulary(allowed=R.masks()["none"])
    En = R.table(R.masks()["none"])
    for f in M.flags():
        id_rows, _ = SP.check_batch(M, B, sents, *f, what=("restricted spans", f))
        assert id_rows == want_rows(En, K.rows(*SP.host_ids(plain.bpe_cython, sents, *f)), f[2])
        _, rows = SW.same(M.core, B, [s for s in sents], *f, what=("restricted SUBWORD", f), fmt=(M.vocab, M.alphabet, M.unk))
        assert rows == id_rows
    assert bpe.set_vocabulary() == (0, 0, 0)
    assert bpe.encode(sents, bos=True) == base


def check_files(B, tmp_path, name="readme_small"):
    """encode_file in its id, id_text and SUBWORD forms at three piece sizes, and count_file: the oracle of the unrestricted file's ids"""
    import youtokentome_amd as yttm
    plain, bpe = yttm.BPE(model_path(name)), yttm.BPE(model_path(name))
    V = bpe.vocab_size()
    R = Rules(model_path(name), V)
    data = K.golden(name)[0]
    path = str(tmp_path / "in.txt")
    open(path, "wb").write(data)
    lines = [ln.decode() for ln in K.py_split(data)]
    alphabet, vocab, unk = SW.alphabet_of(model_path(name)), bpe.vocab(), bpe.subword_to_id("<UNK>")
    for mname in ("none", "odd"):
        allowed = R.masks()[mname]
        E = R.table(allowed)
        bpe.set_vocabulary(allowed)
        for b, e, r in ((0, 0, 0), (1, 1, 1)):
            ids, off = plain.encode_file(path, bos=b, eos=e, reverse=r)
            want = want_rows(E, K.rows(ids, off), r)
            assert want != K.rows(ids, off)
            flat = np.array([t for row in want for t in row], np.int64)
            for chunk in (None, max(len(data) // 8, 1), 1):
                g_ids, g_off = bpe.encode_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
                assert K.rows(g_ids, g_off) == want, (mname, b, e, r, chunk)
                out = str(tmp_path / "out.txt")
                nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, id_text=True)
                assert (nl, ni) == (len(want), len(flat))
                assert open(out, "rb").read() == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want), (mname, chunk, "id_text")
                nl, ni, _ = bpe.encode_file(path, out, bos=b, eos=e, reverse=r, chunk_bytes=chunk, output_type=yttm.OutputType.SUBWORD)
                assert (nl, ni) == (len(want), len(flat))
                assert open(out, "rb").read() == b"".join(SW.format_ids(s, row, vocab, alphabet, unk, r) for s, row in zip(lines, want)), (mname, chunk, "SUBWORD")
                counts = bpe.count_file(path, bos=b, eos=e, reverse=r, chunk_bytes=chunk)
                assert counts.tolist() == np.bincount(flat, minlength=V + 1).tolist(), (mname, chunk, "counts")


# ---- case 4: errors ---------------------------------------------------------------------------------------------------------------------------------
def check_errors(B, name="readme_small"):
    import pytest
    core = D.core_of(name)
    V = core.vocab_size()
    R = Rules(model_path(name), V)
    ids, off = B.put(np.array([5, 6, 7], np.int32)), B.put(np.array([0, 3], np.uint64))
    # the pass without a vocabulary: code 1, and what was pending stays
    n = D.encode_device(core, B, [b"ab cd", b"Z"], 0, 0, 0)
    pending = D.encode_fetch(core, 2, n)[0].tolist()
    assert raw_restrict(core, B.ptr(ids), B.ptr(off), 1, 3) == (1, NO_VOCAB, 0)
    assert D.encode_fetch(core, 2, n)[0].tolist() == pending and stats(core).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="no vocabulary is set"):
        core.restrict_ids_device_raw(B.ptr(ids), B.ptr(off), 1, 3)
    # a mask of another size: code 1, and no vocabulary is set by it
    L, err, info = _lib.load(), C.create_string_buffer(_lib.ERRLEN), (C.c_uint64 * 3)(9, 9, 9)
    for wrong in (V - 1, V + 1, 0):
        mask = np.ones(max(wrong, 1), np.uint8)
        rc = L.yttm_encoder_set_vocabulary(core._h, mask.ctypes.data_as(_lib.u8p), wrong, info, err, _lib.ERRLEN)
        assert rc == 1 and "n must be the vocabulary's size" in err.value.decode() and list(info) == [0, 0, 0], (wrong, err.value)
    assert raw_restrict(core, B.ptr(ids), B.ptr(off), 1, 3)[:2] == (1, NO_VOCAB)
    with pytest.raises(ValueError, match="vocabulary's size"):
        core.set_vocabulary(np.ones(V + 2, bool))
    # a vocabulary set while a result is pending does not change that result; the pass then replaces it and empties the spans slot
    sents = [b"ab Z cd", b"abcd " * 10]
    blob, soff = K.pack(sents)
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(soff)
    n_ids, _ = core.spans_device_raw(B.ptr(d_b), B.ptr(d_o), 2, len(blob), max(map(len, sents)))
    before = D.encode_fetch(core, 2, n_ids)[0].tolist()
    core.set_vocabulary(R.masks()["none"])
    assert D.encode_fetch(core, 2, n_ids)[0].tolist() == before
    assert core.fetch_spans(2, n_ids).shape == (n_ids, 2)
    assert raw_restrict(core, B.ptr(ids), B.ptr(off), 1, 3)[0] == 0
    with pytest.raises(ValueError, match="fetch_spans: no matching result"):
        core.fetch_spans(1, 3)
    assert raw_restrict(core, B.ptr(ids) + 2, B.ptr(off), 1, 3)[0] == 2  # a misaligned address


# ---- case 5: the command line -------------------------------------------------------------------------------------------------------------------------
def check_cli(tmp_path, name="readme_small"):
    """count_file -> a vocabulary file -> encode, encode_file and count_file under it; a vocabulary of another model.  Six processes."""
    import youtokentome_amd as yttm
    plain = yttm.BPE(model_path(name))
    V = plain.vocab_size()
    R = Rules(model_path(name), V)
    data = K.golden(name)[0]
    path, model_file, voc = str(tmp_path / "in.txt"), model_path(name), str(tmp_path / "voc.tsv")
    open(path, "wb").write(data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cli = [sys.executable, "-m", "youtokentome_amd.yttm_cli"]

    def run(args, stdin=None, ok=True):
        p = subprocess.run(cli + args, capture_output=True, env=env, input=stdin)
        assert (p.returncode == 0) == ok, p.stderr.decode()
        return p.stdout if ok else p.stderr

    assert run(["count_file", f"--model={model_file}", f"--input={path}", f"--output={voc}"]) == b""
    rows = [ln.split(b"\t") for ln in open(voc, "rb").read().split(b"\n")[:-1]]
    open(voc, "wb").write(b"".join(b"\t".join(r) + b"\n" for r in rows if int(r[0]) % 7 != 6))  # (ids missing from the file count 0)
    counts = np.array([0 if int(r[0]) % 7 == 6 else int(r[2]) for r in rows])
    allowed = counts >= 3
    E = R.table(allowed)
    ids, off = plain.encode_file(path)
    want = want_rows(E, K.rows(ids, off), 0)
    assert want != K.rows(ids, off)
    text = b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want)
    opts = [f"--vocabulary={voc}", "--vocabulary_threshold=3"]
    assert run(["encode", f"--model={model_file}", "--output_type=id"] + opts, stdin=data) == text
    out = str(tmp_path / "out.txt")
    run(["encode_file", f"--model={model_file}", f"--input={path}", f"--output={out}", "--output_type=id_text"] + opts)
    assert open(out, "rb").read() == text
    printed = run(["count_file", f"--model={model_file}", f"--input={path}"] + opts).split(b"\n")[:-1]
    flat = np.bincount(np.array([t for row in want for t in row]), minlength=V)
    assert [int(ln.split(b"\t")[2]) for ln in printed] == flat.tolist()
    # the default threshold is 1; a vocabulary written for another model is a plain error
    e1 = R.table(counts >= 1)
    got = run(["encode", f"--model={model_file}", "--output_type=id", f"--vocabulary={voc}"], stdin=data)
    assert got == b"".join(b"".join(b"%d " % t for t in row) + b"\n" for row in want_rows(e1, K.rows(ids, off), 0))
    other = model_path("manual_ru" if name != "manual_ru" else "readme_small")
    msg = run(["encode", f"--model={other}", "--output_type=id"] + opts, stdin=b"ab\n", ok=False).decode()
    assert "belongs to another model" in msg, msg


# ---- case 6: torch tensors (MI355X) -----------------------------------------------------------------------------------------------------------------
def check_tensor_api(name="readme_small"):
    import pytest
    import torch
    import youtokentome_amd as yttm
    plain, bpe = yttm.BPE(model_path(name)), yttm.BPE(model_path(name))
    V = bpe.vocab_size()
    R = Rules(model_path(name), V)
    dev = torch.device("cuda", bpe.bpe_cython.device)
    sents = sentences_of(name)[:50] + ["", "ab Z cd", "é中 ab", " "]
    p_ids, p_off = plain.encode_tensor(sents, bos=True, padded=False)
    base = K.rows(p_ids.cpu().numpy(), p_off.cpu().numpy())
    with pytest.raises(ValueError, match="no vocabulary is set"):
        bpe.restrict_tensor(p_ids, offsets=p_off)
    counts = plain.id_counts_tensor()
    allowed = counts[:V].cpu().numpy() >= 4
    E = R.table(allowed)
    assert bpe.set_vocabulary(counts=counts, threshold=4) == R.info(allowed)
    want = want_rows(E, base, 0)
    assert want != base
    ids, off = bpe.encode_tensor(sents, bos=True, padded=False)
    assert ids.dtype == torch.int32 and ids.device == dev and K.rows(ids.cpu().numpy(), off.cpu().numpy()) == want
    m, lengths = bpe.encode_tensor(sents, bos=True, pad_id=V + 5)
    assert m.shape[1] == max(map(len, want))
    for i, row in enumerate(want):
        assert m[i, :int(lengths[i])].tolist() == row and set(m[i, int(lengths[i]):].tolist()) <= {V + 5}
    # the counts of the pending restricted result
    assert bpe.id_counts_tensor().cpu().numpy().tolist() == np.bincount(np.array([t for r in want for t in r]), minlength=V + 1).tolist()
    # ids this object did not encode: ragged, padded with lengths, reversed; idempotent
    r_ids, r_off = bpe.restrict_tensor(p_ids, offsets=p_off)
    assert torch.equal(r_ids, ids) and torch.equal(r_off, off)
    r2, o2 = bpe.restrict_tensor(r_ids, offsets=r_off)
    assert torch.equal(r2, ids) and torch.equal(o2, off)
    pm, pl = plain.encode_tensor(sents, bos=True, pad_id=0)
    rm, rl = bpe.restrict_tensor(pm, lengths=pl, pad_id=V + 5)
    assert torch.equal(rm, m) and torch.equal(rl, lengths)
    rr, ro = bpe.restrict_tensor(p_ids, offsets=p_off, reverse=True)
    assert K.rows(rr.cpu().numpy(), ro.cpu().numpy()) == want_rows(E, base, 1)
    # spans of restricted ids through the property checker
    M = SP.model(name)
    s_ids, s_off, spans = bpe.encode_spans_tensor(sents, padded=False)
    rows, sp = K.rows(s_ids.cpu().numpy(), s_off.cpu().numpy()), SP.rows(spans.cpu().numpy(), s_off.cpu().numpy())
    assert rows == want_rows(E, K.rows(*[t.cpu().numpy() for t in plain.encode_tensor(sents, padded=False)]), 0)
    for raw, r_ids_, r_sp in zip(to_bytes(sents), rows, sp):
        SP.check_properties(M, raw, r_ids_, [tuple(p) for p in r_sp], 0, raw[:40])
    assert bpe.set_vocabulary() == (0, 0, 0)
    assert torch.equal(bpe.encode_tensor(sents, bos=True, padded=False)[0], p_ids)


# ---- case 7: one larger pass (MI355X) -----------------------------------------------------------------------------------------------------------------
def check_large(B, name="zipf", n=50_000, width=128):
    """50 000 x 128 chars through the text route, none-allowed and a threshold mask: both yardsticks as array comparisons"""
    import gen
    plain, core = D.core_of(name), D.core_of(name)
    V = core.vocab_size()
    R = Rules(model_path(name), V)
    raw = gen.zipf_corpus_fast(n * width + 4096, seed=29, vocab=20000).replace(b"\n", b" ")[:n * width]
    data = b"".join(raw[i * width:(i + 1) * width] + b"\n" for i in range(n))
    P = K.Placed(B, data, 9)
    nl, ni, _ = plain.encode_text_device_raw(P.ptr, len(data), True, True, False)
    ids, off = plain.fetch_encode(nl, ni)
    counts = np.bincount(ids, minlength=V)
    leaf = np.array([v not in R.by_z for v in range(V)])
    for mname, allowed in (("none", np.zeros(V, bool)), ("threshold", counts >= int(np.percentile(counts[counts > 0], 60)))):
        E = R.table(allowed)
        core.set_vocabulary(allowed)
        want, start = want_flat(E, V, ids, 0)
        assert len(want) > len(ids), (mname, "nothing splits")
        nl2, ni2, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
        got, g_off = core.fetch_encode(nl2, ni2)
        assert nl2 == nl and ni2 == len(want) and np.array_equal(got, want), mname
        assert np.array_equal(g_off.astype(np.int64), start[off.astype(np.int64)]), (mname, "offsets")
        assert bool((allowed[got] | leaf[got]).all()), (mname, "an id that should have split")
        # restricting again changes nothing, and skips nothing of the input
        d_ids, d_off = B.put(got), B.put(g_off)
        n3, _ = core.restrict_ids_device_raw(B.ptr(d_ids), B.ptr(d_off), nl, ni2)
        again, a_off = core.fetch_encode(nl, n3)
        assert n3 == ni2 and np.array_equal(again, got) and np.array_equal(a_off, g_off), (mname, "twice")
        # the same text from the device decode
        nb, _ = core.decode_device_raw(B.ptr(d_ids), B.ptr(d_off), nl, ni2, (2, 3))
        text_r = core.fetch_decode(nl, nb)
        p_ids, p_off = B.put(ids), B.put(off)
        nb2, _ = core.decode_device_raw(B.ptr(p_ids), B.ptr(p_off), nl, ni, (2, 3))
        text_p = core.fetch_decode(nl, nb2)
        assert nb == nb2 and np.array_equal(text_r[0], text_p[0]) and np.array_equal(text_r[1], text_p[1]), (mname, "decode")
    assert P.intact()
