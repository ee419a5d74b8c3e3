"""Checks of the device decode (yttm_decode_device[_padded], yttm_decode_fetch / _copy_device) and of the device-to-device exits of the encoder
(yttm_encode_copy_device / _padded), shared by the emulator tests (test_decode_device.py: numpy arrays are "device" memory there, the
emulator's hipMalloc is calloc) and the MI355X tests (test_gpu_decode.py: torch tensors).

The yardstick is the host path, yttm_decode (test_cli.py and test_reference_suite.py pin it to the reference); where the compiled reference
is present, its own decode of the same ids is a second one (empty ignore set: all its driver offers).  Equality is exact: bytes and offsets."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np

import gen
import refbin
from youtokentome_amd import _lib

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = (0, 1, 2, 63, 64, 65, 511, 512, 513, 5000)


# ---- "device" memory -----------------------------------------------------------------------------------------------------------------
class NumpyBuf:
    """emulator: host pointers are device pointers"""

    def put(self, arr):
        return np.ascontiguousarray(arr).copy()

    def empty(self, n, dtype):
        return np.full(max(int(n), 1), 0x5A, dtype=dtype) if np.dtype(dtype).itemsize == 1 else np.full(max(int(n), 1), -7, dtype=np.int64).astype(dtype)

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h, n=None):
        return h.copy() if n is None else h[:n].copy()


class TorchBuf:
    """MI355X: torch tensors on cuda:0 (uint64 travels as int64: same bytes)"""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.uint64:
            arr = arr.view(np.int64)
        t = self.torch.from_numpy(arr.copy()).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def empty(self, n, dtype):
        dt = np.dtype(dtype)
        t = self.torch.full((max(int(n), 1),), 0x5A if dt.itemsize == 1 else -7, dtype=getattr(self.torch, "int64" if dt == np.uint64 else str(dt)), device=self.dev)
        self.torch.cuda.synchronize()
        return t

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h, n=None):
        self.torch.cuda.synchronize()
        a = h.cpu().numpy()
        return a.copy() if n is None else a[:n].copy()


# ---- the two paths -------------------------------------------------------------------------------------------------------------------
def core_of(model):
    import youtokentome_amd as yttm
    return yttm.BPE(model if os.path.sep in model else os.path.join(G, f"train_{model}.model")).bpe_cython


def flatten(sents):
    off = np.zeros(len(sents) + 1, np.uint64)
    if sents:
        np.cumsum([len(s) for s in sents], out=off[1:])
    flat = np.ascontiguousarray([t for s in sents for t in s], dtype=np.int32)
    return flat, off


def _ign(ignore):
    a = np.ascontiguousarray(sorted(set(int(i) for i in ignore)), dtype=np.int32)
    return a, a.ctypes.data_as(_lib.i32p), len(a)


def host_decode(core, flat, off, ignore=()):
    """yttm_decode (the parent commit's path): (code, message, bytes, offsets)"""
    L = _lib.load()
    a, ap, an = _ign(ignore)
    blob_p, ooff, err = C.c_void_p(), _lib.u64p(), C.create_string_buffer(_lib.ERRLEN)
    flat = np.ascontiguousarray(flat, np.int32)
    off = np.ascontiguousarray(off, np.uint64)
    n = len(off) - 1
    rc = L.yttm_decode(core._h, flat.ctypes.data_as(_lib.i32p), off.ctypes.data_as(_lib.u64p), n, ap, an, C.byref(blob_p), C.byref(ooff), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None
    oo = np.ctypeslib.as_array(ooff, shape=(n + 1,)).astype(np.uint64, copy=True)
    raw = C.string_at(blob_p, int(oo[-1]))
    L.yttm_free(blob_p)
    L.yttm_free(C.cast(ooff, C.c_void_p))
    return 0, "", raw, oo


def _take_result(core, B, n, n_bytes):
    """the pending decode result by both exits, which must agree: (bytes, offsets)"""
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    raw, off = np.full(max(n_bytes, 1), 0x33, np.uint8), np.full(n + 1, 99, np.uint64)
    assert L.yttm_decode_fetch(core._h, C.c_void_p(raw.ctypes.data), off.ctypes.data_as(_lib.u64p), n, err, _lib.ERRLEN) == 0, err.value
    d_raw, d_off = B.empty(n_bytes + 3, np.uint8), B.empty(n + 1, np.uint64)
    assert L.yttm_decode_copy_device(core._h, C.c_void_p(B.ptr(d_raw)), C.c_void_p(B.ptr(d_off)), n, err, _lib.ERRLEN) == 0, err.value
    got_raw, got_off = B.get(d_raw), B.get(d_off, n + 1).view(np.uint64)
    assert got_off.tolist() == off.tolist()
    assert got_raw[:n_bytes].tobytes() == raw[:n_bytes].tobytes()
    assert got_raw[n_bytes:n_bytes + 3].tolist() == [0x5A] * 3, "the copy wrote past the text"
    assert int(off[-1]) == n_bytes
    return raw[:n_bytes].tobytes(), off


def dev_decode(core, B, flat, off, ignore=()):
    """yttm_decode_device on ids + offsets in device memory: (code, message, bytes, offsets)"""
    L = _lib.load()
    a, ap, an = _ign(ignore)
    n = len(off) - 1
    d_ids, d_off = B.put(np.ascontiguousarray(flat, np.int32)), B.put(np.ascontiguousarray(off, np.uint64))
    nb, ms, err = C.c_uint64(12345), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_decode_device(core._h, C.c_void_p(B.ptr(d_ids)), C.c_void_p(B.ptr(d_off)), n, len(flat), ap, an, C.byref(nb), C.byref(ms), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None
    raw, oo = _take_result(core, B, n, nb.value)
    return 0, "", raw, oo


def dev_decode_padded(core, B, matrix, width, stride, lengths=None, ignore=()):
    """yttm_decode_device_padded on a [n, stride] int32 array of which the first `width` columns count"""
    L = _lib.load()
    a, ap, an = _ign(ignore)
    n = matrix.shape[0]
    d_m = B.put(np.ascontiguousarray(matrix, np.int32).reshape(-1))
    d_l = B.put(np.ascontiguousarray(lengths, np.int32)) if lengths is not None else None
    nb, ms, err = C.c_uint64(), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_decode_device_padded(core._h, C.c_void_p(B.ptr(d_m)), n, width, stride, C.c_void_p(B.ptr(d_l)) if d_l is not None else None, ap, an,
                                     C.byref(nb), C.byref(ms), err, _lib.ERRLEN)
    if rc != 0:
        return rc, err.value.decode(), None, None
    raw, oo = _take_result(core, B, n, nb.value)
    return 0, "", raw, oo


def same(core, B, sents, ignore=(), what=""):
    """device == host on a list of id lists; returns the decoded strings"""
    flat, off = flatten(sents)
    want = host_decode(core, flat, off, ignore)
    got = dev_decode(core, B, flat, off, ignore)
    assert got[0] == want[0] and got[1] == want[1], (what, got[:2], want[:2])
    if want[0] == 0:
        assert got[3].tolist() == want[3].tolist(), what
        assert got[2] == want[2], what
        o = want[3].tolist()
        return [want[2][o[i]:o[i + 1]] for i in range(len(sents))]
    return None


def ref_decode(model_path, sents, tmp_path):
    """the compiled reference's decode of the same ids (empty ignore set), or None where it is not built"""
    if not refbin.available("prod") or tmp_path is None:
        return None
    ids_file, out_file = str(tmp_path / "ids.txt"), str(tmp_path / "dec.txt")
    open(ids_file, "w").write("".join(" ".join(str(t) for t in s) + "\n" for s in sents))
    r = subprocess.run([refbin.path("prod"), "decode", model_path, ids_file, out_file], capture_output=True)
    assert r.returncode == 0, r.stdout
    return open(out_file, "rb").read().split(b"\n")[:-1]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def golden_names():
    return sorted(n for n in (os.path.basename(p)[len("encode_"):-len(".lines")] for p in os.listdir(G) if p.startswith("encode_") and p.endswith(".lines"))
                  if os.path.exists(os.path.join(G, f"train_{n}.model")))


def model_args(name):
    return json.load(open(os.path.join(G, f"train_{name}.args.json")))


def golden_sentences(name):
    return open(os.path.join(G, f"encode_{name}.lines"), "rb").read().decode().split("\n")[:-1]


def check_golden(B, name, tmp_path=None):
    import youtokentome_amd as yttm
    a = model_args(name)
    model = os.path.join(G, f"train_{name}.model")
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    sents = golden_sentences(name)
    special = {k: a[k] for k in ("pad", "unk", "bos", "eos")}
    ignores = [(), (special["bos"], special["eos"]), (special["unk"],), tuple(special.values())]
    ignores = [tuple(i for i in ig if i != -1) for ig in ignores]
    flags = [(b, e, r) for b in (0, 1) for e in (0, 1) for r in (0, 1) if (not b or a["bos"] != -1) and (not e or a["eos"] != -1)]
    for b, e, r in flags:
        ids = bpe.encode(sents, yttm.OutputType.ID, bos=bool(b), eos=bool(e), reverse=bool(r))
        for ig in ignores:
            out = same(core, B, ids, ig, (name, b, e, r, ig))
            if name == "nopad":  # special ids of -1: nothing decodes to their names
                assert not any(t in s for s in out for t in (b"<PAD>", b"<BOS>", b"<EOS>"))
        ref = ref_decode(model, ids, tmp_path)
        if ref is not None and not any("\n" in s for s in sents):
            assert same(core, B, ids, (), name) == ref, (name, b, e, r)


def random_batches(vocab, seed=5, many=20000):
    rng = np.random.RandomState(seed)
    lens = list(LENGTHS) * 2
    random.Random(seed).shuffle(lens)
    yield [rng.randint(0, vocab, size=n).tolist() for n in lens]
    yield [rng.randint(0, vocab, size=n).tolist() for n in rng.randint(0, 41, size=many)]


def check_random(B, name="readme_small", many=20000, ignores=((), (0, 1, 2, 3), (1, 7, 8, 9, 10, 11, 12))):
    """ids no encoder would emit: space pieces in the middle, specials anywhere, runs of <UNK>"""
    core = core_of(name)
    vocab = core.vocab_size()
    for batch in random_batches(vocab, many=many):
        for ig in ignores:
            same(core, B, batch, ig, (name, len(batch), ig))
    same(core, B, [[1] * 300, [1, 1, 2, 3, 0] * 40, []], (), "runs of specials")


def space_pieces(core):
    """(id of the bare space piece, an id whose piece starts with the space sign and goes on, an id without it)"""
    bare = core.subword_to_id("▁")
    with_space = plain = None
    for i in range(core.vocab_size()):
        s = core.id_to_subword(i)
        if s.startswith("▁") and len(s) > 1 and with_space is None:
            with_space = i
        if not s.startswith("▁") and not s.startswith("<") and plain is None:
            plain = i
    assert core.id_to_subword(bare) == "▁" and with_space is not None and plain is not None
    return bare, with_space, plain


def check_strip_rule(B, name="readme_small"):
    core = core_of(name)
    bare, ws, plain = space_pieces(core)
    text = core.id_to_subword(ws)[1:].encode()
    ptext = core.id_to_subword(plain).encode()
    out = same(core, B, [[2, ws, plain], [bare, plain], [2, 3, 2], [ws, ws, bare, ws], [plain, ws], [bare], [2, bare, ws]], (2, 3), "strip")
    assert out[0] == text + ptext            # first id ignored, the second one a space piece: still stripped
    assert out[1] == ptext                   # the bare space piece first: the empty prefix
    assert out[2] == b""                     # ignored ids only
    assert out[3] == text + b" " + text + b" " + b" " + text  # later space pieces keep their space
    assert out[4] == ptext + b" " + text
    assert out[5] == b"" and out[6] == b" " + text
    # without the ignore set the special's name is the first piece, and nothing is stripped behind it
    out = same(core, B, [[2, ws, plain]], (), "strip, nothing ignored")
    assert out[0] == b"<BOS> " + text + ptext
    # many sentences a group, every one starting with a space piece (the first-kept mask across sentence boundaries), some empty
    rng = random.Random(3)
    batch = [([rng.choice([2, 3])] * rng.randint(0, 3) + [rng.choice([ws, bare, plain]) for _ in range(rng.randint(0, 5))]) for _ in range(700)]
    same(core, B, batch, (2, 3), "strip, many short")
    same(core, B, [[]] * 200 + [[ws]] + [[]] * 131 + [[2], [ws, ws]], (2,), "empty sentences around")


def check_errors(B, name="readme_small"):
    core = core_of(name)
    V = core.vocab_size()
    good = [[5, 6, 7], [8, 9], [10] * 70]
    want_good = same(core, B, good, (), "good")
    for bad_id in (-1, V, 2 ** 31 - 1, -2 ** 31):
        flat, off = flatten([[5, 6], [7, bad_id, 8], [9]])
        rc, msg, _, _ = dev_decode(core, B, flat, off, ())
        assert rc == 1 and msg == "id must be in the range [0, vocab_size - 1]. Current value: vocab_size = %d; id=%d;" % (V, bad_id), msg
        assert (rc, msg) == host_decode(core, flat, off, ())[:2]
        # no result is pending after a failure ...
        err = C.create_string_buffer(_lib.ERRLEN)
        assert _lib.load().yttm_decode_fetch(core._h, None, None, 3, err, _lib.ERRLEN) != 0
        # ... and the next good call does not depend on it
        assert same(core, B, good, (), "good after bad") == want_good
    # several bad ids in different sentences: the first in sentence order, then position order, is named -- whichever workgroup saw which
    rng = random.Random(9)
    batch = [[rng.randrange(V) for _ in range(rng.randint(0, 90))] for _ in range(400)]
    for s, p, v in ((399, 0, V + 5), (250, 3, -9), (120, 40, V + 1), (120, 17, V + 2), (333, 1, -1)):
        while len(batch[s]) <= p:
            batch[s].append(4)
        batch[s][p] = v
    flat, off = flatten(batch)
    rc, msg, _, _ = dev_decode(core, B, flat, off, ())
    assert rc == 1 and msg.endswith("id=%d;" % (V + 2)), msg
    assert (rc, msg) == host_decode(core, flat, off, ())[:2]
    # a bad id that is ignored is no error: the ignore set is asked before the range check
    same(core, B, batch, (V + 2,), "first bad id ignored")
    rc, msg, _, _ = dev_decode(core, B, flat, off, (V + 2,))
    assert rc == 1 and msg.endswith("id=%d;" % (V + 1)), msg
    out = same(core, B, batch, (V + 5, -9, V + 1, V + 2, -1, 2 ** 31 - 1), "all bad ids ignored")
    assert out is not None
    same(core, B, [[-1, 5, 2 ** 31 - 1, 6]], (-1, 2 ** 31 - 1), "ignored ids outside the vocabulary")


def check_long_pieces(B, tmp_path):
    """a model in which one piece is a word of several thousand chars: the write kernel's piece-by-piece path"""
    import youtokentome_amd as yttm
    rng = random.Random(4)
    word = "".join(rng.choice("abcdefgh") for _ in range(2300))
    corpus, model = str(tmp_path / "long.txt"), str(tmp_path / "long.model")
    open(corpus, "w").write((word + " xy ") * 6 + "ab cd\n")
    yttm.BPE.train(corpus, model, 4 + 11 + 2400, 1.0, 1, 0, 1, 2, 3)
    bpe = yttm.BPE(model)
    core = bpe.bpe_cython
    whole = core.subword_to_id("▁" + word)
    assert core.id_to_subword(whole) == "▁" + word, "the long word did not become one piece"
    longest = sorted(range(core.vocab_size()), key=lambda i: -len(core.id_to_subword(i)))[:40]
    out = same(core, B, [[whole], [5, whole, whole, 6], longest, [whole] * 3 + longest[::-1] + [7], [], [whole, 8]], (), "long pieces")
    assert out[0] == word.encode() and out[1].count(word.encode()) == 2
    same(core, B, [[2, whole, 3]] * 9, (2, 3), "long pieces, strip")
    sents = [word + " xy", "ab " + word + " " + word]
    assert [s.decode() for s in same(core, B, bpe.encode(sents), (), "long round trip")] == sents


def to_padded(sents, width, stride, pad):
    m = np.full((len(sents), stride), pad, np.int32)
    for i, s in enumerate(sents):
        m[i, :len(s)] = s
    if stride > width:
        m[:, width:] = 0x7FFFFFF0  # never read: an id that would be an error
    return m, np.array([len(s) for s in sents], np.int32)


def check_padded(B, name="readme_small"):
    import youtokentome_amd as yttm
    bpe = yttm.BPE(os.path.join(G, f"train_{name}.model"))
    core = bpe.bpe_cython
    V = core.vocab_size()
    rng = np.random.RandomState(8)
    real = bpe.encode(golden_sentences(name), yttm.OutputType.ID, bos=True, eos=True)
    batches = [real, [rng.randint(4, V, size=n).tolist() for n in (0, 1, 2, 63, 64, 65, 200, 0, 5)], [rng.randint(4, V, size=n).tolist() for n in rng.randint(0, 9, size=300)],
               [[], [], []], [[5]]]
    for sents in batches:
        flat, off = flatten(sents)
        longest = max(len(s) for s in sents)
        for ignore in ((), (2, 3)):
            want = dev_decode(core, B, flat, off, ignore)
            assert want[0] == 0 and want[2:] is not None
            assert (want[2], want[3].tolist()) == (lambda h: (h[2], h[3].tolist()))(host_decode(core, flat, off, ignore))
            for width, stride in ((longest, longest), (longest + 3, longest + 3), (longest, longest + 5), (longest + 1, longest + 70)):
                m, lens = to_padded(sents, width, stride, 0)
                got = dev_decode_padded(core, B, m, width, stride, lens, ignore)
                assert got[0] == 0 and got[2] == want[2] and got[3].tolist() == want[3].tolist(), (width, stride, "lengths")
                # without lengths: the pad id is removed by ignoring it (real ids here are >= 2)
                got = dev_decode_padded(core, B, m, width, stride, None, tuple(ignore) + (0,))
                assert got[0] == 0 and got[2] == want[2] and got[3].tolist() == want[3].tolist(), (width, stride, "no lengths")
    # an invalid id behind a row's length is not read; inside it is the error, named like the ragged call names it
    m, lens = to_padded([[5, 6, 7], [8, 9]], 4, 6, V + 9)
    assert dev_decode_padded(core, B, m, 4, 6, lens, ())[0] == 0
    rc, msg, _, _ = dev_decode_padded(core, B, m, 4, 6, None, ())
    assert rc == 1 and msg == host_decode(core, *flatten([[V + 9]]))[1]


def encode_device(core, B, sents_bytes, bos=0, eos=0, reverse=0):
    L = _lib.load()
    blob = b"".join(sents_bytes)
    off = np.zeros(len(sents_bytes) + 1, np.uint64)
    if sents_bytes:
        np.cumsum([len(s) for s in sents_bytes], out=off[1:])
    d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
    n_ids, ms, err = C.c_uint64(), C.c_double(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_encode_device(core._h, C.c_void_p(B.ptr(d_b)), C.c_void_p(B.ptr(d_o)), len(sents_bytes), len(blob), max([len(s) for s in sents_bytes] + [0]),
                              bos, eos, reverse, 0.0, C.byref(n_ids), C.byref(ms), err, _lib.ERRLEN)
    assert rc == 0, err.value
    return n_ids.value


def encode_fetch(core, n, n_ids):
    ids, off, err = np.zeros(max(n_ids, 1), np.int32), np.zeros(n + 1, np.uint64), C.create_string_buffer(_lib.ERRLEN)
    assert _lib.load().yttm_encode_fetch(core._h, ids.ctypes.data_as(_lib.i32p), off.ctypes.data_as(_lib.u64p), n, err, _lib.ERRLEN) == 0, err.value
    return ids[:n_ids], off


def check_encode_copies(B, name="readme_small"):
    core = core_of(name)
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    rng = random.Random(12)
    sents = [s.encode() for s in golden_sentences(name)] + [b"", b"abcd " * 300, b" "] + [("".join(rng.choice("abcd ") for _ in range(rng.randint(0, 40)))).encode() for _ in range(150)]
    n = len(sents)
    n_ids = encode_device(core, B, sents, 1, 1, 0)
    ids, off = encode_fetch(core, n, n_ids)
    lens = np.diff(off.astype(np.int64))
    longest = int(lens.max())
    # ragged, device to device
    d_ids, d_off = B.empty(n_ids + 2, np.int32), B.empty(n + 1, np.uint64)
    assert L.yttm_encode_copy_device(core._h, C.c_void_p(B.ptr(d_ids)), C.c_void_p(B.ptr(d_off)), n, err, _lib.ERRLEN) == 0, err.value
    assert B.get(d_ids)[:n_ids].tolist() == ids.tolist() and B.get(d_ids)[n_ids:n_ids + 2].tolist() == [-7, -7]
    assert B.get(d_off, n + 1).astype(np.uint64).tolist() == off.tolist()
    # a decode in between leaves the encode result where it is, and its own result survives the copies and a later encode
    dec_sents = [ids[int(off[i]):int(off[i + 1])].tolist() for i in range(n)]
    flat, o2 = flatten(dec_sents)
    want_dec = host_decode(core, flat, o2, (2, 3))
    d_f, d_o = B.put(flat), B.put(o2)
    a, ap, an = _ign((2, 3))
    nb, ms = C.c_uint64(), C.c_double()
    assert L.yttm_decode_device(core._h, C.c_void_p(B.ptr(d_f)), C.c_void_p(B.ptr(d_o)), n, len(flat), ap, an, C.byref(nb), C.byref(ms), err, _lib.ERRLEN) == 0, err.value
    for pad in (0, -100):
        for width in (longest, longest + 1, longest + 6):
            for shift in (0, 1, 2, 3):  # the matrix at every alignment: the 16-byte stores begin at its first boundary
                d_m, d_l = B.empty(n * width + 8, np.int32), B.empty(n, np.int32)
                need = C.c_uint64()
                rc = L.yttm_encode_copy_padded(core._h, C.c_void_p(B.ptr(d_m) + 4 * shift), C.c_void_p(B.ptr(d_l)), n, width, pad, C.byref(need), err, _lib.ERRLEN)
                assert rc == 0 and need.value == longest, err.value
                want = np.full((n, width), pad, np.int32)
                for i in range(n):
                    want[i, :lens[i]] = ids[int(off[i]):int(off[i + 1])]
                got = B.get(d_m)
                assert got[shift:shift + n * width].tolist() == want.reshape(-1).tolist(), (pad, width, shift)
                assert got[:shift].tolist() == [-7] * shift and got[shift + n * width:].tolist() == [-7] * (8 - shift), "stores outside the matrix"
                assert B.get(d_l, n).tolist() == lens.tolist()
    # too narrow: an error that names the width needed, and nothing is written
    d_m, d_l = B.empty(n * longest, np.int32), B.empty(n, np.int32)
    need = C.c_uint64()
    rc = L.yttm_encode_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), C.c_void_p(B.ptr(d_l)), n, longest - 1, 0, C.byref(need), err, _lib.ERRLEN)
    assert rc == 1 and need.value == longest and b"longest" in err.value
    assert set(B.get(d_m).tolist()) == {-7} and set(B.get(d_l).tolist()) == {-7}
    assert L.yttm_encode_copy_padded(core._h, C.c_void_p(B.ptr(d_m)), C.c_void_p(B.ptr(d_l)), n + 1, longest, 0, C.byref(need), err, _lib.ERRLEN) != 0
    # the decode result made before the copies is still there
    raw, oo = _take_result(core, B, n, nb.value)
    assert raw == want_dec[2] and oo.tolist() == want_dec[3].tolist()
    # ... after another encode as well, whose own result a decode does not disturb
    n_ids2 = encode_device(core, B, sents[:7], 0, 0, 1)
    raw, oo = _take_result(core, B, n, nb.value)
    assert raw == want_dec[2]
    ids2, off2 = encode_fetch(core, 7, n_ids2)
    dev_decode(core, B, flat[:50], np.array([0, 20, 50], np.uint64), ())
    ids3, off3 = encode_fetch(core, 7, n_ids2)
    assert ids2.tolist() == ids3.tolist() and off2.tolist() == off3.tolist()


def check_empty_batch(B, name="readme_small"):
    core = core_of(name)
    L = _lib.load()
    err = C.create_string_buffer(_lib.ERRLEN)
    rc, msg, raw, oo = dev_decode(core, B, np.zeros(0, np.int32), np.zeros(1, np.uint64), (1, 2))
    assert rc == 0 and raw == b"" and oo.tolist() == [0]
    nb, ms = C.c_uint64(5), C.c_double()
    assert L.yttm_decode_device(core._h, None, None, 0, 0, None, 0, C.byref(nb), C.byref(ms), err, _lib.ERRLEN) == 0 and nb.value == 0
    assert L.yttm_decode_device_padded(core._h, None, 0, 7, 9, None, None, 0, C.byref(nb), C.byref(ms), err, _lib.ERRLEN) == 0 and nb.value == 0
    off = np.full(1, 9, np.uint64)
    assert L.yttm_decode_fetch(core._h, None, off.ctypes.data_as(_lib.u64p), 0, err, _lib.ERRLEN) == 0 and off[0] == 0
    d_off = B.empty(1, np.uint64)
    assert L.yttm_decode_copy_device(core._h, None, C.c_void_p(B.ptr(d_off)), 0, err, _lib.ERRLEN) == 0 and int(B.get(d_off)[0]) == 0
    assert encode_device(core, B, [], 0, 0, 0) == 0
    d_off = B.empty(1, np.uint64)
    assert L.yttm_encode_copy_device(core._h, None, C.c_void_p(B.ptr(d_off)), 0, err, _lib.ERRLEN) == 0 and int(B.get(d_off)[0]) == 0
    need = C.c_uint64(3)
    assert L.yttm_encode_copy_padded(core._h, None, None, 0, 0, 0, C.byref(need), err, _lib.ERRLEN) == 0 and need.value == 0
    # a padded matrix without columns: rows without ids
    rc, msg, raw, oo = dev_decode_padded(core, B, np.zeros((4, 0), np.int32), 0, 0, None, ())
    assert rc == 0 and raw == b"" and oo.tolist() == [0] * 5


def check_round_trip(B):
    """coverage 1: decode_device(encode_device(s)) == " ".join(s.split()) for sentences without unknown chars"""
    done = 0
    for name in golden_names():
        a = model_args(name)
        if a["coverage"] != 1.0:
            continue
        core = core_of(name)
        alphabet = set(open(os.path.join(G, f"train_{name}.txt"), "rb").read().decode(errors="replace"))
        sents = [s for s in golden_sentences(name) if set(s) <= alphabet | set(" \t\n▁") and "▁" not in s]
        if not sents:
            continue
        raw = [s.encode() for s in sents]
        n_ids = encode_device(core, B, raw)
        ids, off = encode_fetch(core, len(raw), n_ids)
        assert a["unk"] not in ids.tolist(), name
        rc, msg, text, oo = dev_decode(core, B, ids, off, ())
        assert rc == 0
        o = oo.tolist()
        assert [text[o[i]:o[i + 1]].decode() for i in range(len(raw))] == [" ".join(s.split()) for s in sents], name
        done += len(sents)
    assert done > 20
