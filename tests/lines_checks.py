"""Checks of the line split on the device (yttm_lines_device, yttm_lines_fetch / _copy_device), of the encoder's entries for text that is not cut
into sentences (yttm_encode_text_device, yttm_encode_file) and of the `encode_file` command, shared by the emulator tests (test_lines_device.py:
numpy arrays are "device" memory there) and the MI355X tests (test_gpu_lines.py: torch tensors).

Two yardsticks, both older than the code under test:
  1. yttm_encode_as_ids on the same text cut by a plain Python restatement of std::getline's rules (py_split): the existing suite pins that
     path to the reference.  The sentences it gets are the lines WITHOUT their newline.
  2. the golden pairs tests/golden/encode_*.lines / .json, which the reference made.
Equality is exact everywhere: offsets, ids, n_lines, longest."""
import json
import os
import subprocess
import sys

import numpy as np

from decode_checks import G, NumpyBuf, TorchBuf, core_of, golden_names, model_args  # noqa: F401  (the buffers are re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384  # bytes a workgroup takes at a time (k_lines.h LN_TILE); a wave's share of one load is 1024, a lane's 16
GUARD = 48


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------------
def py_split(data):
    """std::getline: a line ends at 0x0A; a last line without one counts; nothing follows a final newline"""
    parts = bytes(data).split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return parts


def py_offsets(data):
    """the packed convention: line i = data[off[i]:off[i + 1]] with its newline"""
    off = [0]
    for p in py_split(data):
        off.append(min(off[-1] + len(p) + 1, len(data)))
    assert off[-1] == len(data) or not data
    return np.array(off, np.uint64)


def pack(lines):
    off = np.zeros(len(lines) + 1, np.uint64)
    if lines:
        np.cumsum([len(s) for s in lines], out=off[1:])
    return b"".join(lines), off


def host_encode(core, data, bos=0, eos=0, rev=0, dropout=0.0):
    """yardstick 1: (ids, offsets) of the existing host path on the lines without their newlines"""
    blob, off = pack(py_split(data))
    return core.encode_packed(blob, off, bool(bos), bool(eos), bool(rev), dropout)


# ---- text in "device" memory, at a chosen alignment, between guard bytes ------------------------------------------------------------------
class Placed:
    """data at an address = align (mod 16) inside a larger buffer; the bytes around it are newlines, so a read outside the text shows up
    as a wrong count, and must be untouched afterwards"""

    def __init__(self, B, data, align=0):
        self.B, self.n = B, len(data)
        host = np.full(GUARD + 16 + self.n + GUARD, 0x0A, np.uint8)
        self.buf = B.put(host)
        self.start = GUARD + (align - (B.ptr(self.buf) + GUARD)) % 16
        host[self.start:self.start + self.n] = np.frombuffer(bytes(data), np.uint8)
        self.host = host
        self._rewrite(host)
        assert (self.ptr % 16) == align

    def _rewrite(self, host):
        buf = self.buf
        if isinstance(buf, np.ndarray):
            buf[:] = host
        else:
            buf.copy_(self.B.torch.from_numpy(host.copy()))
            self.B.torch.cuda.synchronize()
        return buf

    @property
    def ptr(self):
        return self.B.ptr(self.buf) + self.start

    def intact(self):
        return self.B.get(self.buf).tobytes() == self.host.tobytes()


def dev_lines(core, B, data, align=0):
    """yttm_lines_device + both exits, which must agree: (offsets, longest)"""
    P = Placed(B, data, align)
    n_lines, longest, _ = core.lines_device_raw(P.ptr, len(data))
    off = core.fetch_lines(n_lines)
    d_off = B.empty(n_lines + 3, np.uint64)
    core.copy_lines_device(B.ptr(d_off), n_lines)
    got = B.get(d_off).view(np.uint64)
    assert got[:n_lines + 1].tolist() == off.tolist(), "the two exits differ"
    assert got[n_lines + 1:n_lines + 3].view(np.int64).tolist() == [-7, -7], "the copy wrote past the offsets"
    assert P.intact(), "the text or its guard bytes were written"
    return off, longest


def check_split_one(core, B, data, aligns=range(16)):
    want = py_offsets(data)
    want_longest = int(np.diff(want.astype(np.int64)).max()) if len(want) > 1 else 0
    for a in aligns:
        off, longest = dev_lines(core, B, data, a)
        assert len(off) == len(want), (len(data), a, len(off) - 1, len(want) - 1)
        assert off.tolist() == want.tolist(), (len(data), a)
        assert longest == want_longest, (len(data), a, longest, want_longest)


def split_texts():
    rng = np.random.RandomState(3)

    def rand(n, p_nl=0.05):
        a = rng.randint(32, 127, size=n).astype(np.uint8)
        a[rng.rand(n) < p_nl] = 10
        return a.tobytes()

    out = [b"", b"\n", b"\n\n\n\n\n", b"\n" * 4097, b"no newline at all", b"a\nbb\nccc\n", b"a\nbb\nccc", b"x", b"x\n", b"\nx", b"one\r\ntwo\r\n\r\nthree\r",
           b"nul\x00s\x00\n\x00\n\x00\x00", b"\x0b\x0c\x09 \n\x0a"]
    for n in (15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1):
        out.append(rand(n))
        out.append(rand(n)[:-1] + b"\n")          # a newline in the last byte starts no line
        out.append(b"\n" + rand(n, 0.0)[1:])      # a newline in the first byte does
        out.append(rand(n, 0.0)[:-2] + b"\n" + b"z")  # ... and one in the last but one
    return out


def check_split_cases(core, B, aligns=range(16)):
    for data in split_texts():
        check_split_one(core, B, data, aligns)


def check_split_large(core, B, aligns=range(16), big=3 * (1 << 20) + 12345):
    """one line of several MB across many workgroups (also as the last line, without a newline), and 10^5 one-byte lines"""
    line = (b"abcdefghij" * (big // 10 + 1))[:big]
    check_split_one(core, B, b"head\n" + line + b"\ntail", aligns)
    check_split_one(core, B, b"x\n" * 100000, aligns)
    check_split_one(core, B, b"first\n" + line, (0, 7))


# ---- encode ----------------------------------------------------------------------------------------------------------------------------
def take_encoded(core, B, n, n_ids):
    """the pending encode result by both exits, which must agree: (ids, offsets)"""
    ids, off = core.fetch_encode(n, n_ids)
    d_ids, d_off = B.empty(n_ids + 2, np.int32), B.empty(n + 1, np.uint64)
    core.copy_encode_device(B.ptr(d_ids), B.ptr(d_off), n)
    assert B.get(d_ids)[:n_ids].tolist() == ids.tolist() and B.get(d_ids)[n_ids:n_ids + 2].tolist() == [-7, -7]
    assert B.get(d_off, n + 1).astype(np.uint64).tolist() == off.tolist()
    assert int(off[-1]) == n_ids
    return ids, off


def dev_encode_text(core, B, data, bos=0, eos=0, rev=0, dropout=0.0, align=0):
    P = Placed(B, data, align)
    n, n_ids, _ = core.encode_text_device_raw(P.ptr, len(data), bool(bos), bool(eos), bool(rev), dropout)
    assert n == len(py_split(data))
    ids, off = take_encoded(core, B, n, n_ids)
    assert core.fetch_lines(n).tolist() == py_offsets(data).tolist()  # the lines' offsets are pending too
    assert P.intact()
    return ids, off


def rows(ids, off):
    o = [int(x) for x in off]
    flat = ids.tolist()
    return [flat[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def golden(name):
    data = open(os.path.join(G, f"encode_{name}.lines"), "rb").read()
    want = json.load(open(os.path.join(G, f"encode_{name}.json")))
    return data, {k: v for k, v in want.items() if len(k) == 3}  # "bos eos reverse" -> ids per line


def check_golden(B, name):
    """yardstick 2, and yardstick 1 beside it: the .lines file as one text, every flag combination the golden covers"""
    core = core_of(name)
    data, want = golden(name)
    assert len(want) >= 4 or model_args(name)["bos"] == -1
    for key, ids_want in sorted(want.items()):
        b, e, r = (int(c) for c in key)
        for cache in (0, 1):
            core.set_cache(cache)
            ids, off = dev_encode_text(core, B, data, b, e, r, align=(3 if cache else 0))
            assert rows(ids, off) == ids_want, (name, key, cache)
            h_ids, h_off = host_encode(core, data, b, e, r)
            assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist(), (name, key, cache)


ODD_TEXTS = [
    b"ab\xc3\ncd\xe2\x82\nef\xf0\x9f\x98\ngh\xe2\nij\xf0\nkl\xf0\x9f\nmn",   # truncated 2-, 3- and 4-byte heads before a newline
    b"tail cut in a char \xd0\xb0\xd0",                                      # ... and at the end of the text
    b"tail cut \xe2\x82", b"tail cut \xf0\x9f\x98", b"\xff\n\xfe\xff\n\x80\n\xbf\xbf\n",
    b"\xd0\xb0\xd0\xb1 \xd0\xb2\n\xe2\x96\x81x\n",                           # valid two- and three-byte chars, the space token itself
    b"\n\n\nab cd\n\n \n\t\nef\n\n",                                         # empty and blank lines
    b"one\r\ntwo\r\n\r\nthree\r", b"nul\x00s in\x00 a line\n\x00\n", b"", b"\n", b"a", b"a\n",
    b"abcd " * 300 + b"\n" + b"dcba" * 200 + b"\n" + b"a b " * 40,          # lines beyond the encoder's LDS size
]


def check_odd_texts(B, names=("readme_small", "manual_ru", "mix_cov")):
    for name in names:
        core = core_of(name)
        a = model_args(name)
        flags = [(0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)] if a["bos"] != -1 and a["eos"] != -1 else [(0, 0, 0), (0, 0, 1)]
        for cache in (0, 1):
            core.set_cache(cache)
            for i, data in enumerate(ODD_TEXTS):
                for b, e, r in flags:
                    ids, off = dev_encode_text(core, B, data, b, e, r, align=(i + cache) % 16)
                    h_ids, h_off = host_encode(core, data, b, e, r)
                    assert off.tolist() == h_off.tolist() and ids.tolist() == h_ids.tolist(), (name, cache, i, b, e, r)
    # empty lines with bos + eos are sentences of exactly those two ids
    core = core_of("readme_small")
    ids, off = dev_encode_text(core, B, b"\n\n\n", 1, 1, 0)
    a = model_args("readme_small")
    assert rows(ids, off) == [[a["bos"], a["eos"]]] * 3


def check_errors(B):
    import pytest
    core = core_of("nopad")  # trained without <BOS> / <EOS>
    P = Placed(B, b"ab\ncd\n")
    for b, e, word in ((1, 0, "<BOS>"), (0, 1, "<EOS>")):
        with pytest.raises(ValueError, match="Can't add %s token. Model was trained without it." % word):
            core.encode_text_device_raw(P.ptr, P.n, bool(b), bool(e))
    with pytest.raises(ValueError, match="no matching result"):
        core.lines_device_raw(P.ptr, P.n)
        core.fetch_lines(7)


def check_padded_and_round_trip(B, name="readme_small"):
    """the pending result through yttm_encode_copy_padded, and back to text through yttm_decode_device"""
    core = core_of(name)
    a = model_args(name)
    data, _ = golden(name)
    data += b"\n\nlast line without a newline"
    lines = py_split(data)
    P = Placed(B, data, 5)
    n, n_ids, _ = core.encode_text_device_raw(P.ptr, len(data), True, True, False)
    ids, off = take_encoded(core, B, n, n_ids)
    want = rows(ids, off)
    longest = max(len(r) for r in want)
    assert core.encode_longest(n) == longest
    width = longest + 3
    d_m, d_l = B.empty(n * width, np.int32), B.empty(n, np.int32)
    assert core.copy_encode_padded(B.ptr(d_m), B.ptr(d_l), n, width, -100) == longest
    m, l = B.get(d_m, n * width).reshape(n, width), B.get(d_l, n)
    assert l.tolist() == [len(r) for r in want]
    for i, r in enumerate(want):
        assert m[i, :len(r)].tolist() == r and m[i, len(r):].tolist() == [-100] * (width - len(r))
    # a split in between leaves the encode result where it is
    Q = Placed(B, b"x\ny\nz", 9)
    assert core.lines_device_raw(Q.ptr, 5)[0] == 3
    ids2, off2 = take_encoded(core, B, n, n_ids)
    assert ids2.tolist() == ids.tolist() and off2.tolist() == off.tolist()
    # ids -> text on the device: what the host's decode makes of the same ids
    d_ids, d_off = B.put(ids), B.put(off)
    n_bytes, _ = core.decode_device_raw(B.ptr(d_ids), B.ptr(d_off), n, n_ids, (a["bos"], a["eos"]))
    raw, o = core.fetch_decode(n, n_bytes)
    raw, o = raw.tobytes(), o.tolist()
    got = [raw[o[i]:o[i + 1]].decode() for i in range(n)]
    assert got == core.decode(want, [a["bos"], a["eos"]])
    alphabet = set(open(os.path.join(G, f"train_{name}.txt"), "rb").read().decode())
    same = [i for i, s in enumerate(lines) if set(s.decode()) <= alphabet | set(" \t")]
    assert len(same) > 20 and all(got[i] == " ".join(lines[i].decode().split()) for i in same)


def check_cache_modes(B, name="zipf"):
    core = core_of(name)
    data, _ = golden(name)
    data = data * 3 + b"no newline at the end"
    res = []
    for mode in (0, 1):
        core.set_cache(mode)
        ids, off = dev_encode_text(core, B, data, 1, 1, 0, align=8 * mode)  # (the cache needs 8-byte alignment: both modes at aligned text ...)
        res.append((ids.tolist(), off.tolist()))
        assert (core.cache_words() > 0) == (mode == 1)
        ids, off = dev_encode_text(core, B, data, 1, 1, 0, align=3)        # (... and mode 1 falls back to the direct path at an odd address)
        res.append((ids.tolist(), off.tolist()))
    h_ids, h_off = host_encode(core, data, 1, 1, 0)
    assert all(r == (h_ids.tolist(), h_off.tolist()) for r in res)


# ---- dropout ---------------------------------------------------------------------------------------------------------------------------
def check_dropout_all(B, name="readme_small"):
    """dropout_prob = 1: no merge survives, every line comes out as its characters' ids -- exactly what the existing path gives"""
    core = core_of(name)
    data = open(os.path.join(G, f"encode_{name}.lines"), "rb").read() + b"\n\nabc\xc3\nlast"
    for b, e, r in ((0, 0, 0), (1, 1, 1)):
        ids, off = dev_encode_text(core, B, data, b, e, r, dropout=1.0, align=2)
        h_ids, h_off = host_encode(core, data, b, e, r, dropout=1.0)
        assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist()


def check_dropout_distribution(B, name="readme_small", p=0.1, repeat=12):
    """dropout_prob = 0.1 on the input of the golden dropout_<name>.json (the same lines as encode_<name>.lines; `repeat` times, so that the
    count's own scatter is small against the bound): the draws differ per call, so the text route and the existing route are compared as
    distributions, by the criteria and bounds of stage_checks.check_dropout_distribution -- summed id count within 1 %, two-sample KS on the
    line lengths at alpha ~ 0.001, chi-square per degree of freedom of the unigram counts below 1.5."""
    from stage_checks import dropout_stats
    assert os.path.exists(os.path.join(G, f"dropout_{name}.json"))
    core = core_of(name)
    data = open(os.path.join(G, f"encode_{name}.lines"), "rb").read() * repeat
    vocab = core.vocab_size()
    ids, off = dev_encode_text(core, B, data, dropout=p)
    h_ids, h_off = host_encode(core, data, dropout=p)
    lg, hg = dropout_stats(rows(ids, off), vocab)
    lw, hw = dropout_stats(rows(h_ids, h_off), vocab)
    print(f"dropout p={p}: ids text route {int(lg.sum())}, existing route {int(lw.sum())}")
    assert len(lg) == len(lw)
    assert abs(lg.sum() - lw.sum()) / lw.sum() < 0.01, (lg.sum(), lw.sum())
    grid = np.arange(0, max(lw.max(), lg.max()) + 2)
    cw = np.searchsorted(np.sort(lw), grid, side="right") / len(lw)
    cg = np.searchsorted(np.sort(lg), grid, side="right") / len(lg)
    ks = np.abs(cw - cg).max()
    assert ks < 1.95 * np.sqrt(2.0 / len(lw)), ks
    mask = (hw + hg) >= 20
    chi = (((hg[mask] - hw[mask]) ** 2) / (hg[mask] + hw[mask])).sum() / max(1, mask.sum() - 1)
    assert chi < 1.5, chi


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def read_out(prefix):
    return np.fromfile(prefix + ".ids", np.int32), np.fromfile(prefix + ".off", np.uint64)


def check_file(name, tmp_path, flags=((0, 0, 0), (1, 1, 1))):
    """encode_file against the in-memory route and the golden, as arrays and as PREFIX.ids / PREFIX.off, with the file crossing in 1, 2 and
    many pieces: one and the same result"""
    core = core_of(name)
    a = model_args(name)
    data, want = golden(name)
    path = str(tmp_path / f"{name}.txt")
    open(path, "wb").write(data)
    text_off = py_offsets(data).tolist()
    longest = int(np.diff(np.array(text_off, np.int64)).max())
    cut_on_newline = text_off[len(text_off) // 3]  # the first piece ends exactly at its last byte, a newline
    sizes = [(None, 1), (len(data), 1), (len(data) + 1000, 1), ((len(data) + 1) // 2 + longest, 2), (cut_on_newline, None), (longest - 1, None), (7, None), (1, None)]
    for b, e, r in flags:
        if (b and a["bos"] == -1) or (e and a["eos"] == -1):
            continue
        h_ids, h_off = host_encode(core, data, b, e, r)
        key = f"{b}{e}{r}"
        if key in want:
            assert rows(h_ids, h_off) == want[key]
        for k, (chunk, pieces) in enumerate(sizes):
            ids, off, rep = core.encode_file(path, None, b, e, r, 0.0, chunk, report=True)
            assert ids.dtype == np.int32 and off.dtype == np.uint64
            assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist(), (name, key, chunk)
            assert rep["lines"] == len(h_off) - 1 and rep["ids"] == len(h_ids) and rep["bytes"] == len(data)
            if pieces == 1:
                assert rep["pieces"] == 1, (chunk, rep)
            elif chunk == 1:
                assert rep["pieces"] == len(h_off) - 1, (chunk, rep)  # every line is a piece of its own: none was cut
            elif len(data) > 1000:
                assert rep["pieces"] == pieces if pieces else rep["pieces"] > 2, (chunk, rep)
            prefix = str(tmp_path / f"out_{key}_{k}")
            n_lines, n_ids = core.encode_file(path, prefix, b, e, r, 0.0, chunk)
            f_ids, f_off = read_out(prefix)
            assert (n_lines, n_ids) == (len(h_off) - 1, len(h_ids))
            assert f_ids.tolist() == h_ids.tolist() and f_off.tolist() == h_off.tolist(), (name, key, chunk)


def check_file_edges(tmp_path, name="readme_small"):
    import pytest
    import youtokentome_amd as yttm
    bpe = yttm.BPE(os.path.join(G, f"train_{name}.model"))
    core = bpe.bpe_cython
    for i, data in enumerate([b"", b"\n", b"\n\n", b"a", b"no newline", b"ab\xc3\ncd\xe2\x82", b"x\n" * 300 + b"y" * 5000 + b"\nz"]):
        path = str(tmp_path / f"edge{i}.txt")
        open(path, "wb").write(data)
        h_ids, h_off = host_encode(core, data, 1, 1, 0)
        for chunk in (None, 1, 3, 4096):
            ids, off = bpe.encode_file(path, bos=True, eos=True, chunk_bytes=chunk)
            assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist(), (i, chunk)
            assert bpe.encode_file(path, out=str(tmp_path / "edge_out"), bos=True, eos=True, chunk_bytes=chunk) == (len(h_off) - 1, len(h_ids))
            f_ids, f_off = read_out(str(tmp_path / "edge_out"))
            assert f_ids.tolist() == h_ids.tolist() and f_off.tolist() == h_off.tolist(), (i, chunk)
    path = str(tmp_path / "edge4.txt")
    with pytest.raises(ValueError, match="Failed to open file: .*no_such_file"):
        bpe.encode_file(str(tmp_path / "no_such_file.txt"))
    with pytest.raises(ValueError, match="Failed to open file for writing: .*no_such_dir"):
        bpe.encode_file(path, out=str(tmp_path / "no_such_dir" / "out"))
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_file(path, dropout_prob=1.5)
    nopad = yttm.BPE(os.path.join(G, "train_nopad.model"))
    with pytest.raises(ValueError, match="Can't add <BOS> token. Model was trained without it."):
        nopad.encode_file(path, bos=True)
    # dropout through the file route: p = 1 is deterministic
    ids, off = bpe.encode_file(path, dropout_prob=1.0, chunk_bytes=5)
    h_ids, h_off = host_encode(core, open(path, "rb").read(), dropout=1.0)
    assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist()


def check_file_write_failure(tmp_path, name="readme_small"):
    """A full disk under PREFIX.ids or PREFIX.off (a link to /dev/full: pwrite gives ENOSPC inside the download thread, whatever the piece
    size) is this call's error -- and the same BPE object goes on to encode the file: both lanes were released and are as good as before"""
    import pytest
    import youtokentome_amd as yttm
    bpe = yttm.BPE(os.path.join(G, f"train_{name}.model"))
    data, _ = golden(name)
    path = str(tmp_path / f"{name}.txt")
    open(path, "wb").write(data)
    h_ids, h_off = host_encode(bpe.bpe_cython, data)
    for full in (".ids", ".off"):
        prefix = str(tmp_path / f"full{full[1:]}")
        os.symlink("/dev/full", prefix + full)
        for chunk in (None, 1, 700):
            with pytest.raises(ValueError, match=r"Failed to write file: .*\.ids / \.off"):
                bpe.encode_file(path, out=prefix, chunk_bytes=chunk)
            ids, off = bpe.encode_file(path, chunk_bytes=chunk)
            assert ids.tolist() == h_ids.tolist() and off.tolist() == h_off.tolist(), (full, chunk)


def check_cli(tmp_path, name="readme_small"):
    """`yttm encode_file` writes the same two files"""
    core = core_of(name)
    data, _ = golden(name)
    path, model = str(tmp_path / "in.txt"), os.path.join(G, f"train_{name}.model")
    open(path, "wb").write(data)
    for extra, (b, e, r) in ((["--bos", "--eos"], (1, 1, 0)), (["--reverse"], (0, 0, 1))):
        prefix = str(tmp_path / ("cli" + "".join(extra)))
        r_ = subprocess.run([sys.executable, "-m", "youtokentome_amd.yttm_cli", "encode_file", f"--model={model}", f"--input={path}", f"--output={prefix}"] + extra,
                            capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r_.returncode == 0, r_.stderr.decode()
        f_ids, f_off = read_out(prefix)
        h_ids, h_off = host_encode(core, data, b, e, r)
        assert f_ids.tolist() == h_ids.tolist() and f_off.tolist() == h_off.tolist()
