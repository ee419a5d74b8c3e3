"""The line split on the device and the encoder's entries for unsplit text on a real MI355X: the cases of lines_checks.py with torch tensors as
device memory, the tensor API on top (BPE.encode_text_tensor, BPE.text_lines_tensor), and the full-size pins through a file."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import gen
import lines_checks as K

pytestmark = pytest.mark.gpu

G = K.G


@pytest.fixture()
def B():
    return K.TorchBuf()


def test_split_cases_at_every_alignment(B):
    K.check_split_cases(K.core_of("readme_small"), B)


def test_split_long_line_and_many_lines(B):
    K.check_split_large(K.core_of("readme_small"), B)


@pytest.mark.parametrize("name", K.golden_names())
def test_golden_texts(B, name):
    K.check_golden(B, name)


def test_invalid_utf8_and_empty_lines(B):
    K.check_odd_texts(B)


def test_errors(B):
    K.check_errors(B)


def test_padded_hand_over_and_round_trip(B):
    K.check_padded_and_round_trip(B)


def test_word_cache_modes(B):
    K.check_cache_modes(B)


def test_dropout_of_every_merge(B):
    K.check_dropout_all(B)


def test_dropout_distribution(B):
    K.check_dropout_distribution(B, repeat=40)


@pytest.mark.parametrize("name", K.golden_names())
def test_file_in_pieces(name, tmp_path):
    K.check_file(name, tmp_path)


def test_file_edges_and_errors(tmp_path):
    K.check_file_edges(tmp_path)


def test_file_write_failure_releases_the_lanes(tmp_path):
    K.check_file_write_failure(tmp_path)


def test_command_line(tmp_path):
    K.check_cli(tmp_path)


def _repad(ids, width, pad):
    m = np.full((len(ids), width), pad, np.int32)
    for i, s in enumerate(ids):
        m[i, :len(s)] = s
    return m


def test_text_tensor_api():
    """BPE.encode_text_tensor / text_lines_tensor: a uint8 tensor (at an odd address too) or bytes in, what encode_tensor returns out"""
    import torch
    import youtokentome_amd as yttm
    bpe = yttm.BPE(os.path.join(G, "train_readme_small.model"))
    data = open(os.path.join(G, "encode_readme_small.lines"), "rb").read() + b"\n\nab\xc3\nlast line"
    lines = K.py_split(data)
    text_off = K.py_offsets(data).astype(np.int64).tolist()
    whole = torch.frombuffer(bytearray(b"\n\n\n" + data + b"\n\n"), dtype=torch.uint8).cuda()
    sources = [data, bytearray(data), memoryview(data), whole[3:3 + len(data)]]
    for b, e, r in ((0, 0, 0), (1, 1, 0), (1, 0, 1)):
        h_ids, h_off = K.host_encode(bpe.bpe_cython, data, b, e, r)
        want = K.rows(h_ids, h_off)
        longest = max(len(s) for s in want)
        for src in sources:
            m, lens = bpe.encode_text_tensor(src, bos=bool(b), eos=bool(e), reverse=bool(r))
            assert m.dtype == torch.int32 and lens.dtype == torch.int32 and m.is_cuda and lens.is_cuda
            assert tuple(m.shape) == (len(lines), longest) and lens.cpu().tolist() == [len(s) for s in want]
            assert np.array_equal(m.cpu().numpy(), _repad(want, longest, 0))
            m, lens = bpe.encode_text_tensor(src, bos=bool(b), eos=bool(e), reverse=bool(r), width=longest + 5, pad_id=-100)
            assert np.array_equal(m.cpu().numpy(), _repad(want, longest + 5, -100))
            ids, off = bpe.encode_text_tensor(src, bos=bool(b), eos=bool(e), reverse=bool(r), padded=False)
            assert ids.dtype == torch.int32 and off.dtype == torch.int64
            assert ids.cpu().tolist() == h_ids.tolist() and off.cpu().tolist() == h_off.astype(np.int64).tolist()
            t_off = bpe.text_lines_tensor(src)
            assert t_off.dtype == torch.int64 and t_off.is_cuda and t_off.cpu().tolist() == text_off
    # decode_tensor takes the result back
    m, lens = bpe.encode_text_tensor(data, bos=True, eos=True)
    assert bpe.decode_tensor(m, lengths=lens, ignore_ids=[2, 3]) == bpe.decode(K.rows(*K.host_encode(bpe.bpe_cython, data)))
    # empty text, and the checks of encode_tensor
    m, lens = bpe.encode_text_tensor(b"")
    assert tuple(m.shape) == (0, 0) and lens.numel() == 0
    assert bpe.text_lines_tensor(b"").cpu().tolist() == [0]
    assert bpe.text_lines_tensor(b"\n").cpu().tolist() == [0, 1]
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_text_tensor(b"a", dropout_prob=1.5)
    with pytest.raises(ValueError, match="smaller than the longest row"):
        bpe.encode_text_tensor(data, width=1)
    with pytest.raises(ValueError, match="text is a 1-D uint8 tensor"):
        bpe.encode_text_tensor(torch.zeros(4, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="the encoder on"):
        bpe.encode_text_tensor(torch.zeros(4, dtype=torch.uint8))
    nopad = yttm.BPE(os.path.join(G, "train_nopad.model"))
    with pytest.raises(ValueError, match="trained without <PAD>"):
        nopad.encode_text_tensor(b"ab\n")
    with pytest.raises(ValueError, match="Can't add <BOS> token. Model was trained without it."):
        nopad.encode_text_tensor(b"ab\n", bos=True, pad_id=0)


def test_zz_full_size_file_pins(tmp_path):
    """The inputs of test_zz_full_size_pins through a file: the c2_1gb model, the 10^7 x 129-byte stream of C4 written to disk (md5 pinned), and
    the reference's own n_ids and FNV-1a-64 (tests/golden/full_size_pins.json c4_10m) from encode_file -- arrays with the default piece size,
    files with a small one -- and from encode_text_device on the same bytes in HBM."""
    import torch
    import youtokentome_amd as yttm
    from youtokentome_amd import _lib
    pins = json.load(open(os.path.join(G, "full_size_pins.json")))
    pin, p4 = pins["c2_1gb"], pins["c4_10m"]
    text = gen.abcd_corpus(pin["corpus_bytes"] + 1, seed=19, survey_stream=True)
    assert hashlib.md5(text).hexdigest() == pin["corpus_md5"]
    corpus, model = str(tmp_path / "c2.txt"), str(tmp_path / "c2.model")
    open(corpus, "wb").write(text)
    del text
    bpe = yttm.BPE.train(corpus, model, pin["vocab_size"])
    os.remove(corpus)
    assert hashlib.md5(open(model, "rb").read()).hexdigest() == pin["model_md5"]
    line, n = 128, p4["n_sentences"]
    sents = gen.abcd_corpus(n * (line + 1), seed=123, line=line, survey_stream=True)
    assert hashlib.md5(sents).hexdigest() == p4["input_md5"]
    path = str(tmp_path / "c4.txt")
    open(path, "wb").write(sents)
    L = _lib.load()

    def fnv(ids, off):
        assert ids.dtype == np.int32 and off.dtype == np.uint64 and ids.flags.c_contiguous and off.flags.c_contiguous
        return "%016x" % L.yttm_ids_fnv1a64(ids.ctypes.data_as(_lib.i32p), off.ctypes.data_as(_lib.u64p), len(off) - 1)

    core = bpe.bpe_cython
    ids, off, rep = core.encode_file(path, report=True)
    print("encode_file, default piece size:", rep)
    assert len(off) == n + 1 and len(ids) == p4["n_ids"] and fnv(ids, off) == p4["fnv1a64"]
    del ids, off
    prefix = str(tmp_path / "c4_small")
    assert bpe.encode_file(path, out=prefix, chunk_bytes=48 << 20) == (n, p4["n_ids"])
    ids, off = K.read_out(prefix)
    assert len(off) == n + 1 and len(ids) == p4["n_ids"] and fnv(ids, off) == p4["fnv1a64"]
    del ids, off
    os.remove(prefix + ".ids")
    os.remove(path)
    d_text = torch.frombuffer(bytearray(sents), dtype=torch.uint8).cuda()
    del sents
    torch.cuda.synchronize()
    n_lines, n_ids, ms = core.encode_text_device_raw(d_text.data_ptr(), d_text.numel())
    print("encode_text_device: kernel_ms", ms)
    assert (n_lines, n_ids) == (n, p4["n_ids"])
    ids, off = core.fetch_encode(n_lines, n_ids)
    assert fnv(np.ascontiguousarray(ids), off) == p4["fnv1a64"]
