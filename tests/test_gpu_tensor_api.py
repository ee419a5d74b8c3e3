"""BPE.encode_tensor / BPE.decode_tensor (youtokentome_amd/tensor.py) with torch tensors on a real MI355X: device tensors in, device tensors
out, against the list API of the same object (BPE.encode / BPE.decode, which the reference suite pins)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import decode_checks as D
import gen

pytestmark = pytest.mark.gpu

G = D.G


def _bpe(name="readme_small"):
    import youtokentome_amd as yttm
    return yttm.BPE(os.path.join(G, f"train_{name}.model"))


def _sentences(name="readme_small"):
    rng = random.Random(2)
    return D.golden_sentences(name) + ["", " ", "abcd " * 200] + ["".join(rng.choice("abcd ") for _ in range(rng.randint(0, 60))) for _ in range(500)]


def _repad(ids, width, pad):
    m = np.full((len(ids), width), pad, np.int32)
    for i, s in enumerate(ids):
        m[i, :len(s)] = s
    return m


def _device_input(torch, sents):
    raw = [s.encode() for s in sents]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return torch.frombuffer(bytearray(b"".join(raw) + b"\0"), dtype=torch.uint8)[:-1].cuda(), torch.from_numpy(off).cuda()


def test_encode_tensor_equals_encode():
    import torch
    import youtokentome_amd as yttm
    bpe, sents = _bpe(), _sentences()
    for b, e, r in ((0, 0, 0), (1, 1, 0), (1, 0, 1)):
        want = bpe.encode(sents, yttm.OutputType.ID, bos=bool(b), eos=bool(e), reverse=bool(r))
        longest = max(len(s) for s in want)
        for source in (sents, _device_input(torch, sents)):
            m, lens = bpe.encode_tensor(source, bos=bool(b), eos=bool(e), reverse=bool(r))
            assert m.dtype == torch.int32 and lens.dtype == torch.int32 and m.is_cuda and lens.is_cuda
            assert tuple(m.shape) == (len(sents), longest)
            assert lens.cpu().tolist() == [len(s) for s in want]
            assert np.array_equal(m.cpu().numpy(), _repad(want, longest, 0))
            m, lens = bpe.encode_tensor(source, bos=bool(b), eos=bool(e), reverse=bool(r), width=longest + 9, pad_id=-100)
            assert np.array_equal(m.cpu().numpy(), _repad(want, longest + 9, -100))
            ids, off = bpe.encode_tensor(source, bos=bool(b), eos=bool(e), reverse=bool(r), padded=False)
            assert ids.dtype == torch.int32 and off.dtype == torch.int64 and ids.is_cuda and off.is_cuda
            assert ids.cpu().tolist() == [t for s in want for t in s]
            assert off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
    m, lens = bpe.encode_tensor([])
    assert tuple(m.shape) == (0, 0) and lens.numel() == 0


def test_decode_tensor_equals_decode():
    import torch
    import youtokentome_amd as yttm
    bpe, sents = _bpe(), _sentences()
    ids = bpe.encode(sents, yttm.OutputType.ID, bos=True, eos=True)
    for ignore in (None, [2, 3], {0, 2, 3}):
        want = bpe.decode(ids, ignore_ids=ignore)
        longest = max(len(s) for s in ids)
        m = torch.from_numpy(_repad(ids, longest + 2, 0)).cuda()
        lens = torch.tensor([len(s) for s in ids], dtype=torch.int32).cuda()
        assert bpe.decode_tensor(m, lengths=lens, ignore_ids=ignore) == want
        assert bpe.decode_tensor(m.to(torch.int64), lengths=lens.to(torch.int64), ignore_ids=ignore) == want  # int64: one conversion
        flat = torch.tensor([t for s in ids for t in s], dtype=torch.int32).cuda()
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in ids])]).astype(np.int64)).cuda()
        assert bpe.decode_tensor(flat, offsets=off, ignore_ids=ignore) == want
        assert bpe.decode_tensor(flat.to(torch.int64), offsets=off, ignore_ids=ignore) == want
        # non-contiguous: a column slice of a wider matrix (the row stride is passed through), and a transposed one (made contiguous)
        wide = torch.full((len(ids), longest + 40), 7, dtype=torch.int32).cuda()
        wide[:, 5:longest + 7] = m
        view = wide[:, 5:longest + 7]
        assert not view.is_contiguous()
        assert bpe.decode_tensor(view, lengths=lens, ignore_ids=ignore) == want
        t = m.t().contiguous().t()
        assert not t.is_contiguous()
        assert bpe.decode_tensor(t, lengths=lens, ignore_ids=ignore) == want
        every_other = torch.stack([flat, flat], dim=1)[:, 0]
        assert not every_other.is_contiguous()
        assert bpe.decode_tensor(every_other, offsets=off, ignore_ids=ignore) == want
        # without lengths the pad id is ignored away
        if ignore is not None and 0 in ignore:
            assert bpe.decode_tensor(m, ignore_ids=ignore) == want
        # the text left on the device
        text, toff = bpe.decode_tensor(m, lengths=lens, ignore_ids=ignore, as_str=False)
        assert text.dtype == torch.uint8 and toff.dtype == torch.int64 and text.is_cuda and toff.is_cuda
        raw, o = text.cpu().numpy().tobytes(), toff.cpu().tolist()
        assert [raw[o[i]:o[i + 1]].decode() for i in range(len(ids))] == want
    # encode_tensor -> decode_tensor without leaving the device
    m, lens = bpe.encode_tensor(sents)
    assert bpe.decode_tensor(m, lengths=lens) == bpe.decode(bpe.encode(sents, yttm.OutputType.ID))


def test_value_errors():
    import torch
    bpe = _bpe()
    nopad = _bpe("nopad")
    with pytest.raises(ValueError):
        nopad.encode_tensor(["ab cd"])  # trained with pad_id=-1: the argument is required
    m, lens = nopad.encode_tensor(["ab cd", "a"], pad_id=-1)
    assert m.shape[0] == 2 and int(m[1, -1]) == -1
    with pytest.raises(ValueError):
        bpe.encode_tensor(["abcd abcd abcd", "a"], width=1)  # narrower than the longest row
    with pytest.raises(ValueError):
        bpe.encode_tensor(["a"], bos=True, eos=True, dropout_prob=1.5)
    with pytest.raises(ValueError):
        nopad.encode_tensor(["a"], bos=True, pad_id=0)  # the library's own error: no <BOS> in the model
    ids = torch.tensor([[5, 6, 7]], dtype=torch.int32)
    with pytest.raises(ValueError):
        bpe.decode_tensor(ids)  # a host tensor: another device than the encoder's
    with pytest.raises(ValueError):
        bpe.encode_tensor(["a"], device="cpu")
    with pytest.raises(ValueError):
        bpe.decode_tensor(ids.cuda().to(torch.float32))
    with pytest.raises(ValueError):
        bpe.decode_tensor(ids.cuda()[0])  # 1-D without offsets
    with pytest.raises(ValueError) as e:
        bpe.decode_tensor(torch.tensor([[5, bpe.vocab_size(), 7]], dtype=torch.int32).cuda())
    assert "id must be in the range [0, vocab_size - 1]" in str(e.value)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            bpe.decode_tensor(ids.to("cuda:1"))


def test_stream_hand_over():
    """the input is produced by torch kernels queued right before the call (on torch's stream; the library works on its own)"""
    import torch
    import youtokentome_amd as yttm
    bpe = _bpe()
    V = bpe.vocab_size()
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    for _ in range(3):
        base = torch.randint(4, V, (4000, 300), generator=g, device="cuda", dtype=torch.int64)
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            big = big @ big  # keeps the stream busy in front of the producer below
            big = big / big.abs().max()
        ids = ((base * 7 + 3) % (V - 4) + 4).to(torch.int32)  # queued, not waited for
        got = bpe.decode_tensor(ids)
        assert got == bpe.decode(ids.cpu().tolist())
        text = "abcd abc dcba " * 2000
        raw = torch.frombuffer(bytearray(text.encode()), dtype=torch.uint8).cuda()
        shifted = (raw + 1) - 1  # a kernel's output
        off = torch.arange(0, len(text) + 1, 14, dtype=torch.int64, device="cuda")
        m, lens = bpe.encode_tensor((shifted, off))
        want = bpe.encode([text[i:i + 14] for i in range(0, len(text), 14)], yttm.OutputType.ID)
        assert m.cpu().tolist() == _repad(want, max(len(s) for s in want), 0).tolist()


def test_full_size_decode():
    """the ids of the 10^7 x 128-char encode batch of bench.py --full (the same generator and seed), decoded on the device, against the host
    yttm_decode of the same ids"""
    import torch
    from bench import ENCODE_LINE
    from youtokentome_amd import _lib
    n_want = 10_000_000
    host = gen.abcd_corpus(n_want * (ENCODE_LINE + 1), seed=123, line=ENCODE_LINE, survey_stream=True)
    n = len(host) // (ENCODE_LINE + 1)
    assert n == n_want
    bpe = _bpe()
    d_bytes = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    del host
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * (ENCODE_LINE + 1)
    ids, off = bpe.encode_tensor((d_bytes, d_off), padded=False)
    del d_bytes
    text, toff = bpe.decode_tensor(ids, offsets=off, as_str=False)
    h_ids, h_off = ids.cpu().numpy(), off.cpu().numpy().astype(np.uint64)
    L = _lib.load()
    blob_p, ooff, err = C.c_void_p(), _lib.u64p(), C.create_string_buffer(_lib.ERRLEN)
    rc = L.yttm_decode(bpe.bpe_cython._h, h_ids.ctypes.data_as(_lib.i32p), h_off.ctypes.data_as(_lib.u64p), n, None, 0, C.byref(blob_p), C.byref(ooff), err, _lib.ERRLEN)
    assert rc == 0, err.value
    want_off = np.ctypeslib.as_array(ooff, shape=(n + 1,))
    got_off = toff.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_off, want_off)
    total = int(want_off[-1])
    assert total == text.numel() and total > 64 * n
    want = np.ctypeslib.as_array(C.cast(blob_p, C.POINTER(C.c_uint8)), shape=(total,))
    assert np.array_equal(text.cpu().numpy(), want)
    L.yttm_free(blob_p)
    L.yttm_free(C.cast(ooff, C.c_void_p))
