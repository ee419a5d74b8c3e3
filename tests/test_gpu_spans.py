"""Byte spans on the device on a real MI355X: the cases of spans_checks.py with torch tensors as device memory, against the rule written out in
Python and the property check; plus the tensor API and one larger pass."""
import pytest

import spans_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


@pytest.mark.parametrize("name", S.all_models())
def test_golden_models(B, name):
    S.check_golden(B, name)


def test_dropout(B):
    S.check_dropout(B)


def test_id_zero_quirk(B, tmp_path):
    S.check_id0_quirk(B, tmp_path)


def test_step_boundaries(B):
    S.check_step_boundaries(B)


def test_large_sentences(B, tmp_path):
    S.check_large_sentences(B, tmp_path)


def test_spaces_and_invalid_bytes(B):
    S.check_spaces_and_invalid(B)


def test_groups_at_every_alignment(B):
    S.check_groups(B, aligns=tuple(range(16)))


def test_api_forms(B):
    S.check_api_forms(B)


def test_errors_and_pending_results(B):
    S.check_errors(B)


def test_large_batch(B):
    S.check_large(B)


def test_tensor_api():
    """encode_spans_tensor / encode_text_spans_tensor: int32 tensors on the device, padded and ragged == the list API in bytes"""
    import torch
    bpe = S.model("readme_small").bpe
    sents = S.sentences_of("readme_small")[:50] + ["", "ab Z cd", "é中 ab", " "]
    for b, e, r in S.FLAGS:
        want_ids, want = bpe.encode_with_spans(sents, bos=bool(b), eos=bool(e), reverse=bool(r), unit="byte")
        flat = [list(p) for row in want for p in row]
        ids, off, spans = bpe.encode_spans_tensor(sents, bos=b, eos=e, reverse=r, padded=False)
        assert ids.dtype == torch.int32 and off.dtype == torch.int64 and spans.dtype == torch.int32 and spans.is_cuda and tuple(spans.shape) == (ids.numel(), 2)
        assert ids.cpu().tolist() == [t for row in want_ids for t in row] and spans.cpu().tolist() == flat
        longest = max(len(row) for row in want)
        for width in (None, longest + 2):
            m, lengths, sp = bpe.encode_spans_tensor(sents, bos=b, eos=e, reverse=r, width=width)
            w = width or longest
            assert tuple(sp.shape) == (len(sents), w, 2) and tuple(m.shape) == (len(sents), w) and lengths.cpu().tolist() == [len(row) for row in want]
            assert sp.cpu().tolist() == [[list(p) for p in row] + [[0, 0]] * (w - len(row)) for row in want]
        blob = "\n".join(sents).encode() + b"\n"
        i2, o2, s2 = bpe.encode_text_spans_tensor(blob, bos=b, eos=e, reverse=r, padded=False)
        assert torch.equal(i2, ids) and torch.equal(o2, off) and torch.equal(s2, spans)
    ids, off, spans = bpe.encode_spans_tensor([], padded=False)
    assert ids.numel() == 0 and off.cpu().tolist() == [0] and tuple(spans.shape) == (0, 2)
    with pytest.raises(ValueError, match="width = 1 is smaller"):
        bpe.encode_spans_tensor(sents, width=1)
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_spans_tensor(sents, dropout_prob=1.5)
