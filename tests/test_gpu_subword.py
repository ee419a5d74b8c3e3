"""SUBWORD output on the device on a real MI355X: the cases of subword_checks.py with torch tensors as device memory, against the host path
yttm_encode_as_subwords, the goldens and the independent formatter; plus the tensor API and one larger pass."""
import pytest

import subword_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


@pytest.mark.parametrize("name", S.golden_names())
def test_golden_models(B, name):
    S.check_golden(B, name)


def test_sentence_lengths(B):
    S.check_lengths(B)


def test_unknown_runs(B):
    S.check_unknown_runs(B)


def test_long_piece(B, tmp_path):
    S.check_long_piece(B, tmp_path)


def test_groups_of_short_sentences(B):
    S.check_groups(B)


def test_sentences_that_fill_the_tile(B):
    S.check_full_tile(B)


def test_errors_and_pending_results(B):
    S.check_errors(B)


def test_dropout_against_the_formatter(B):
    S.check_dropout(B)


def test_unsplit_text(B):
    S.check_text(B)


def test_file_in_pieces(tmp_path):
    S.check_file(tmp_path)


def test_file_errors_and_the_id_default(tmp_path):
    S.check_file_errors(tmp_path)


def test_command_line(tmp_path):
    S.check_cli(tmp_path)


def test_large_batch(B):
    S.check_large(B)


def test_tensor_api():
    """encode_subword_tensor / encode_text_subword_tensor: tensors on the device, or the lines as strings == BPE.encode(SUBWORD) joined"""
    import torch
    import youtokentome_amd as yttm
    bpe = S.bpe_of("readme_small")
    sents = S.golden_sentences("readme_small")[:50] + ["", "ab Z cd", "é中 ab", " "]
    for b, e, r in S.FLAGS:
        want = ["".join(p + " " for p in row) + "\n" for row in bpe.encode(sents, yttm.OutputType.SUBWORD, bos=bool(b), eos=bool(e), reverse=bool(r))]
        assert bpe.encode_subword_tensor(sents, bos=b, eos=e, reverse=r, as_str=True) == want
        text, off = bpe.encode_subword_tensor(sents, bos=b, eos=e, reverse=r)
        assert text.dtype == torch.uint8 and off.dtype == torch.int64 and text.is_cuda and off.is_cuda and off.numel() == len(sents) + 1
        assert bytes(text.cpu().numpy()) == "".join(want).encode() and off.cpu().tolist()[-1] == text.numel()
        blob = "\n".join(sents).encode() + b"\n"
        assert bpe.encode_text_subword_tensor(blob, bos=b, eos=e, reverse=r, as_str=True) == want
        t2, o2 = bpe.encode_text_subword_tensor(torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda(), bos=b, eos=e, reverse=r)
        assert torch.equal(t2, text) and torch.equal(o2, off)
    assert bpe.encode_subword_tensor([], as_str=True) == []
    with pytest.raises(ValueError, match="dropout_prob value must be in the range"):
        bpe.encode_subword_tensor(sents, dropout_prob=1.5)
