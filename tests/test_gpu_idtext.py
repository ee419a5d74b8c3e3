"""Decimal id text on the device on a real MI355X: the cases of idtext_checks.py with torch tensors as device memory, every text at every address
alignment, against the Python parser, yttm_decode_cli and yttm_encode_cli; plus the tensor API and one larger pass.  The whole file was measured at
14.6 s, 6.3 s of it the command line's process starts (14 then, 10 now); every other test takes about a second or less."""
import pytest

import idtext_checks as T

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return T.TorchBuf()


def test_line_structure(B):
    T.check_line_structure(B)


def test_signs_and_glue(B):
    T.check_signs(B)


def test_fail_points(B):
    T.check_fail_points(B)


def test_int32_range_and_long_runs(B):
    T.check_range(B)


def test_steps_at_every_shift(B):
    T.check_steps(B)


def test_groups_of_lines(B):
    T.check_groups(B)


def test_random_byte_soup(B):
    T.check_soup(B)


@pytest.mark.parametrize("name", T.golden_names())
def test_golden_models(B, name):
    T.check_golden(B, name)


def test_every_digit_count(B):
    T.check_digit_counts(B)


def test_pending_results(B):
    T.check_pending(B)


def test_long_pieces_between_newlines(B, tmp_path):
    T.check_long_piece_lines(B, tmp_path)


def test_decode_file_in_pieces(tmp_path):
    T.check_decode_file(tmp_path)


def test_id_text_file_in_pieces(tmp_path):
    T.check_idtext_file(tmp_path)


def test_file_errors(tmp_path):
    T.check_file_errors(tmp_path)


def test_command_line(tmp_path):
    T.check_cli(tmp_path)


def test_large_batch(B):
    T.check_large(B)


def test_tensor_api():
    """parse_ids_tensor / decode_text_tensor: tensors on the device, or the lines as strings == BPE.decode of the parsed ids"""
    import torch
    bpe = T.S.bpe_of("readme_small")
    rows = [[5, 6, 7], [], [8], [9, 10, 11, 12]]
    text = T.py_print(rows) + b"13 x 14"
    rows.append([13])
    for src in (text, torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()):
        ids, off = bpe.parse_ids_tensor(src)
        assert ids.dtype == torch.int32 and off.dtype == torch.int64 and ids.is_cuda and off.is_cuda
        assert ids.cpu().tolist() == [t for r in rows for t in r] and off.cpu().tolist() == [0, 3, 3, 4, 8, 9]
        m, lens = bpe.parse_ids_tensor(src, padded=True, pad_id=-1)
        assert lens.cpu().tolist() == [3, 0, 1, 4, 1] and m.shape == (5, 4) and m.cpu().tolist()[2] == [8, -1, -1, -1]
        assert bpe.decode_text_tensor(src) == bpe.decode(rows)
        t, o = bpe.decode_text_tensor(src, as_str=False)
        assert t.dtype == torch.uint8 and o.dtype == torch.int64 and t.is_cuda and o.numel() == 6
        assert bytes(t.cpu().numpy()) == "".join(s + "\n" for s in bpe.decode(rows)).encode() and o.cpu().tolist()[-1] == t.numel()
    assert bpe.decode_text_tensor(b"5 6 7\n", ignore_ids=[6]) == bpe.decode([[5, 6, 7]], ignore_ids=[6])
    assert bpe.decode_text_tensor(b"") == []
    with pytest.raises(ValueError, match="99999"):
        bpe.decode_text_tensor(b"5 99999\n")
