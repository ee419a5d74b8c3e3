"""The added tokens on a real MI355X: the cases of added_checks.py with torch tensors as device memory, against the matcher and the join in
Python; the text of the split at all sixteen byte offsets, between guard bytes that complete a token if they are read; plus the tensor API and
one larger pass."""
import pytest

import added_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


def test_split_on_synthetic_text_at_every_alignment(B):
    S.check_synthetic(B, aligns=tuple(range(16)))


@pytest.mark.parametrize("name", S.all_models())
def test_encode_device_golden_models(B, name):
    S.check_routes_model(B, name)


def test_bos_eos_reverse_and_small_sentences(B):
    S.check_small_cases(B)


def test_dropout_with_the_salt_pinned(B):
    S.check_dropout(B)


def test_with_a_restricted_vocabulary_and_byte_fallback(B):
    S.check_with_settings(B)


def test_python_names_subword_decode_counts_and_spans(B):
    S.check_python_routes(B)


def test_blocks_and_batches_of_the_pending_result(B):
    S.check_blocks_and_batches(B)


def test_file_routes(B, tmp_path):
    S.check_files(B, tmp_path)


def test_errors(B):
    S.check_errors(B)


def test_command_line(tmp_path):
    S.check_cli(tmp_path)


def test_tensor_api():
    S.check_tensor_api()


def test_large_batch(B):
    S.check_large(B)
