"""The byte fallback on a real MI355X: the cases of bytefb_checks.py with torch tensors as device memory, against the rule in Python and the
round trip; the input of the pass at all sixteen element offsets of the ids and all sixteen byte offsets of the text, between guard ids and
bytes that would change the result if read; plus the tensor API and one larger pass."""
import pytest

import bytefb_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


def test_pass_on_synthetic_ids_and_text_at_every_alignment(B):
    S.check_synthetic(B, shifts=tuple(range(16)), aligns=tuple(range(16)))


@pytest.mark.parametrize("name", S.all_models())
def test_encode_device_golden_models(B, name):
    S.check_routes_model(B, name)


def test_dropout_with_the_salt_pinned(B):
    S.check_dropout(B)


def test_with_a_restricted_vocabulary(B):
    S.check_with_vocabulary(B)


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
