"""Encode under a restricted vocabulary on a real MI355X: the cases of restrict_checks.py with torch tensors as device memory, against the rule
as a Python recursion over the model file's rules and against the properties; the input of the pass at all sixteen element offsets between
guard ids that would split if read; plus the tensor API and one larger pass."""
import pytest

import restrict_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


def test_pass_on_synthetic_ids_at_every_alignment(B):
    S.check_synthetic(B, shifts=tuple(range(16)))


def test_expansions_longer_than_the_tile(B, tmp_path):
    S.check_long(B, tmp_path)


@pytest.mark.parametrize("name", S.all_models())
def test_encode_device_golden_models(B, name):
    S.check_routes_model(B, name)


def test_dropout_with_the_salt_pinned(B):
    S.check_dropout(B)


def test_python_spans_and_subword_routes(B):
    S.check_python_routes(B)


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
