"""Training blocks on the device on a real MI355X: the cases of blocks_checks.py with torch tensors as device memory, against the rule written as
Python loops and against the array properties; plus the tensor API, the input at all sixteen element offsets and one larger pass."""
import pytest

import blocks_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


@pytest.mark.parametrize("L", S.LENGTHS)
def test_every_seq_len(B, L):
    S.check_lengths(B, (L,))


def test_boundaries_empty_runs_edge_values(B):
    S.check_boundaries(B)


def test_orbit_skips_a_block(B):
    S.check_orbit_skip(B)


def test_whole_mode_fits(B):
    S.check_whole_fits(B)


def test_sentence_longer_than_seq_len(B):
    S.check_too_long(B)


def test_every_alignment(B):
    S.check_alignment(B, shifts=tuple(range(16)))


def test_batch_cut_into_calls(B):
    S.check_split_calls(B)


def test_open_row_binding_and_exits(B):
    S.check_binding_and_exits(B)


@pytest.mark.parametrize("name", S.all_models())
def test_pending_golden_models(B, name):
    S.check_pending_model(B, name)


def test_pending_parse_restricted_empty(B):
    S.check_pending_misc(B)


def test_dropout(B):
    S.check_dropout(B)


def test_file_route(B, tmp_path):
    S.check_file(B, tmp_path)


def test_file_dropout(tmp_path):
    S.check_file_dropout(tmp_path)


def test_file_errors(B, tmp_path):
    S.check_file_errors(B, tmp_path)


def test_encode_file_blocks_and_cli(tmp_path):
    S.check_python_and_cli(tmp_path)


def test_tensor_api():
    S.check_tensor_api()


def test_large_batch(B):
    S.check_large(B)
