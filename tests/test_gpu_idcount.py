"""Token frequencies on the device on a real MI355X: the cases of idcount_checks.py with torch tensors as device memory, against numpy.bincount
of the synthetic arrays and of the ids the existing routes return; plus the tensor API and one larger pass.  Window edges inside a 600-bin
histogram through YTTM_IDCOUNT_WINDOW."""
import pytest

import idcount_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


def test_sizes_at_every_alignment(B):
    S.check_sizes(B, shifts=tuple(range(16)))


def test_edge_values(B):
    S.check_edge_values(B)


def test_hot_bins(B):
    S.check_hot_bins(B)


def test_window_hook(B):
    """YTTM_IDCOUNT_WINDOW in {0, 1, 64, 599, 600, 601, unset} on 600 bins: the same counts"""
    S.check_window_hook(B)


def test_window_built(B):
    S.check_window_built(B)


def test_accumulate_and_exits(B):
    S.check_accumulate(B)


@pytest.mark.parametrize("name", S.all_models())
def test_pending_golden_models(B, name):
    S.check_pending_model(B, name)


def test_pending_parse_spans_errors(B):
    S.check_pending_misc(B)


def test_dropout(B):
    S.check_dropout(B)


def test_file_route(B, tmp_path):
    S.check_file(B, tmp_path)


def test_file_dropout(tmp_path):
    S.check_file_dropout(tmp_path)


def test_file_errors(B, tmp_path):
    S.check_file_errors(B, tmp_path)


def test_count_file_and_cli(tmp_path):
    S.check_count_file_and_cli(tmp_path)


def test_tensor_api():
    S.check_tensor_api()


def test_large_pending_batch(B):
    S.check_large_pending(B)


def test_large_array():
    S.check_large_array()
