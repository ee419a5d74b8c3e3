"""Token frequencies on the device on GPU-less machines: the UNMODIFIED product sources (k_idcount.h, host_decode.cpp, host_lines.cpp) built
against the HIP emulator, where numpy arrays serve as device memory.  The cases live in idcount_checks.py; test_gpu_idcount.py runs the same
ones on a real MI355X.  The window's edges are moved inside a 600-bin histogram with YTTM_IDCOUNT_WINDOW (idcount_checks.window)."""
import pytest

import idcount_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


def test_sizes_and_alignment(B):
    S.check_sizes(B)


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
