"""Byte spans on the device on GPU-less machines: the UNMODIFIED product sources (k_spans.h, host_decode.cpp, host_lines.cpp) built against the
HIP emulator, where numpy arrays serve as device memory.  The cases live in spans_checks.py; test_gpu_spans.py runs the same ones on a real
MI355X."""
import pytest

import spans_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


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


def test_groups_of_short_sentences(B):
    S.check_groups(B)


def test_api_forms(B):
    S.check_api_forms(B)


def test_errors_and_pending_results(B):
    S.check_errors(B)
