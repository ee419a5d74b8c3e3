"""Encode under a restricted vocabulary on GPU-less machines: the UNMODIFIED product sources (k_restrict.h, host_encoder.cpp) built against the
HIP emulator, where numpy arrays serve as device memory.  The cases live in restrict_checks.py; test_gpu_restrict.py runs the same ones on a
real MI355X.  The yardsticks: the rule as a Python recursion over the model file's rules, applied to the unrestricted ids of the same call, and
the properties (same decoded text, only allowed ids or leaves, idempotent)."""
import pytest

import restrict_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


def test_pass_on_synthetic_ids(B):
    S.check_synthetic(B)


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
