"""The byte fallback on GPU-less machines: the UNMODIFIED product sources (k_bytefb.h, host_encoder.cpp, host_decode.cpp) built against the HIP
emulator, where numpy arrays serve as device memory.  The cases live in bytefb_checks.py; test_gpu_bytefb.py runs the same ones on a real
MI355X.  The yardsticks: the rule in Python -- the alphabet from the model file, the runs cut from the text, V + b spliced into the setting-off
ids of the same call -- and the round trip decode(encode(s)) == s."""
import pytest

import bytefb_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


def test_pass_on_synthetic_ids_and_text(B):
    S.check_synthetic(B)


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
