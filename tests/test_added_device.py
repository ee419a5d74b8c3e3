"""The added tokens on GPU-less machines: the UNMODIFIED product sources (k_added.h, host_encoder.cpp, host_decode.cpp) built against the HIP
emulator, where numpy arrays serve as device memory.  The cases live in added_checks.py; test_gpu_added.py runs the same ones on a real MI355X.
The yardsticks: the matcher as the loop of the rule in Python over bytes, the join as list concatenation over the setting-off encode of every
segment, and the properties of the result (decode, the id ranges, idempotence, the skip without a match)."""
import pytest

import added_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


def test_split_on_synthetic_text(B):
    S.check_synthetic(B)


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
