"""Device decode and the device-to-device exits of the encoder on GPU-less machines: the UNMODIFIED product sources (k_decode.h, host_decode.cpp)
built against the HIP emulator, where numpy arrays serve as device memory.  The cases live in decode_checks.py; test_gpu_decode.py runs the
same ones on a real MI355X."""
import pytest

import decode_checks as D

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return D.NumpyBuf()


@pytest.mark.parametrize("name", D.golden_names())
def test_golden_models(B, name, tmp_path):
    D.check_golden(B, name, tmp_path)


def test_random_ids(B):
    D.check_random(B)


def test_strip_rule(B):
    D.check_strip_rule(B)


def test_errors(B):
    D.check_errors(B)


def test_long_pieces(B, tmp_path):
    D.check_long_pieces(B, tmp_path)


def test_padded_form(B):
    D.check_padded(B)


def test_encode_copy_device_and_padded(B):
    D.check_encode_copies(B)


def test_empty_batch(B):
    D.check_empty_batch(B)


def test_round_trip(B):
    D.check_round_trip(B)
