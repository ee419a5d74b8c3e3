"""Device decode and the device-to-device exits of the encoder on a real MI355X: the cases of decode_checks.py with torch tensors as device
memory, against the host path yttm_decode."""
import pytest

import decode_checks as D

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return D.TorchBuf()


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
