"""Decimal id text on the device on GPU-less machines: the UNMODIFIED product sources (k_idtext.h, k_decode.h, host_decode.cpp, host_lines.cpp) built
against the HIP emulator, where numpy arrays serve as device memory.  The cases live in idtext_checks.py; test_gpu_idtext.py runs the same ones on
a real MI355X, every one at every address alignment -- here the larger texts take a few of the sixteen, the emulator's time goes with the bytes."""
import pytest

import idtext_checks as T

pytestmark = pytest.mark.usefixtures("sim_lib")

FEW = (0, 5, 11, 15)


@pytest.fixture()
def B():
    return T.NumpyBuf()


def test_line_structure(B):
    T.check_line_structure(B)


def test_signs_and_glue(B):
    T.check_signs(B)


def test_fail_points(B):
    T.check_fail_points(B)


def test_int32_range_and_long_runs(B):
    T.check_range(B)


def test_steps_at_every_shift(B):
    T.check_steps(B)


def test_groups_of_lines(B):
    T.check_groups(B, FEW)


def test_random_byte_soup(B):
    T.check_soup(B, (3, 12))


@pytest.mark.parametrize("name", T.golden_names())
def test_golden_models(B, name):
    T.check_golden(B, name)


def test_every_digit_count(B):
    T.check_digit_counts(B)


def test_pending_results(B):
    T.check_pending(B)


def test_long_pieces_between_newlines(B, tmp_path):
    T.check_long_piece_lines(B, tmp_path, FEW)


def test_decode_file_in_pieces(tmp_path):
    T.check_decode_file(tmp_path, use_ref=True)


def test_id_text_file_in_pieces(tmp_path):
    T.check_idtext_file(tmp_path, use_ref=True, picks=(0, 1, 2, 3, 6, 9))


def test_file_errors(tmp_path):
    T.check_file_errors(tmp_path)


def test_command_line(tmp_path):
    T.check_cli(tmp_path)
