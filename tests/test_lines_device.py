"""The line split and the encoder's entries for unsplit text on GPU-less machines: the UNMODIFIED product sources (k_lines.h, host_lines.cpp) built
against the HIP emulator, where numpy arrays serve as device memory.  The cases live in lines_checks.py; test_gpu_lines.py runs the same
ones on a real MI355X."""
import pytest

import lines_checks as K

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return K.NumpyBuf()


def test_split_cases_at_every_alignment(B):
    K.check_split_cases(K.core_of("readme_small"), B)


def test_split_long_line_and_many_lines(B):
    K.check_split_large(K.core_of("readme_small"), B)


@pytest.mark.parametrize("name", K.golden_names())
def test_golden_texts(B, name):
    K.check_golden(B, name)


def test_invalid_utf8_and_empty_lines(B):
    K.check_odd_texts(B)


def test_errors(B):
    K.check_errors(B)


def test_padded_hand_over_and_round_trip(B):
    K.check_padded_and_round_trip(B)


def test_word_cache_modes(B):
    K.check_cache_modes(B)


def test_dropout_of_every_merge(B):
    K.check_dropout_all(B)


def test_dropout_distribution(B):
    K.check_dropout_distribution(B)


@pytest.mark.parametrize("name", K.golden_names())
def test_file_in_pieces(name, tmp_path):
    K.check_file(name, tmp_path)


def test_file_edges_and_errors(tmp_path):
    K.check_file_edges(tmp_path)


def test_file_write_failure_releases_the_lanes(tmp_path):
    K.check_file_write_failure(tmp_path)


def test_command_line(tmp_path):
    K.check_cli(tmp_path)
