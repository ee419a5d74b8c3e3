"""SUBWORD output on the device on GPU-less machines: the UNMODIFIED product sources (k_subword.h, host_decode.cpp, host_lines.cpp) built against
the HIP emulator, where numpy arrays serve as device memory.  The cases live in subword_checks.py; test_gpu_subword.py runs the same ones on a
real MI355X."""
import pytest

import subword_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


@pytest.mark.parametrize("name", S.golden_names())
def test_golden_models(B, name):
    S.check_golden(B, name)


def test_sentence_lengths(B):
    S.check_lengths(B)


def test_unknown_runs(B):
    S.check_unknown_runs(B)


def test_long_piece(B, tmp_path):
    S.check_long_piece(B, tmp_path)


def test_groups_of_short_sentences(B):
    S.check_groups(B)


def test_sentences_that_fill_the_tile(B):
    S.check_full_tile(B)


def test_errors_and_pending_results(B):
    S.check_errors(B)


def test_dropout_against_the_formatter(B):
    S.check_dropout(B)


def test_unsplit_text(B):
    S.check_text(B)


def test_file_in_pieces(tmp_path):
    S.check_file(tmp_path, use_ref=True)


def test_file_errors_and_the_id_default(tmp_path):
    S.check_file_errors(tmp_path)


def test_command_line(tmp_path):
    S.check_cli(tmp_path)
