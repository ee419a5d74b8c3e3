"""Batches by length under a token budget on GPU-less machines: the UNMODIFIED product sources (k_batches.h, host_decode.cpp) built against the HIP
emulator, where numpy arrays serve as device memory.  The cases live in batches_checks.py; test_gpu_batches.py runs the same ones on a real
MI355X.  On the commit before this feature every test here fails: the library lacks the yttm_batches_* symbols."""
import pytest

import batches_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")


@pytest.fixture()
def B():
    return S.NumpyBuf()


@pytest.mark.parametrize("n", S.SIZES)
def test_every_size(B, n):
    S.check_sizes(B, (n,))


def test_stability_and_hot_digits(B):
    S.check_stability(B)


def test_digit_edges_and_pass_counts(B):
    S.check_digits(B)


def test_budget_edges_and_refusals(B):
    S.check_budget(B)


def test_filter(B):
    S.check_filter(B)


def test_orbit_jumps_over_blocks(B):
    """YTTM_BATCHES_ORBIT shrinks the block of positions a workgroup of the cuts resolves: the same plan at 64, 256, 960 and the built 8 192"""
    S.check_orbit(B)


def test_gather(B):
    S.check_gather(B)


def test_slot_and_exits(B):
    S.check_slot(B)


@pytest.mark.parametrize("name", S.all_models())
def test_pending_golden_models(B, name):
    S.check_pending_model(B, name)


def test_pending_parse_restricted_empty(B):
    S.check_pending_misc(B)


def test_dropout(B):
    S.check_dropout(B)
