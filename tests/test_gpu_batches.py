"""Batches by length under a token budget on a real MI355X: the cases of batches_checks.py with torch tensors as device memory, against the rule
written as Python loops and against the array properties; plus the tensor API, the input ids at all sixteen element offsets and one larger pass.
On the commit before this feature every test here fails: the library lacks the yttm_batches_* symbols."""
import pytest

import batches_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B():
    return S.TorchBuf()


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
    S.check_orbit(B)


def test_gather_every_alignment(B):
    S.check_gather(B, shifts=tuple(range(16)))


def test_slot_and_exits(B):
    S.check_slot(B)


@pytest.mark.parametrize("name", S.all_models())
def test_pending_golden_models(B, name):
    S.check_pending_model(B, name)


def test_pending_parse_restricted_empty(B):
    S.check_pending_misc(B)


def test_dropout(B):
    S.check_dropout(B)


def test_tensor_api():
    S.check_tensor_api()


def test_large_batch(B):
    S.check_large(B)
