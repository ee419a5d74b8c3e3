"""Decimal id text on the device under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED, as test_sim_schedules.py passes
it): workgroups last to first or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  The ids and
the bytes must not depend on the schedule -- the carries across the parser's steps, the staging tile's hand-offs between lanes, the newline
counts of the decode's LDS atomics, the groups' shared 16-byte units -- and every value the kernels pass as wave-uniform is checked across the
wave in any order."""
import pytest

import idtext_checks as T

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_signs_fail_points_and_range(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    T.check_signs(T.NumpyBuf(), (0, 9))
    T.check_fail_points(T.NumpyBuf(), (3, 15))
    T.check_range(T.NumpyBuf(), (0, 7))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_steps(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    T.check_steps(T.NumpyBuf(), (0, 5, 10, 15), range(48, 131))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_groups_and_digit_counts(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    T.check_groups(T.NumpyBuf(), (0, 13), big=20_000)
    T.check_digit_counts(T.NumpyBuf(), (0, 6))
    T.check_soup(T.NumpyBuf(), (2,), n_lines=3000)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_models(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in T.golden_names():
        T.check_golden(T.NumpyBuf(), name)
