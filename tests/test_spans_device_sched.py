"""Byte spans on the device under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to first or in a
fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  The spans must not depend on the schedule, and
every value the kernel passes as wave-uniform -- the step's masks, the carries across the steps -- is checked across the wave in any order."""
import pytest

import spans_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_models(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in S.golden_names():
        S.check_golden(S.NumpyBuf(), name)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_step_boundaries_and_spaces(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_step_boundaries(S.NumpyBuf())
    S.check_spaces_and_invalid(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_groups_and_forms(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_groups(S.NumpyBuf())
    S.check_api_forms(S.NumpyBuf())
