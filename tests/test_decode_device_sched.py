"""The device decode under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED, as test_sim_schedules.py passes it):
workgroups last to first or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  The bytes must
not depend on the schedule -- the staging tile's hand-offs between lanes, the per-workgroup atomicMin of the first invalid id -- and every
value the kernels pass as wave-uniform is checked across the wave in any order."""
import pytest

import decode_checks as D

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_models(sched, monkeypatch, tmp_path):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in D.golden_names():
        D.check_golden(D.NumpyBuf(), name, tmp_path)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_random_ids(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    D.check_random(D.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_errors_and_padded(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    D.check_errors(D.NumpyBuf())
    D.check_padded(D.NumpyBuf())
