"""The line split under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED, as test_sim_schedules.py passes it):
workgroups last to first or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  Offsets, ids
and the longest line must not depend on the schedule -- the per-tile counts, the ranks handed through LDS, the per-workgroup atomicMax."""
import pytest

import lines_checks as K

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_split_cases(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    K.check_split_cases(K.core_of("readme_small"), K.NumpyBuf(), aligns=(0, 5, 15))
    K.check_split_large(K.core_of("readme_small"), K.NumpyBuf(), aligns=(11,), big=(1 << 20) + 77)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_texts(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in K.golden_names():
        K.check_golden(K.NumpyBuf(), name)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_odd_texts_and_file(sched, monkeypatch, tmp_path):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    K.check_odd_texts(K.NumpyBuf(), names=("manual_ru",))
    K.check_file("readme_small", tmp_path, flags=((1, 1, 1),))
