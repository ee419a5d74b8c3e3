"""Training blocks on the device under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to first or in
a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  No kernel of k_blocks.h waits for another
workgroup, and the pointer doubling of the orbit pass must not depend on the order in which a workgroup's threads reach its barriers."""
import pytest

import blocks_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_seq_lens(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_lengths(S.NumpyBuf(), (2, 65, 1000))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_orbit_and_calls(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_orbit_skip(S.NumpyBuf())
    S.check_split_calls(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_model(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_pending_model(S.NumpyBuf(), "readme_small")
    S.check_boundaries(S.NumpyBuf())
