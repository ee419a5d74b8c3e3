"""Token frequencies on the device under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to first
or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  The counts are integer sums and must not
depend on the schedule; the ballots of the wave-combine are checked across the wave in any order."""
import pytest

import idcount_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_sizes_and_edge_values(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_sizes(S.NumpyBuf(), shifts=(0, 3), big=40_000)
    S.check_edge_values(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_hot_bins_and_windows(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_hot_bins(S.NumpyBuf(), big=40_000)
    S.check_window_hook(S.NumpyBuf(), n=10_000)  # YTTM_IDCOUNT_WINDOW
    S.check_window_built(S.NumpyBuf(), n=10_000)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_model(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_pending_model(S.NumpyBuf(), "readme_small")
    S.check_accumulate(S.NumpyBuf())
