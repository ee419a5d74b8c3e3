"""The byte fallback under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to first or in a fresh
random order per launch, the fibers of a workgroup resumed in reverse or random order.  The ids must not depend on the schedule, and every value
the kernel passes as wave-uniform -- the step's totals, the runs of lanes of a step that does not fit the tile, the run directory's window --
is checked across the wave in any order."""
import pytest

import bytefb_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_pass_on_synthetic_ids_and_text(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_synthetic(S.NumpyBuf(), shifts=(0, 5), aligns=(3, 8))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_wired_routes(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_routes_model(S.NumpyBuf(), "readme_small")
    S.check_routes_model(S.NumpyBuf(), "mix_cov")
    S.check_dropout(S.NumpyBuf())
