"""The added tokens under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to first or in a fresh
random order per launch, the fibers of a workgroup resumed in reverse or random order.  The split and the ids must not depend on the schedule,
and every value the kernels pass as wave-uniform -- `covered`, the accepted matches of a step, the sub-sentence a wavefront appends -- is checked
across the wave in any order."""
import pytest

import added_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_split_on_synthetic_text(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_synthetic(S.NumpyBuf(), aligns=(5, 8))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_wired_routes(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_routes_model(S.NumpyBuf(), "readme_small")
    S.check_routes_model(S.NumpyBuf(), "mix_cov")
    S.check_dropout(S.NumpyBuf())
