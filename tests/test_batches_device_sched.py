"""Batches by length under a token budget under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups last to
first or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  No kernel of k_batches.h waits for
another workgroup; where a sentence lands in a pass of the sort depends on the scan of the tiles' counts and on its place in its tile only, and
the wavefronts of a tile take their turns whatever order their threads reach the barriers in.  On the commit before this feature every test
here fails: the library lacks the yttm_batches_* symbols."""
import pytest

import batches_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_sizes(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_sizes(S.NumpyBuf(), (65, 257, 5000))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_stability(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_stability(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_orbit(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_orbit(S.NumpyBuf(), big=False)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_model(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_pending_model(S.NumpyBuf(), "readme_small")
