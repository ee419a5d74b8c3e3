"""SUBWORD output on the device under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED, as test_sim_schedules.py passes
it): workgroups last to first or in a fresh random order per launch, the fibers of a workgroup resumed in reverse or random order.  The bytes
must not depend on the schedule -- the staging tile's hand-offs between lanes, the run directory's LDS atomics, the groups' shared 16-byte
units -- and every value the kernels pass as wave-uniform is checked across the wave in any order."""
import pytest

import subword_checks as S

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_models(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in S.golden_names():
        S.check_golden(S.NumpyBuf(), name)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_unknown_runs_and_lengths(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_unknown_runs(S.NumpyBuf())
    S.check_lengths(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_groups_and_text(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_groups(S.NumpyBuf())
    S.check_text(S.NumpyBuf())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_long_piece_beside_busy_waves(sched, monkeypatch, tmp_path):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    bpe, word, fmt = S.long_model(tmp_path)
    S.check_long_neighbours(S.NumpyBuf(), bpe, word, fmt, flags=((0, 0, 0), (1, 1, 1)))
