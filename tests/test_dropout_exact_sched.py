"""The exact dropout checks under emulator schedules other than the default one (HIPSIM_SCHED, as test_decode_device_sched.py passes it), on a
reduced case list: the ids must not depend on the order in which workgroups run or the lanes of a wave are resumed -- the word counter the lanes
of a pack take their words from, the event queues side by side in LDS."""
import pytest

import dropout_checks as DC

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_models(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    for name in ("readme_small", "manual_ru", "manual_ja", "mix_cov", "nopad"):
        DC.check_golden_model(name, ps=(0.1, 0.9), flags=((0, 0, 0), (1, 1, 1)))


@pytest.mark.parametrize("sched", SCHEDULES)
def test_shapes_under_path_hooks(sched, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    DC.check_shapes_under_hooks(ps=(0.5,), rows=(2, 4, 6, 8, 11, 14), big=False)

