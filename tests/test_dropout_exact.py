"""BPE-dropout on GPU-less machines, exact: the UNMODIFIED k_encode.hip built against the HIP emulator gives, id for id, what the oracle's
restatement of the reference's DropoutQueue process gives when both draw the keyed draws (dropout_checks.py; test_gpu_dropout.py runs the same
cases, larger, on a real MI355X) -- and the keyed draw stream by itself, which needs no emulator: uniform, and independent across draws, words
and sentences.  The two together are the distribution match with the reference."""
import pytest

import decode_checks as D
import dropout_checks as DC

sim = pytest.mark.usefixtures("sim_lib")


# ---- the draw stream (CPU only) ----------------------------------------------------------------------------------------------------------
def test_draw_function_is_the_documented_one():
    DC.check_draw_function()


@pytest.mark.parametrize("salt", DC.STREAM_SALTS)
def test_draw_stream_uniform_and_independent(salt):
    print(DC.check_stream(salt))


# ---- the kernel against the oracle -------------------------------------------------------------------------------------------------------
@sim
@pytest.mark.parametrize("name", DC.golden_model_names())
def test_golden_models(name):
    DC.check_golden_model(name)


@sim
@pytest.mark.parametrize("ki", range(len(DC.LAYOUT_KINDS)))
@pytest.mark.parametrize("li", range(len(DC.LAYOUTS)))
def test_special_id_layouts(li, ki, tmp_path):
    DC.check_layout(tmp_path, li, ki)


@sim
def test_shapes_under_every_path_hook():
    DC.check_shapes_under_hooks()


@sim
def test_entry_points(tmp_path):
    DC.check_entry_points(D.NumpyBuf(), tmp_path)

