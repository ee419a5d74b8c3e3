"""BPE-dropout on a real MI355X, exact: the cases of dropout_checks.py (sized so that the file stays near half a minute: the oracle's passes
are most of it), then what only the GPU can take: a model of 40 000 tokens and 200 000 sentences in one pass -- every id equal to the
oracle's under the keyed draws."""
import pytest

import decode_checks as D
import dropout_checks as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings its own HIP runtime: it finds the GPU only if it initialises before the library's runtime does (run by itself this file
    would otherwise reach torch first in test_entry_points, after dozens of encodes)"""
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", DC.golden_model_names())
def test_golden_models(name):
    DC.check_golden_model(name)


@pytest.mark.parametrize("ki", range(len(DC.LAYOUT_KINDS)))
@pytest.mark.parametrize("li", range(len(DC.LAYOUTS)))
def test_special_id_layouts(li, ki, tmp_path):
    DC.check_layout(tmp_path, li, ki)


def test_shapes_under_every_path_hook():
    DC.check_shapes_under_hooks()


def test_entry_points(tmp_path):
    DC.check_entry_points(D.TorchBuf(), tmp_path, torch_routes=True)



def test_vocab_40000(tmp_path):
    DC.check_large_vocab(tmp_path)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_at_scale_200k_sentences(p, tmp_path):
    differ = DC.check_at_scale(tmp_path, p)
    print(f"dropout p={p}: 200000 sentences exact; at least {differ} differ from the deterministic ids")
