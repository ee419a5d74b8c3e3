"""Word-mode merge rounds and the candidate filter, state by state, on the MI355X: the checks of tests/test_round_state.py (what is asserted
after every round: tests/round_checks.py) with the grids the launchers pick themselves, and test_zz_fused_tail_state -- the ordering argument
of a fused tail (k_merge_shared.h, F1 - F4) held to the oracle's counts round by round, on a corpus of hundreds of workgroups."""
import pytest

import gen
import round_checks as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("corpus,config", R.cases())
def test_round_state(corpus, config, monkeypatch):
    R.run_scenario(monkeypatch, corpus, config, small_grids=False)


@pytest.fixture(scope="module")
def zipf_2mb():
    return gen.zipf_corpus(2_000_000, seed=3, vocab=30000)


@pytest.mark.parametrize("words", ["tiles", "words", "words_unfused"])
def test_zz_fused_tail_state(words, zipf_2mb, monkeypatch):
    """200 rounds of 2 MB of Zipf text -- some three hundred class-A tiles, workgroups on every XCD -- with the candidate scan in the tail of
    every round's last launch: the tile kernels' tail (word mode left to the library: it stays off at this size), k_words<FUSED>'s (word mode
    forced), and k_delta_apply's (the same with YTTM_WORDS_FUSE_MAX=0).  A count the tail read before the store that made it arrived shows as
    a candidate whose count is not the oracle's, in the round it happened; a store the tail overtook for good, as a pair count that differs."""
    if words != "tiles":
        R.set_config(monkeypatch, "default" if words == "words" else "unfused_words", small_grids=False)
    got = R.run_rounds(zipf_2mb, rounds=200, target=64)
    assert got["rounds"] == 200 and got["fused_rounds"] >= 195, got
    if words == "tiles":
        assert got["word_rounds"] == 0, got
    else:
        assert got["checked_word_rounds"] >= 190 and (got["word_fused_rounds"] >= 190) == (words == "words"), got
