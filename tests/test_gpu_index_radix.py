"""The pair index built by radix partition of its postings, on the MI355X with the launchers' own grids: the checks of
tests/test_index_radix.py (YTTM_INDEX_RADIX_MIN=0 against a huge value; what is asserted: tests/index_radix_checks.py) and the same on 2 MB of Zipf text -- some three hundred class-A
tiles, workgroups on every XCD and more workgroups than level-1 groups."""
import pytest

import gen
import index_radix_checks as X
import round_checks as R

pytestmark = pytest.mark.gpu


def test_index_right_after_the_switch(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0])
    assert builds[0] is not None and st["index_radix_builds"] == 1, st


def test_index_of_words_with_holes(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0], env=X.TINY_LISTS, want_builds=2, min_word_rounds=10)
    assert len(builds) >= 2 and builds[-1] is not None and st["word_rounds"] >= 10 and st["index_radix_builds"] >= 2, st


def test_index_of_runs_and_self_pairs(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_b()[0])
    assert builds[0] is not None and st["index_radix_builds"] == 1, st


def test_index_of_many_keys(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, gen.zipf_corpus(120000, vocab=3000))
    assert builds[0] is not None and st["index_radix_builds"] == 1 and len(builds[0][0]) > 256, st


@pytest.fixture(scope="module")
def zipf_2mb():
    return gen.zipf_corpus(2_000_000, seed=3, vocab=30000)


def test_index_of_many_tiles(zipf_2mb, monkeypatch):
    """2 MB of Zipf text under the lists' own sizes: a build of enough postings for the large chunks"""
    builds, st, _ = X.both_builds(monkeypatch, zipf_2mb)
    assert builds[0] is not None and st["index_radix_builds"] == 1, st
    assert builds[0][2] >= 1 << 16, f"{builds[0][2]} postings: fewer than the large chunks are used from"


def test_index_of_many_tiles_with_holes(zipf_2mb, monkeypatch):
    """the same text under the tiny lists: a second build after at least ten word-mode rounds"""
    builds, st, _ = X.both_builds(monkeypatch, zipf_2mb, env=X.TINY_LISTS, want_builds=2, min_word_rounds=10)
    assert len(builds) >= 2 and builds[0] is not None and builds[-1] is not None and st["word_rounds"] >= 10 and st["index_radix_builds"] >= 2, st


def test_no_postings_leaves_the_index_invalid(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, X.text_only_class_b_pairs(), env=X.ONLY_B_ENV, max_rounds=6)
    assert builds and builds[0] is None, "the index holds postings: the text does not reach the case"
    assert st["index_builds"] >= 1 and st["index_radix_builds"] == 0, st


def test_falls_back_without_room_for_the_records(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0], radix_env={"YTTM_TEST_FREE_BYTES": 32 << 20})
    assert builds[0] is not None and st["index_builds"] >= 1 and st["index_radix_builds"] == 0, st


@pytest.mark.parametrize("corpus,config", [("a", "tiny_lists"), ("g", "tiny_lists"), ("b", "default")])
def test_round_state_with_the_radix_build(corpus, config, monkeypatch):
    X.scenario(monkeypatch, corpus, config, small_grids=False)
