"""The pair index built by radix partition of its postings, on GPU-less machines (the product sources on the HIP emulator): what the index
holds against the word table it was built from, the radix build (YTTM_INDEX_RADIX_MIN=0) against the streaming build (a huge
YTTM_INDEX_RADIX_MIN) on the same states, and the word-mode rounds state
by state with the radix build forced (tests/index_radix_checks.py says what is asserted).  The same on the MI355X: tests/test_gpu_index_radix.py."""
import pytest

import gen
import index_radix_checks as X
import round_checks as R

pytestmark = pytest.mark.usefixtures("sim_lib")


def test_index_right_after_the_switch(monkeypatch):
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0])
    assert builds[0] is not None and st["index_radix_builds"] == 1, st


def test_index_of_words_with_holes(monkeypatch):
    """a second build after at least ten word-mode rounds: the words have shrunk in place"""
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0], env=X.TINY_LISTS, want_builds=2, min_word_rounds=10)
    assert len(builds) >= 2 and builds[-1] is not None and st["word_rounds"] >= 10 and st["index_radix_builds"] >= 2, st


def test_index_of_runs_and_self_pairs(monkeypatch):
    """runs, x == x pairs, and one key that holds most postings"""
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_b()[0])
    assert builds[0] is not None and st["index_radix_builds"] == 1, st
    keys = builds[0][0]
    assert ((keys >> 32) == (keys & X.MX_ALL)).any(), "no x == x pair among the keys"


def test_index_of_many_keys(monkeypatch):
    """Zipf text of several class-A tiles: more than 256 keys, so level-1 groups hold several slots (a build of this size is cut into chunks
    of 256 records: the frequent keys' groups are several work items)"""
    builds, st, _ = X.both_builds(monkeypatch, gen.zipf_corpus(120000, vocab=3000))
    assert builds[0] is not None and st["index_radix_builds"] == 1, st
    keys, pairs, _ = builds[0]
    assert len(keys) > 256 and len(pairs) > 256 * 4, (len(keys), len(pairs))


def test_no_postings_leaves_the_index_invalid(monkeypatch):
    """a hot list whose pairs occur only in class-B words"""
    builds, st, st_old = X.both_builds(monkeypatch, X.text_only_class_b_pairs(), env=X.ONLY_B_ENV, max_rounds=6)
    assert builds and builds[0] is None, "the index holds postings: the text does not reach the case"
    assert st["index_builds"] >= 1 and st["index_radix_builds"] == 0, st


def test_falls_back_without_room_for_the_records(monkeypatch):
    """the free HBM the context believes in does not hold the radix build's buffers: the streaming build, the same index"""
    builds, st, _ = X.both_builds(monkeypatch, R.corpus_a()[0], radix_env={"YTTM_TEST_FREE_BYTES": 32 << 20})
    assert builds[0] is not None and st["index_builds"] >= 1 and st["index_radix_builds"] == 0, st


@pytest.mark.parametrize("corpus,config", [("a", "default"), ("a", "tiny_lists"), ("b", "default"), ("c", "tiny_lists"), ("g", "tiny_lists")])
def test_round_state_with_the_radix_build(corpus, config, monkeypatch):
    X.scenario(monkeypatch, corpus, config, small_grids=True)
