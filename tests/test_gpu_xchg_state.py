"""The sharded merge loop's per-round delta exchange, state by state, on the MI355X: the rows of tests/test_xchg_state.py (what is asserted
after every round on every rank: tests/xchg_checks.py) with the grids the launchers pick themselves, in worlds of two, three and four ranks --
threads of this process with one context and one stream each, on one GPU -- and test_zz_four_ranks_zipf: a text of hundreds of workgroups a
rank, so that real waves race for the slots of the delta table (dt_add) while four streams share the process's hardware queues."""
import pytest

import gen
import xchg_checks as X

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", (2, 3, 4))
@pytest.mark.parametrize("row,variant", X.cases())
def test_xchg_state(row, variant, world, monkeypatch):
    X.run_row(monkeypatch, row, variant, world, small_grids=False)


@pytest.fixture(scope="module")
def zipf_text():
    return gen.zipf_corpus(1_500_000, seed=5, vocab=30000)


@pytest.mark.parametrize("words", ["tiles", "words"])
def test_zz_four_ranks_zipf(words, zipf_text, monkeypatch):
    """120 rounds of 1.5 MB of Zipf text over four ranks, every round checked on every rank: workgroups on every XCD claim and fill the
    records of a round's send block while the other ranks' kernels run beside them; word mode left to the library (it stays off at this
    size), and forced"""
    import round_checks as R
    if words == "words":
        R.set_config(monkeypatch, "default", small_grids=False)
    shards = X.split_like_the_reference(zipf_text, 4)
    results, account = X.run_world(shards, zipf_text, monkeypatch=monkeypatch, rounds=120, target=64)
    for r in results:
        assert r["rounds"] == 120 and r["fused_rounds"] >= 110, r
        assert (r["word_rounds"] == 0) if words == "tiles" else (r["checked_word_rounds"] >= 100), r
    assert account["rounds"] == 120 and account["shared_rounds"] >= 110 and account["made_and_destroyed"] == 0, account
