"""The kernel-level oracle checks again, under emulator schedules other than the default one (tests/hipsim, HIPSIM_SCHED): workgroups
run last to first or in a fresh random order on every launch, and the fibers of a workgroup are resumed in reverse or random order on
every scheduling pass (every value passed as wave-uniform -- readfirstlane, inverse_ballot -- is checked across the wave in any order).  A
result that depends on dispatch order -- a ticketed tail that assumes the last workgroup is grid-1, a missing barrier between a write and a
read of LDS -- fails here while the default order passes."""
import ctypes as C
import filecmp
import json
import random

import pytest

import gen
import oracle_lib as O
import round_checks as R
import stage_checks as S
import xchg_checks as X

pytestmark = pytest.mark.usefixtures("sim_lib")

SCHEDULES = ["desc/desc", "shuffle:1", "shuffle:2"]
WORD_MODE = {"YTTM_WORD_MIN_TILES": "0", "YTTM_WORD_MIN_TOKENS": "0", "YTTM_WORD_DIV": "0", "YTTM_WORDS_GRID": "3", "YTTM_WGATHER_GRID": "2"}


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _train(text, vocab, tmp_path, tag):
    """the C ABI's file -> model training: (model path, report)"""
    from youtokentome_amd import _lib
    L = _lib.load()
    corpus, model = str(tmp_path / f"{tag}.txt"), str(tmp_path / f"{tag}.model")
    open(corpus, "wb").write(text)
    err, rep = C.create_string_buffer(2048), C.create_string_buffer(16384)
    assert L.yttm_train_bpe_ex(corpus.encode(), model.encode(), vocab, 1.0, 1, 0, 1, 2, 3, 0, rep, 16384, err, 2048) == 0, err.value
    return model, json.loads(rep.value.decode())


@pytest.mark.parametrize("sched", SCHEDULES)
def test_front_end_and_pair_count(sched, monkeypatch):
    """K1 (char histogram), K2 (word table) and K3 (pair count): the small-alphabet kernels, the general tile kernel, radix partition"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    rng = random.Random(7)
    for t in S.texts_small(0, n=2, size=1500) + [S.three_byte_text(rng, 5000)]:
        S.check_char_hist(t)
    for t in S.texts_by_alphabet_size(sizes=(2, 5, 33, 64, 70), n_words=300):
        S.check_word_table_and_pairs(t)
    monkeypatch.setenv("YTTM_K3_RADIX_MIN", "0")
    for t in S.texts_by_alphabet_size(sizes=(66, 300, 1500), n_words=300):
        S.check_word_table_and_pairs(t)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_merge_apply(sched, monkeypatch):
    """K4 (tile merge rounds: run, site placement, the measurement pass) and its delta tail"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_merge_rounds(S.texts_small(2, n=1, size=1500)[0], rounds=5, seed=1)
    words = ["ab" * k for k in range(60, 125, 13)] + ["a" * k for k in range(150, 250, 29)]
    S.check_merge_rounds((" ".join(words) + " ").encode(), rounds=5, seed=4)
    S.check_merge_rounds(S.texts_small(5, n=1, size=1200)[0], rounds=4, seed=1, id_shift=40000)
    S.check_site_placements(trials=12, seed=8)
    S.check_k4_measure(gen.readme_corpus(60, 100, seed=4), rounds=5, seed=2)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_word_mode(sched, tmp_path, monkeypatch):
    """word mode forced on: one launch per round (k_words<FUSED>), k_wgather + k_words + k_delta_apply, record regions and a record log that
    overflow; a batch of hundreds of disjoint pairs cut in two -- the oracle's models"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    _setenv(monkeypatch, WORD_MODE)
    text = gen.readme_corpus(120, 90, seed=8)
    for cfg in ({}, {"YTTM_WORDS_FUSE_MAX": "0"}, {"YTTM_WORD_LOG": "300", "YTTM_WORD_DREC": "16"},
                {"YTTM_WORDS_FUSE_MAX": "0", "YTTM_WORDS_INLINE_MAX": "0", "YTTM_WORD_DREC": "16"}):
        _setenv(monkeypatch, cfg)
        S.check_train_vs_oracle(text, 400, tmp_path, tag="wm")
        for k in cfg:
            monkeypatch.delenv(k)
    S.check_train_vs_oracle(gen.disjoint_words_corpus(150), 4 + 600 + 375, tmp_path, tag="wmsplit")


@pytest.mark.parametrize("sched", SCHEDULES)
def test_word_mode_round_state(sched, monkeypatch):
    """word-mode rounds with the candidate scan in their tail, the whole state against the oracle after every round (tests/round_checks.py):
    ordinary class-A rounds, and class-B tiles launched before k_words"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    R.run_scenario(monkeypatch, "a", "default", rounds=20)
    R.run_scenario(monkeypatch, "c", "default", rounds=20)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_multi_rank_exchange_round_state(sched, monkeypatch):
    """two and three ranks' per-round delta exchange, every rank's state against the oracle after every round (tests/xchg_checks.py), where the
    order of workgroups and lanes matters most: dt_add's claim of a slot and publication of its record number, the fold's appends to the
    lists -- blocks too small and the notes overflowed (a repeat behind a walk over every block), tiny lists over mirrored shards, and class-C
    words on one rank"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    X.run_row(monkeypatch, "notes", "with_repeats", 2, rounds=20)
    X.run_row(monkeypatch, "mirrored", "tiny_lists", 3)  # (all its rounds: the crossings by the ranks' sum are a few in forty)
    X.run_row(monkeypatch, "giant", "small_blocks", 2, rounds=20)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_encode(sched, monkeypatch):
    """K5: the word cache, sentences of every shape, dropout's heap against its array"""
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_encode_word_cache(n_sent=40)
    S.check_encode_mixed_shapes(n_sent=50)
    S.check_dropout_heap_equals_array()


@pytest.mark.parametrize("sched", SCHEDULES)
def test_golden_train(sched, tmp_path, monkeypatch):
    monkeypatch.setenv("HIPSIM_SCHED", sched)
    S.check_golden_train("mix_cov", tmp_path)


# integer report keys that describe the layout, not the algorithm (the seconds and per-kernel times are not integers: left out anyway)
NOT_ALGORITHMIC = {
    "touched_tiles",  # tiles with a merge site, summed over rounds: words are dealt into tiles in word-table slot order, and which slot a
    "touched_tile_tokens",  # word takes on a hash collision depends on the order of the inserts (the same words, the same merges)
}


def test_schedule_does_not_change_the_result(tmp_path, monkeypatch):
    """The same corpora trained under asc, desc and shuffle:1 (word mode forced on one of them): byte-identical models, equal to the oracle's,
    and equal counters in the report -- the number of rounds, word-mode rounds, index builds, list rebuilds and overflows must not depend on
    the order in which workgroups and lanes ran."""
    rng = random.Random(11)
    cases = [(gen.readme_corpus(100, 90, seed=21), 300, {}), (gen.unicode_text(rng, 6000, "mix"), 200, {}),
             (gen.zipf_corpus(30000, vocab=800, seed=3), 300, WORD_MODE)]
    for i, (text, vocab, env) in enumerate(cases):
        O.train(text, str(tmp_path / f"o{i}.model"), vocab)
        reports = {}
        for sched in ("asc/asc", "desc/desc", "shuffle:1"):
            monkeypatch.setenv("HIPSIM_SCHED", sched)
            _setenv(monkeypatch, env)
            model, rep = _train(text, vocab, tmp_path, f"c{i}_{sched.replace('/', '_').replace(':', '_')}")
            assert filecmp.cmp(model, str(tmp_path / f"o{i}.model"), shallow=False), (i, sched)
            reports[sched] = {k: v for k, v in rep.items() if isinstance(v, int) and k not in NOT_ALGORITHMIC}
        if env:
            assert reports["asc/asc"]["word_rounds"] > 0, reports["asc/asc"]
        for sched in ("desc/desc", "shuffle:1"):
            diff = {k: (reports["asc/asc"][k], reports[sched].get(k)) for k in reports["asc/asc"] if reports["asc/asc"][k] != reports[sched].get(k)}
            assert not diff, (i, sched, diff)
