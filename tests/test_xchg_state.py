"""The sharded merge loop's per-round delta exchange, state by state, on GPU-less machines (the product sources on the HIP emulator): worlds
of two and three ranks -- threads of this process, one context and one host-callback communicator each -- run the trainer's round protocol,
and after EVERY round every rank's words, its replica of the pair table, its candidates (the same on every rank) and the pick are held to the
oracle (tests/xchg_checks.py says what is asserted, how the ranks meet and what each row is there to reach).  One test per scenario row,
parametrised over its variants and the world; each proves its path from the ranks' counters and the oracle's account of the rounds
(xchg_checks.assert_row).  The same rows with the launchers' own grids, and worlds of up to four, on the MI355X: tests/test_gpu_xchg_state.py."""
import pytest

import xchg_checks as X

pytestmark = pytest.mark.usefixtures("sim_lib")

WORLDS = (2, 3)


def _variants(row):
    return tuple(X.ROWS[row][2])


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("variant", _variants("ordinary"))
def test_ordinary_text(variant, world, monkeypatch):
    """(1) ordinary text cut like the reference cuts it: rounds on tiles, then word mode, the scan in the fold's tail on every rank; once
    through yttm_gpu_merge_apply (no counts: blocks sized by the bound, the scan a launch of its own), and once with hooks of its own on
    one rank (that rank's word rounds in three launches, the others' in one)"""
    X.run_row(monkeypatch, "ordinary", variant, world)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("variant", _variants("repeat"))
def test_blocks_too_small_are_repeated(variant, world, monkeypatch):
    """(2) blocks too small in most rounds: settle_exchange repeats the exchange for the skipped ranks (only_mask), nothing is applied twice,
    the scan that came too early is made again; with the lists' own sizes and with tiny hot and top lists"""
    X.run_row(monkeypatch, "repeat", variant, world)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("variant", _variants("notes"))
def test_notes_overflow_walks_every_block(variant, world, monkeypatch):
    """(3) two notes: the fold walks every rank's block, this rank's included; with repeats, the walk must come again behind the repeat"""
    X.run_row(monkeypatch, "notes", variant, world)


@pytest.mark.parametrize("world", WORLDS)
def test_class_c_words_on_one_rank(world, monkeypatch):
    """(4) words of 2100 .. 3000 chars on rank 0 only (k_giant.hip takes back every old adjacency of a tile it counts anew, the merged pairs
    included), blocks too small: the deltas that arrive with the repeat land on pairs the early scan had zeroed -- zeroed again"""
    X.run_row(monkeypatch, "giant", "small_blocks", world)


@pytest.mark.parametrize("world", WORLDS)
def test_class_b_words_and_runs_on_different_ranks(world, monkeypatch):
    """(5) class-B words on rank 0, x == y rules and runs on rank 1"""
    X.run_row(monkeypatch, "classb_and_runs", "scan", world)


@pytest.mark.parametrize("world", WORLDS)
def test_a_rank_without_words_and_a_rank_of_one_tile(world, monkeypatch):
    """(6) a rank of white space sends a header every round and takes every batch; the switch to word mode is one decision (the sums over
    the headers), taken in the same round by ranks of many tiles, of one tile and of none"""
    X.run_row(monkeypatch, "blank_and_few", "scan", world)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("variant", _variants("mirrored"))
def test_thresholds_crossed_by_the_sum_of_the_ranks(variant, world, monkeypatch):
    """(7) mirrored shards over two letters: pairs reach a threshold by the ranks' sum where no rank's own adds do (shown from the oracle's
    shard tables); every rank lists the same slots, round by round, with the lists' own sizes and with tiny ones"""
    X.run_row(monkeypatch, "mirrored", variant, world)


@pytest.mark.parametrize("world", WORLDS)
def test_radix_pair_count_travels_through_the_set_up_exchange(world, monkeypatch):
    """(8) K3 by radix partition on 300 symbols: k3r_final's records through exchange_deltas (comm_plan.h's offsets); the replica is held to
    the oracle before the first round"""
    X.run_row(monkeypatch, "radix", "scan", world)
