"""The sharded merge loop -- N ranks, one exchange of pair-count deltas per round -- driven through the stage ABI with
every rank's whole state compared with the oracle after every round.

tests/test_multi_rank_gloo.py holds this path to one thing, the finished model.  Here N stage-ABI contexts run as N ranks of ONE process,
on one GPU or on the emulator: each rank is a thread with its own context and its own host-callback communicator
(yttm_comm_callback_create), and the transport behind the two callbacks is a threading.Barrier and a list (World).  Every rank runs the
trainer's protocol exactly as round_checks.run_rounds drives it for one context -- the same function, with a Rank in the place of
round_checks.Alone -- and after EVERY candidates call asserts, bit exact (oracle/bpe_oracle.c):

  shard words       the rank's word table is the oracle's table of ITS shard with the batches applied
  replica           every pair and count of the rank's pair table is the from-scratch recount summed over ALL shards' oracle tables, the
                    applied batch's pairs at zero
  candidates        round_checks' complete-prefix checks against the global counts; and every rank got the same n and the same set -- what
                    keeps the ranks in lock step (a list that differs in length makes one rank rebuild it, in collectives the others never post)
  pick              the batch picked from the device's candidates is the oracle's

What the run reached comes back from every rank's counters (yttm_gpu_round_stats: exchange_retries, word rounds, fused rounds ...) and from
what rank 0 computes FROM THE ORACLE ALONE about every round (Rank._account): how many ranks' shards held a site of the batch, pairs made
on one rank and destroyed on another, threshold crossings that only the ranks' sum makes or that one rank makes and the sum takes back; the
rounds whose notes of possible crossings (YTTM_XCHG_NOTES) must have overflowed are told from the candidates themselves (Rank.agree).  Shared by tests/test_xchg_state.py and
tests/test_sim_schedules.py (emulator) and tests/test_gpu_xchg_state.py (MI355X)."""
import ctypes as C
import random
import threading

import numpy as np

import gen
import oracle_lib as O
import round_checks as R
from stage_lib import Ctx

# Safety cap of every wait (a barrier, a join), seconds: it ends a run whose ranks have diverged and is never waited out by a run that passes.
# Sized from the slowest run measured -- one core, emulator, three ranks, forty rounds of the mirrored shards under tiny lists: 8.1 s for the
# whole run, under the shuffled schedules 9 s; on the MI355X no run takes 3 s -- with a factor of thirty for a loaded machine.
TIMEOUT = 300.0


class Diverged(AssertionError):
    pass


class World:
    """The transport and the meeting point of `world` rank threads: a barrier and one slot per rank.  exchange(rank, value) hands every rank
    the list of all ranks' values (two barrier waits: nobody overwrites a slot somebody else still reads)."""

    def __init__(self, world, timeout=TIMEOUT):
        self.world = world
        self.timeout = timeout
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.shared = {}

    def exchange(self, rank, value):
        self.slots[rank] = value
        self.barrier.wait(self.timeout)
        got = list(self.slots)
        self.barrier.wait(self.timeout)
        return got


class CallbackComm:
    """yttm_comm_callback_create over a World: the two callbacks meet the other ranks at the barrier.  A rank that failed aborts the barrier;
    the callbacks of the others then return non-zero, which the library reports ("allgather callback failed"): every thread ends."""

    def __init__(self, L, w, rank):
        self.L, self.w, self.rank = L, w, rank

        def allreduce(user, buf, n):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(n,))
                parts = w.exchange(rank, arr.astype(np.uint64, copy=True))
                arr[:] = np.sum(np.stack(parts), axis=0, dtype=np.uint64)  # (modulo 2^64)
                return 0
            except BaseException:  # (threading.BrokenBarrierError: another rank failed, or the wait ran out)
                return 1

        def allgather(user, send, nbytes, recv, cap, out_bytes):
            try:
                parts = w.exchange(rank, C.string_at(send, nbytes) if nbytes else b"")
                blob = b"".join(parts[r] for r in range(w.world) if r != rank)  # the others' strings, in rank order
                out_bytes[0] = len(blob)
                if len(blob) <= cap:
                    C.memmove(recv, blob, len(blob))
                return 0
            except BaseException:
                return 1

        self.fns = (L.ALLREDUCE_FN(allreduce), L.ALLGATHER_FN(allgather))  # (kept alive with the communicator)
        self.h = C.c_void_p()
        assert L.yttm_comm_callback_create(rank, w.world, self.fns[0], self.fns[1], None, C.byref(self.h)) == 0

    def destroy(self):
        if self.h:
            self.L.yttm_comm_destroy(self.h)
            self.h = None


def split_like_the_reference(text, world):
    """the reference's per-thread split (bpe.cpp:864-873, as tests/mp_train_worker.py): byte i * len / world, advanced to the next ASCII space"""
    def cut(i):
        if i == 0:
            return 0
        c = len(text) * i // world
        while c < len(text) and text[c] not in b" \t\n\v\f\r":
            c += 1
        return c
    return [text[cut(r):cut(r + 1)] for r in range(world)]


def _merge_counts(parts):
    """[(keys, counts) per shard, each sorted by key] -> (xs, ys, cs) of the sum, sorted by key, zero sums left out"""
    keys = np.concatenate([k for k, _ in parts]) if parts else np.zeros(0, np.uint64)
    cnts = np.concatenate([c for _, c in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), np.int64)
    np.add.at(sums, inv, cnts)
    live = sums != 0
    uk, sums = uk[live], sums[live]
    return (uk >> np.uint64(32)).astype(np.uint32), (uk & np.uint64(R.MX_ALL)).astype(np.uint32), sums.astype(np.uint64)


def _lookup(keys, cnts, want):
    """counts of the pairs `want` in a (sorted keys, counts) table, 0 where absent; int64"""
    if len(keys) == 0:
        return np.zeros(len(want), np.int64)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return np.where(keys[pos] == want, cnts[pos].astype(np.int64), 0)


class Rank(R.Alone):
    """One rank of the world in run_rounds' terms.  Rank 0 also keeps the oracle's account of every round (self.w.shared["oracle"])."""

    def __init__(self, w, rank, ctx, shards):
        self.w, self.rank, self._ctx, self.shards = w, rank, ctx, shards
        self.prev = None  # the shards' recounts before the round that is being checked (rank 0)
        self.batch = None
        self.nxt = 0
        self.notes_cap = None  # YTTM_XCHG_NOTES of this rank's context, where a run is to prove the walk over every record
        self.fused_before = None
        self.walks = 0

    def ctx(self):
        return self._ctx

    def shard(self, text):
        return self.shards[self.rank]

    def recount(self, tok, off, cnt):
        xs, ys, cs = O.pair_counts(tok, off, cnt)  # (the oracle's functions used here keep no state: every rank's thread calls them)
        parts = self.w.exchange(self.rank, (R._keys(xs, ys), cs))
        if self.rank == 0:
            self.w.shared["recount"] = _merge_counts(parts)
            self._account(parts)
        self.w.exchange(self.rank, None)  # (rank 0's sum is there)
        return self.w.shared["recount"]

    def agree(self, what, value, where):
        if self.notes_cap is not None and self.fused_before is not None:
            # An answer from the fold's tail (fused_rounds went up in this candidates call, and neither list was rebuilt or refilled in it:
            # a fused answer that is discarded for a rebuild lists new pairs from the whole table) was read from the top list, and in a
            # multi-GPU round a slot joins a list in k_fold_list only: through a note (at most notes_cap of them are kept) or through the
            # walk over every record.  A pair with a token the batch made was on no list before: more of them among the candidates than
            # notes fit proves the walk.
            now = self._ctx.round_stats()
            fused = now["fused_rounds"] > self.fused_before[0] and (now["hot_rebuilds"], now["top_refills"]) == self.fused_before[1:]
            keys = np.frombuffer(value[1], np.uint64)
            new = int((np.maximum(keys >> np.uint64(32), keys & np.uint64(R.MX_ALL)) >= np.uint64(self.batch[0][2])).sum())
            self.walks += fused and new > self.notes_cap
            self.fused_before = None
        got = self.w.exchange(self.rank, value)
        same = [g == got[0] for g in got]
        if not all(same):
            ns = [g[0] if isinstance(g, tuple) else g for g in got]
            raise Diverged(f"the ranks differ in their {what} after {where}: rank {same.index(False)} against rank 0 ({ns})")

    def batch_picked(self, batch, nxt, lower_to, where):
        self.batch, self.nxt = batch, lower_to
        st = self._ctx.round_stats()
        self.fused_before = (st["fused_rounds"], st["hot_rebuilds"], st["top_refills"])

    # ---- the oracle's account of the round just checked (rank 0; from the shards' oracle tables alone: no device value enters) ----------
    def _account(self, parts):
        acc = self.w.shared.setdefault("oracle", dict(rounds=0, shared_rounds=0, made_and_destroyed=0, crossed_by_sum=0, crossed_and_back=0))
        prev, self.prev = self.prev, parts
        if prev is None or not self.batch:
            return
        bkeys = np.array([(x << 32) | y for x, y, _ in self.batch], np.uint64)
        holders = sum(1 for k, c in prev if _lookup(k, c, bkeys).any())  # ranks whose shard held a site of the batch
        acc["rounds"] += 1
        acc["shared_rounds"] += holders >= 2
        # every pair some shard's count of changed in the round: per-shard deltas, the global count before and after
        touched = np.unique(np.concatenate([k for k, _ in prev] + [k for k, _ in parts]))
        touched = touched[~np.isin(touched, bkeys)]
        d = np.stack([_lookup(k1, c1, touched) - _lookup(k0, c0, touched) for (k0, c0), (k1, c1) in zip(prev, parts)])  # [rank, pair]
        before = np.sum(np.stack([_lookup(k0, c0, touched) for k0, c0 in prev]), axis=0)
        after = before + d.sum(axis=0)
        acc["made_and_destroyed"] += int(((d > 0).any(axis=0) & (d < 0).any(axis=0)).sum())  # one rank's shard gained it, another's lost it
        # the threshold the next scan lists down to (the count of the target-th candidate the batch leaves over; in the rounds that first ask
        # for more than any pair has, the rescan's): where the fold's scan and, with lists as small as the target, the lists themselves cut
        t = int(self.nxt)
        up = np.maximum(d, 0)
        acc["crossed_by_sum"] += int(((before < t) & (after >= t) & (before + up.max(axis=0) < t)).sum())  # no single rank's adds get there
        acc["crossed_and_back"] += int(((before < t) & (after < t) & (before + up.max(axis=0) >= t)).sum())  # one rank's adds do, the sum does not


def run_world(shards, text=None, envs=None, monkeypatch=None, timeout=TIMEOUT, notes_cap=None, **kw):
    """`len(shards)` ranks through round_checks.run_rounds, rank r on shards[r] (`text`: what the alphabet is taken from, default the
    shards joined).  envs: per rank, environment set while THAT rank's context is created (a context snapshots its hooks at creation).
    Returns (the ranks' results, the oracle's account of the rounds)."""
    from youtokentome_amd import _lib
    L = _lib.load()
    world = len(shards)
    w = World(world, timeout)
    text = text if text is not None else b"".join(shards)
    comms, ranks = [], []
    for r in range(world):  # one after another, on this thread
        with monkeypatch.context() as m:
            for k, v in ((envs or [{}] * world)[r]).items():
                m.setenv(k, str(v))
            c = Ctx()
        comm = CallbackComm(L, w, r)
        c.set_comm(comm.h)
        comms.append(comm)
        ranks.append(Rank(w, r, c, shards))
        ranks[-1].notes_cap = notes_cap
    results, errors = [None] * world, [None] * world

    def main(r):
        try:
            results[r] = R.run_rounds(text, peer=ranks[r], **kw)
        except BaseException as e:  # noqa: the other ranks must not wait for this one
            errors[r] = e
            w.barrier.abort()

    threads = [threading.Thread(target=main, args=(r,), daemon=True, name=f"rank{r}") for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    hung = [t.name for t in threads if t.is_alive()]
    if hung:
        w.barrier.abort()
        for t in threads:
            t.join(5.0)
    # the first failure that is not the echo of another rank's (a broken barrier, a callback that gave up)
    real = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError) and "callback failed" not in str(e)]
    for r in range(world):
        if not threads[r].is_alive():
            if results[r] is None:
                ranks[r]._ctx.close()
            comms[r].destroy()
    assert not hung, f"ranks still running after {timeout} s (diverged: one waits in a collective the others never post): {hung}; first error: {real[:1] or errors}"
    if real:
        raise real[0]
    assert not any(errors), errors
    for r in range(world):
        results[r]["notes_walks_proven"] = ranks[r].walks
    return results, w.shared.get("oracle", {})


# ---- texts ---------------------------------------------------------------------------------------------------------------------------------
def text_ordinary():
    return gen.readme_corpus(160, 100, seed=3) + gen.zipf_corpus(30000, vocab=1200, seed=4)


def shards_mirrored(world, seed=2, n=1500):
    """Shards over two letters that mirror each other (round_checks.corpus_h's shape): every word of shard 0 is in shard 1 reversed with the
    letters swapped (two words in three), and in shard 2 reversed.  A dozen pairs hold nearly all the counts, each rank holds about 1 / world
    of every one of them, and every merge leaves its neighbours' pairs and the new token's pairs near the thresholds of the lists and of the
    scan: pairs get across a threshold by the SUM of the ranks' adds where no rank's own adds reach it (Rank._account counts them from the
    oracle's shard tables)."""
    rng = random.Random(seed)
    ws = ["".join(rng.choice("ab") for _ in range(rng.randint(2, 9))) for _ in range(n)]
    swap = str.maketrans("ab", "ba")
    a = " ".join(ws) + "\n"
    b = " ".join(x.translate(swap)[::-1] if i % 3 else x for i, x in enumerate(ws)) + "\n"
    c = " ".join(x[::-1] for x in ws[: n // 2]) + "\n"
    d = " ".join(x.translate(swap) for x in ws[n // 2:]) + "\n"
    return [a.encode(), b.encode(), c.encode(), d.encode()][:world]


def shards_giant_on_one_rank(world, seed=9):
    """words of 2100 .. 3000 chars (class C, k_giant.hip) on rank 0 only, short words everywhere"""
    rng = random.Random(seed)
    longs = ["".join(rng.choice("abc") for _ in range(n)) for n in (2100, 2600, 3000)]
    def short(k):
        return ["".join(rng.choice("abcd") for _ in range(rng.randint(1, 9))) for _ in range(k)]
    first = " ".join(short(150) + longs + short(150) + longs[:2]) + "\n"
    return [first.encode()] + [(" ".join(short(300)) + "\n").encode() for _ in range(world - 1)]


def shards_classb_and_runs(world):
    """class-B words on one rank, x == y rules and runs on another, ordinary words on the rest"""
    rng = random.Random(6)
    out = [R.corpus_c(seed=7)[0], R.corpus_b()[0]]
    out += [(" ".join("".join(rng.choice("abc") for _ in range(rng.randint(1, 9))) for _ in range(600)) + "\n").encode() for _ in range(world - 2)]
    return out[:world]


def shards_blank_and_few(world, seed=300):
    """Shard sets for a word-mode switch that must be one decision: ranks with many distinct words (many class-A tiles), one rank with a
    handful of words repeated (one tile), one with nothing but white space (no word at all: it still sends a header every round).  A world
    of two cannot hold all three: two sets there."""
    rng = random.Random(seed + world)
    big = b" ".join("".join(rng.choice("abcdefgh") for _ in range(rng.randint(2, 14))).encode() for _ in range(3000)) + b"\n"
    few = b"abab cdcd abcd " * 400 + b"\n"
    blank = b" \n" * 500
    if world == 2:
        return [[big, few], [blank, big]]
    return [[big] * (world - 2) + [few, blank]]


# ---- scenario rows -------------------------------------------------------------------------------------------------------------------------
REPEAT = {"YTTM_XCHG_BLK_MIN": 2, "YTTM_XCHG_MARGIN": 0.05}  # blocks of a few records, sized at a twentieth of the prediction: nearly every round's are too small
TINY = {"YTTM_HOT_TARGET": 40, "YTTM_HOT_MIN": 4, "YTTM_HOT_CAP": 400, "YTTM_TOP_TARGET": 8, "YTTM_TOP_CAP": 24, "YTTM_TOP_MIN": 1}
NOTES = {"YTTM_XCHG_NOTES": 2}  # two notes of possible threshold crossings: more new candidates than that and the fold walks every record
ONE_DECISION = {"YTTM_WORD_MIN_TILES": 6, "YTTM_HOT_TARGET": 24, "YTTM_HOT_MIN": 6, "YTTM_HOT_TARGET_WORDS": 96}  # (as test_word_mode_switch_is_one_decision)


def _cut(make_text):
    def shards(world):
        text = make_text()
        return [(split_like_the_reference(text, world), text)]
    return shards


def _explicit(make_shards):
    return lambda world: [(make_shards(world), None)]


def _radix_text():
    import stage_checks as S
    return S.texts_by_alphabet_size(sizes=(300,), n_words=300, seed=2)[0]


def _rank1_unfused(world):
    """hooks of one rank alone: rank 1 runs its word rounds as k_wgather + k_words + k_delta_apply, the others in one launch"""
    return [{"YTTM_WORDS_FUSE_MAX": 0} if r == 1 else {} for r in range(world)]


# row -> (shard sets of a world, run_rounds arguments, {variant: (round_checks configuration, extra environment[, world -> per-rank hooks])})
ROWS = {
    "ordinary": (_cut(text_ordinary), dict(rounds=30), {"scan": ("default", {}), "plain_apply": ("plain_apply", {}),
                                                        "one_rank_unfused": ("default", {}, _rank1_unfused)}),
    "repeat": (_cut(text_ordinary), dict(rounds=30), {"default_lists": ("default", REPEAT), "tiny_lists": ("default", dict(REPEAT, **TINY))}),
    # (target=4096: the scans are asked for nearly everything listed, so that the new pairs a walk listed come back as candidates)
    "notes": (_cut(text_ordinary), dict(rounds=30, target=4096, notes_cap=2), {"alone": ("default", NOTES), "with_repeats": ("default", dict(REPEAT, **NOTES))}),
    "giant": (_explicit(shards_giant_on_one_rank), dict(rounds=25), {"small_blocks": ("default", REPEAT)}),
    "classb_and_runs": (_explicit(shards_classb_and_runs), dict(rounds=30), {"scan": ("default", {})}),
    "blank_and_few": (lambda world: [(s, None) for s in shards_blank_and_few(world)], dict(rounds=25), {"scan": ("default", ONE_DECISION)}),
    "mirrored": (_explicit(shards_mirrored), dict(rounds=40), {"default_lists": ("default", {}), "tiny_lists": ("default", TINY)}),
    "radix": (_cut(_radix_text), dict(rounds=12), {"scan": ("default", {"YTTM_K3_RADIX_MIN": 0})}),
}
# in at least half of the checked rounds of these rows, two or more ranks' shards hold a site of the batch (else the exchange carried nothing)
SHARED_SITES = ("ordinary", "repeat", "notes", "mirrored")


def cases():
    return [(row, variant) for row, (_, _, variants) in ROWS.items() for variant in variants]


def run_row(monkeypatch, row, variant, world, small_grids=True, rounds=None):
    """every shard set of a row in a world of `world` ranks under one variant: all assertions after every round on every rank, then the
    conditions on what the run reached (assert_row)"""
    make, kw, variants = ROWS[row]
    config, extra, envs = (variants[variant] + (None,))[:3]
    out = []
    with monkeypatch.context() as m:  # (the row's hooks end with the row: a test may run several)
        kw = dict(kw, mode=R.set_config(m, config, small_grids, extra))
        if rounds:
            kw["rounds"] = rounds
        for shards, text in make(world):
            results, account = run_world(shards, text, envs=envs(world) if envs else None, monkeypatch=m, **kw)
            assert_row(row, variant, shards, results, account)
            out.append((results, account))
    return out


def assert_row(row, variant, shards, results, account):
    """the path a row is there for, from every rank's counters and from the oracle's account of the rounds"""
    world = len(results)
    rounds = results[0]["rounds"]
    has_words = [bool(s.split()) for s in shards]
    what = (row, variant, world, results, account)
    assert all(r["rounds"] == rounds and r["merge_rounds"] == rounds for r in results) and account["rounds"] == rounds >= 10, what
    assert len({r["word_switch_round"] for r in results}) == 1 and results[0]["word_switch_round"] >= 1, what  # ONE decision, after rounds on tiles
    for r, words in zip(results, has_words):
        assert (r["checked_word_rounds"] >= 8 and r["word_rounds"] == rounds - r["word_switch_round"]) if words else r["word_rounds"] == 0, what
        assert r["fused_rounds"] >= rounds // 2 or variant == "plain_apply", what  # the scan rode in the fold's tail
        assert r["rescans"] >= 1, what
    if variant == "plain_apply":
        assert all(r["fused_rounds"] == 0 for r in results), what
    if row in SHARED_SITES:
        assert 2 * account["shared_rounds"] >= rounds, what
    # Within a round a shard's count of a pair goes up only if the pair holds a token the batch made, and down only if it does not: no pair
    # gains on one rank and loses on another, and no rank's own adds take a count across a threshold the ranks' sum ends below.  (Counts that
    # go up and down within a round do so inside one rank: a tile counted anew -- the "giant" row.)
    assert account["made_and_destroyed"] == 0 and account["crossed_and_back"] == 0, what
    if (row in ("repeat", "giant") or variant == "with_repeats"):
        assert all(2 * r["exchange_retries"] > rounds for r in results), what
    else:
        assert all(r["exchange_retries"] == 0 for r in results), what
    if variant == "tiny_lists":
        assert all(r["top_refills"] >= 5 and r["hot_rebuilds"] >= 2 for r in results), what
    if row == "notes":
        assert all(r["notes_walks_proven"] >= 5 for r in results), what
    if variant == "one_rank_unfused":  # (what a rank's own kernels are is its own business: the exchange does not see it)
        assert results[1]["word_fused_rounds"] == 0 and all(r["word_fused_rounds"] >= 8 for i, r in enumerate(results) if i != 1), what
    elif row not in ("giant", "blank_and_few"):
        assert all(r["word_fused_rounds"] >= 8 for r in results), what
    if row == "giant":  # a batch goes to k_words<FUSED> in the kernel arguments unless the rank has class-C tiles: rank 0 alone has them
        assert results[0]["word_fused_rounds"] == 0 and all(r["word_fused_rounds"] >= 8 for r in results[1:]), what
    if row == "classb_and_runs":
        assert results[0]["classb_word_rounds"] >= 5 and all(r["classb_word_rounds"] == 0 for r in results[1:]), what
        assert results[1]["self_rules_in_word_mode"] >= 1, what
    if row == "mirrored":
        assert account["crossed_by_sum"] >= 1, what
    if row == "radix":
        assert all(r["k3_radix"] == 1 for r in results), what
    else:
        assert all(r["k3_radix"] == 0 for r in results), what
