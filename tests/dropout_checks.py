"""BPE-dropout, exact: the ids of the dropout kernel (k_encode.hip dropout_merge and everything around it) against the oracle's restatement of the
reference's DropoutQueue process (oracle/bpe_oracle.c, pinned to the real reference by test_oracle_golden.py), BOTH drawing the keyed draws of
DESIGN.md, K5, "The draw function" -- which the oracle computes from that text, in its own code.  Shared by the emulator tests
(test_dropout_exact.py, test_dropout_exact_sched.py) and the MI355X tests (test_gpu_dropout.py).

Every comparison sets YTTM_DROPOUT_SEED, makes a fresh encoder (so the call's one pass is the encoder's first, c = 1) and demands equal ids and equal offsets for every sentence; nothing is excluded.  For 0.1 <= p <= 0.9 a case also shows that it is not
vacuous: the oracle's keyed ids differ from its deterministic ids in at least half of the sentences that have a word (Tally)."""
import contextlib
import glob
import hashlib
import os
import random

import numpy as np

import gen
import lines_checks as LN
import oracle_lib as O
import stage_checks as S

G = S.G
SALT = 0x5EED0D20
PS = (1e-18, 0.01, 0.1, 0.5, 0.9, 0.999, 1.0)
FLAGS = ((0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1))
HOOKS = ("YTTM_DROPOUT_SEED", "YTTM_DROPOUT_HEAP_FROM", "YTTM_K5_GROUP", "YTTM_DROPOUT_PACK_SENT", "YTTM_DROPOUT_NO_PACK", "YTTM_DROPOUT_HBM_QUEUES",
         "YTTM_K5_LANE_SENT", "YTTM_ENC_PIPE_FROM", "YTTM_ENC_SUB_KB", "YTTM_IO_CHUNK_KB")


@contextlib.contextmanager
def env(**kw):
    """the salt and the given hooks for the encoders made inside; whatever stood before comes back"""
    old = {k: os.environ.get(k) for k in HOOKS}
    try:
        for k in HOOKS:
            os.environ.pop(k, None)
        os.environ["YTTM_DROPOUT_SEED"] = str(SALT)
        for k, v in kw.items():
            assert k in HOOKS, k
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fresh(model_path):
    import youtokentome_amd as yttm
    return yttm.BPE(model_path)


def pack(raw):
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        np.cumsum([len(s) for s in raw], out=off[1:])
    return b"".join(raw), off


def want_ids(m, raw, p, flags=(0, 0, 0), call=1, base=0):
    """the oracle under the keyed draws of an encoder's call-th dropout call: (ids, offsets), or the message of its error"""
    b, e, r = flags
    with O.keyed(SALT, call):
        try:
            return m.encode_packed(raw, b, e, r, p, base)
        except ValueError as ex:
            return str(ex)


def first_difference(got, want, raw):
    gi, go = got
    wi, wo = want
    go, wo = [int(x) for x in go], [int(x) for x in wo]
    gi, wi = gi.tolist(), wi.tolist()
    for i in range(len(raw)):
        a, b = gi[go[i]:go[i + 1]], wi[wo[i]:wo[i + 1]]
        if a != b:
            k = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
            return "sentence %d of %d (%d bytes: %r...), first differing id at %d: got %s, oracle %s" % (i, len(raw), len(raw[i]), raw[i][:60], k, a[k:k + 8], b[k:k + 8])
    return "offsets differ"


def same(got, want, raw, what):
    assert not isinstance(want, str), (what, want)
    ok = got[1].tolist() == want[1].tolist() and got[0].tolist() == want[0].tolist()
    assert ok, (what, first_difference(got, want, raw))


def exact(model_path, m, raw, p, flags=(0, 0, 0), what=""):
    """a fresh encoder's first call, encode_packed, against the oracle -- ids and offsets, or the same error"""
    want = want_ids(m, raw, p, flags)
    core = fresh(model_path).bpe_cython
    blob, off = pack(raw)
    b, e, r = flags
    if isinstance(want, str):
        try:
            core.encode_packed(blob, off, b, e, r, p)
        except ValueError as ex:
            assert str(ex) == want, (what, str(ex), want)
            return None
        raise AssertionError("expected the oracle's error: %s %s" % (want, what))
    same(core.encode_packed(blob, off, b, e, r, p), want, raw, (what, p, flags))
    return want


class Tally:
    """non-vacuity per (model, p): of the sentences that have a word, how many the keyed oracle encodes differently from the deterministic one"""

    def __init__(self, m, raw):
        ids, off = m.encode_packed(raw)
        self.det = LN.rows(ids, off)
        self.words = sum(1 for d in self.det if d)

    def check(self, want, p, what):
        if not (0.1 <= p <= 0.9) or want is None:
            return
        differ = sum(1 for a, b in zip(LN.rows(*want), self.det) if a != b)
        assert self.words > 0 and 2 * differ >= self.words, "vacuous: %s p=%g: %d of %d sentences differ from the deterministic ids" % (what, p, differ, self.words)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def model_file(name):
    return os.path.join(G, f"train_{name}.model")


def golden_model_names():
    stress = [os.path.basename(p)[len("train_"):-len(".model")] for p in glob.glob(os.path.join(G, "train_stress*.model"))]
    return sorted(set(S.golden_encode_names()) | set(stress))


def script_of(text):
    """the gen.UNICODE_ALPHABETS kind nearest to a training text, and another one (foreign to it)"""
    s = text.decode(errors="ignore")
    if any("Ѐ" <= c <= "ӿ" for c in s):
        return "cyr", "cjk"
    if any(c >= "　" for c in s):
        return "cjk", "cyr"
    return "ascii", "cyr"


def join_lines(lines, size):
    """consecutive lines joined by a space into sentences of about `size` bytes (enough merges a sentence for dropout to show)"""
    out, cur = [], b""
    for ln in lines:
        cur = cur + b" " + ln if cur else ln
        if len(cur) >= size:
            out.append(cur)
            cur = b""
    if cur:
        out.append(cur)
    return out


def model_sentences(name, seed=31, scale=1):
    """a model's own lines, then what plain encode is tested on and dropout was not: invalid bytes, a foreign script inside words, U+2581 and tabs
    as spaces, empty and all-space sentences"""
    rng = random.Random(seed)
    train = open(os.path.join(G, f"train_{name}.txt"), "rb").read()
    enc = os.path.join(G, f"encode_{name}.lines")
    own = open(enc, "rb").read().split(b"\n")[:-1] if os.path.exists(enc) else []
    tlines = [ln for ln in train.split(b"\n") if ln][:400 * scale]
    raw = own[:300 * scale] + join_lines(tlines, 300)[:120 * scale]
    for _ in range(3):  # (small models, short lines: sentences long enough for p = 0.1 to show in most, and enough of them)
        rng.shuffle(tlines)
        raw += join_lines(tlines, 800)[:60 * scale]
    kind, foreign = script_of(train)
    for _ in range(20 * scale):
        raw.append(gen.unicode_text(rng, rng.randint(100, 400), kind, p_invalid=0.03))
    words = [w for w in train.split() if w][:2000] or [b"a"]
    other = gen.unicode_text(rng, 600, foreign).split()
    for _ in range(100 * scale):  # the model's own words in a fresh order, unknown runs inside some, other spaces between them
        s = b""
        for _ in range(rng.randint(20, 60)):
            w = rng.choice(words)
            if rng.random() < 0.3:
                cut = rng.randint(0, len(w))
                w = w[:cut] + rng.choice(other) + w[cut:]  # (a cut inside a UTF-8 sequence leaves invalid bytes: dropped, as everywhere)
            s += w + rng.choice([b" ", b" ", b"\t", "▁".encode(), b"  ", b"\n"])
        raw.append(s)
    raw += [b"", b" ", b"   \t ", "▁▁".encode(), b"\xff", b"\xff \xfe", words[0], words[0] + b" "]
    return raw


def shape_sentences(seed=29, big=True):
    """the sentence mixes of stage_checks.check_dropout_heap_equals_array and check_encode_mixed_shapes (for train_readme_small: letters abcd, a few
    unknown ones): words of 1 .. 700 tokens around 255/256/257, sentences below, around and above the LDS budget, many short sentences a pack,
    more words than lanes, runs of one letter; `big` adds a sentence of 60 000 chars"""
    rng = random.Random(seed)
    sents = [" ".join("".join(rng.choice("abcd") for _ in range(rng.choice((1, 2, 3, 5, 8, 13, 40, 200, 255, 256, 257, 700)))) for _ in range(rng.randint(1, 6)))
             for _ in range(60)] + ["", "a", "ab" * 300, "abcd" * 250]
    sents += [" ".join("".join(rng.choice("abcd") for _ in range(rng.choice((1, 2, 3, 4, 5, 8)))) for _ in range(rng.randint(0, 30))) for _ in range(70)]
    for i in range(60):  # check_encode_mixed_shapes
        kind = i % 10
        nbytes = rng.randint(0, 40) if kind < 4 else rng.randint(100, 260) if kind < 7 else rng.randint(261, 519) if kind < 9 else rng.randint(520, 1500)
        out, size = [], 0
        while size < nbytes:
            r = rng.random()
            wl = rng.randint(1, 4) if r < 0.5 else rng.randint(5, 8) if r < 0.8 else rng.randint(9, 16) if r < 0.95 else rng.randint(17, 60)
            w = rng.choice("abcd") * wl if rng.random() < 0.1 else "".join(rng.choice("abcd") if rng.random() > 0.03 else rng.choice("xyzя") for _ in range(wl))
            out.append(w)
            size += wl + 1
        sents.append((" " * rng.randint(0, 2)).join([""] + out) if rng.random() < 0.2 else " ".join(out))

    def text(n):
        return "".join(rng.choice("abcd  ") for _ in range(n)).strip()[:n]
    for n in (259, 260, 261, 518, 519, 520, 521, 1600):  # around the LDS budgets in bytes
        s = text(n + 8)[:n]
        sents.append(s if not s.endswith(" ") else s[:-1] + "a")
    sents += ["a" * 300 + " " + "b" * 255 + " " + "c" * 256 + " " + "d" * 257, " ".join("ab" for _ in range(200)), " ".join(rng.choice("abcd") for _ in range(180))]
    if big:
        sents.append(text(60000))
    return [s.encode() for s in sents]


# the 13 rows of stage_checks.check_dropout_heap_equals_array (heap_from, HBM queues, no pack, group), then YTTM_K5_LANE_SENT
HOOK_ROWS = [("1000000000", False, False, "1"), ("0", False, False, "1"), ("256", False, False, "1"), ("256", True, False, "1"), ("0", True, False, "7"),
             ("256", False, True, "1"), ("0", True, True, "1"), ("256", False, False, "7"), ("0", False, False, "24"), ("256", False, True, "24"),
             ("256", False, False, "0"), ("256", False, False, "24s2"), ("0", False, False, "24s2")]


def hook_envs():
    out = []
    for heap_from, hbm, no_pack, group in HOOK_ROWS:
        kw = {"YTTM_DROPOUT_HEAP_FROM": heap_from, "YTTM_K5_GROUP": group[:-2] if group.endswith("s2") else group}
        if group.endswith("s2"):
            kw["YTTM_DROPOUT_PACK_SENT"] = "2"
        if no_pack:
            kw["YTTM_DROPOUT_NO_PACK"] = "1"
        if hbm:
            kw["YTTM_DROPOUT_HBM_QUEUES"] = "1"
        out.append(kw)
    out += [{"YTTM_K5_LANE_SENT": v} for v in ("0", "5", "1000")]
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def check_model(model_path, raw, ps=PS, flags=FLAGS, what=""):
    m = O.Model(model_path)
    tally = Tally(m, raw)
    with env():
        for p in ps:
            for f in flags:
                want = exact(model_path, m, raw, p, f, what)
                if f == (0, 0, 0):
                    tally.check(want, p, what)


def check_golden_model(name, ps=PS, flags=FLAGS, scale=1):
    check_model(model_file(name), model_sentences(name, scale=scale), ps, flags, name)


LAYOUTS = [(0, 1, 2, 3), (-1, 0, -1, -1), (5, 7, -1, 2), (3, 2, 1, 0), (0, 40, 29, 35)]  # of test_train_encode_vs_oracle_random
LAYOUT_KINDS = ("ascii", "cyr", "cjk")


def check_layout(tmp_path, li, ki, ps=(0.01, 0.1, 0.5, 0.9), n_sent=120):
    """a model trained here by the oracle with special ids laid out otherwise -- (-1,0,-1,-1) and (3,2,1,0) make id 0 an ordinary token or <EOS>:
    the reference's "dead node = id 0" quirk under dropout; coverage 1 and below it by turns"""
    rng = random.Random(100 + 7 * li + ki)
    kind = LAYOUT_KINDS[ki]
    cov = 1.0 if (li + ki) % 2 == 0 else 0.9
    text = gen.unicode_text(rng, 12000, kind)
    model = str(tmp_path / f"layout{li}_{kind}.model")
    O.train(text, model, 60 + 40 * ki + 4, cov, *LAYOUTS[li])
    raw = [gen.unicode_text(rng, rng.randint(150, 400), kind, p_invalid=0.01) for _ in range(n_sent)]
    raw += [gen.unicode_text(rng, 200, LAYOUT_KINDS[(ki + 1) % 3]) + b" " + raw[0], b"", b"  ", raw[1] + "▁".encode() + raw[2]]
    check_model(model, raw, ps, FLAGS, (LAYOUTS[li], kind, cov))


def check_shapes_under_hooks(ps=(0.1, 0.5, 0.9, 1.0), rows=None, big=True, name="readme_small"):
    """every path of the kernel equals the ORACLE (check_dropout_heap_equals_array: the paths equal each other)"""
    model_path = model_file(name)
    m = O.Model(model_path)
    raw = shape_sentences(big=big)
    tally = Tally(m, raw)
    envs = hook_envs()
    for p in ps:
        with env():
            want = want_ids(m, raw, p)
        tally.check(want, p, "shapes")
        for kw in (envs if rows is None else [envs[i] for i in rows]):
            with env(**kw):
                core = fresh(model_path).bpe_cython
                blob, off = pack(raw)
                same(core.encode_packed(blob, off, False, False, False, p), want, raw, ("shapes", p, kw))


def check_entry_points(B, tmp_path, name="readme_small", ps=(0.1, 0.5, 1.0), torch_routes=False):
    """the same ids by every route that takes dropout_prob: encode (list of str), encode_packed, the device entry, the text entries (a sentence is
    the line WITH its newline, lines_checks.py) and encode_file; on the MI355X also BPE.encode_tensor / encode_text_tensor"""
    import youtokentome_amd as yttm
    model_path = model_file(name)
    m = O.Model(model_path)
    lines = [s for s in (open(os.path.join(G, f"encode_{name}.lines"), "rb").read().split(b"\n")[:-1]) if b"\r" not in s][:200]
    lines += [b"", b"ab cd", b" ", b"abcd " * 300, b"dcba" * 200]
    data = b"\n".join(lines) + b"\n"
    assert LN.py_split(data) == lines
    with_nl = [ln + b"\n" for ln in lines]
    path = str(tmp_path / "dropout_lines.txt")
    open(path, "wb").write(data)
    tally = Tally(m, lines)
    with env():
        for p in ps:
            for f in ((0, 0, 0), (1, 1, 1)):
                b, e, r = f
                want = want_ids(m, lines, p, f)
                want_nl = want_ids(m, with_nl, p, f)
                assert want_nl[0].tolist() == want[0].tolist()  # (a newline is a space: the two yardsticks are one)
                if f == (0, 0, 0):
                    tally.check(want, p, "entry points")
                rows = LN.rows(*want)
                assert fresh(model_path).encode([s.decode() for s in lines], yttm.OutputType.ID, bos=b, eos=e, reverse=r, dropout_prob=p) == rows, ("encode", p, f)
                blob, off = pack(lines)
                same(fresh(model_path).bpe_cython.encode_packed(blob, off, b, e, r, p), want, lines, ("encode_packed", p, f))
                core = fresh(model_path).bpe_cython  # input already in device memory
                d_b, d_o = B.put(np.frombuffer(blob + b"\0" * 16, np.uint8)), B.put(off)
                n_ids, _ = core.encode_device_raw(B.ptr(d_b), B.ptr(d_o), len(lines), len(blob), max(len(s) for s in lines), b, e, r, p)
                same(LN.take_encoded(core, B, len(lines), n_ids), want, lines, ("encode_device", p, f))
                core = fresh(model_path).bpe_cython
                same(LN.dev_encode_text(core, B, data, b, e, r, dropout=p, align=5), want, with_nl, ("encode_text_device", p, f))
                # (one piece: a file cut into several is several passes, each keyed by itself -- the distribution checks of lines_checks.py)
                same(fresh(model_path).encode_file(path, bos=b, eos=e, reverse=r, dropout_prob=p), want, with_nl, ("encode_file", p, f))
                if torch_routes:
                    bpe = fresh(model_path)
                    ids, o = bpe.encode_tensor([s.decode() for s in lines], bos=b, eos=e, reverse=r, dropout_prob=p, padded=False)
                    same((ids.cpu().numpy(), o.cpu().numpy().astype(np.uint64)), want, lines, ("encode_tensor", p, f))
                    bpe = fresh(model_path)
                    mat, lens = bpe.encode_tensor([s.decode() for s in lines], bos=b, eos=e, reverse=r, dropout_prob=p, padded=True)
                    mat, lens = mat.cpu().numpy(), lens.cpu().numpy()
                    assert [mat[i, :lens[i]].tolist() for i in range(len(lines))] == rows, ("encode_tensor padded", p, f)
                    bpe = fresh(model_path)
                    ids, o = bpe.encode_text_tensor(data, bos=b, eos=e, reverse=r, dropout_prob=p, padded=False)
                    same((ids.cpu().numpy(), o.cpu().numpy().astype(np.uint64)), want, with_nl, ("encode_text_tensor", p, f))


_SCALE_DET = {}


def check_at_scale(tmp_path, p, n=200_000):
    """the sentences and the vocab-2000 model of test_dropout_distribution_vs_reference_semantics, exact: one pass of 512 workgroups over groups of 24"""
    import youtokentome_amd as yttm
    corpus, model = str(tmp_path / "d.txt"), str(tmp_path / "d.model")
    open(corpus, "wb").write(gen.readme_corpus(4000, 100))
    yttm.BPE.train(corpus, model, 2000)
    blob = gen.abcd_corpus(n * 129, seed=77, line=128)
    off = np.arange(n + 1, dtype=np.uint64) * 129
    m = O.Model(model)
    key = (n, hashlib.md5(open(model, "rb").read()).hexdigest())  # (every p trains the model anew in its own directory: the same file, by its hash)
    if key not in _SCALE_DET:  # the deterministic ids once per model and batch
        _SCALE_DET[key] = m.encode_blob(blob, off)
    with env():
        with O.keyed(SALT):
            want = m.encode_blob(blob, off, dropout_prob=p)
        got = fresh(model).bpe_cython.encode_packed(blob, off, False, False, False, p)
    # non-vacuity, counted from below without Python lists of 200 000 rows: the sentences whose NUMBER of ids differs from the deterministic one
    differ = int((np.diff(want[1].astype(np.int64)) != np.diff(_SCALE_DET[key][1].astype(np.int64))).sum())
    assert 2 * differ >= n, (differ, n)
    assert got[1].tolist() == want[1].tolist() and np.array_equal(got[0], want[0]), first_difference(got, want, [blob[i * 129:(i + 1) * 129] for i in range(n)])
    return differ  # (a lower bound)


def check_large_vocab(tmp_path, ps=(0.1, 0.5, 0.9)):
    """vocab 40 000 on the corpus of test_vocab_above_32768_vs_oracle (which pins this model to the oracle's): rule numbers up to 2^15.3 in the
    packed events"""
    import youtokentome_amd as yttm
    corpus, model = str(tmp_path / "v40k.txt"), str(tmp_path / "v40k.model")
    open(corpus, "wb").write(gen.zipf_corpus(6_000_000, seed=5, vocab=150000))
    yttm.BPE.train(corpus, model, 40000)
    raw = join_lines([ln for ln in gen.zipf_corpus(100000, seed=12, vocab=150000).split(b"\n") if ln], 250)
    check_model(model, raw, ps, ((0, 0, 0), (1, 1, 1)), "vocab 40000")


# ---- the draw stream by itself (CPU only) ------------------------------------------------------------------------------------------------
STREAM_SALTS = (0, 1, 12345, 0x5EED0D20, 2 ** 32 - 1, 2 ** 63 + 17, 2 ** 64 - 1, 0x0123456789ABCDEF)


def stream_block(salt, n_sent=4000, n_words=32, n_draws=16):
    """h[sentence, word, draw] of call 1 under `salt`, from the oracle's draw function"""
    seed = O.call_seed(salt, 1)
    out = np.empty((n_sent, n_words, n_draws), np.uint32)
    for s in range(n_sent):
        for w in range(n_words):
            out[s, w] = O.keyed_draws(seed, s, w, n_draws)
    return out


def _corr(a, b):
    a = a.astype(np.float64).ravel()
    b = b.astype(np.float64).ravel()
    a -= a.mean()
    b -= b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())), a.size


def check_stream(salt):
    """Bounds from the statistics, not from the outcome (the test is deterministic): a skip count is binomial, |z| < 4.5 (two-sided 7e-6 per look);
    chi2 over 256 equal bins has 255 degrees of freedom, mean 1 and standard deviation sqrt(2/255) per degree, 5 of them; a sample correlation
    of n independent pairs has standard deviation 1/sqrt(n), 4.5 of them.  8 salts x 11 looks: about 1e-3 that a perfect source fails."""
    h = stream_block(salt)
    n = h.size
    out = {}
    for p in (0.01, 0.1, 0.5, 0.9):
        thr = int(p * 2.0 ** 64) >> 32
        q = thr / 2.0 ** 32
        k = int((h < thr).sum())
        z = (k - n * q) / np.sqrt(n * q * (1 - q))
        out["z%g" % p] = z
        assert abs(z) < 4.5, (salt, p, z)
    bins = np.bincount((h >> 24).ravel(), minlength=256).astype(np.float64)
    chi = float(((bins - n / 256.0) ** 2 / (n / 256.0)).sum() / 255.0)
    out["chi2/dof"] = chi
    assert abs(chi - 1.0) < 5 * np.sqrt(2.0 / 255.0), (salt, chi)
    for what, (a, b) in (("draws", (h[:, :, :-1], h[:, :, 1:])), ("words", (h[:, :-1, :], h[:, 1:, :])), ("sentences", (h[:-1], h[1:]))):
        c, m = _corr(a, b)
        out["corr " + what] = c
        assert abs(c) < 4.5 / np.sqrt(m), (salt, what, c, m)
    return out


def check_draw_function():
    """oracle_keyed_draw (one value) and oracle_keyed_draws (a run) are one function, and it is the arithmetic of DESIGN.md restated once more here
    in Python integers"""
    M32 = 0xFFFFFFFF
    for salt, sidx, word in ((0, 0, 0), (12345, 7, 3), (2 ** 64 - 1, 199_999, 511), (SALT, 2 ** 33 + 5, 70_000)):
        seed = O.call_seed(salt, 3)
        wkey = O.mix64(seed + sidx * 0x9e3779b97f4a7c15 + (word << 34))
        draw, run = wkey & M32, O.keyed_draws(seed, sidx, word, 40)
        for k in range(40):
            draw = (draw + 0x9e3779b9) & M32
            h = draw ^ (wkey >> 32)
            h ^= h >> 16
            h = (h * 0x85ebca6b) & M32
            h ^= h >> 13
            h = (h * 0xc2b2ae35) & M32
            h ^= h >> 16
            assert h == int(run[k]) == O.keyed_draw(seed, sidx, word, k), (salt, sidx, word, k)
