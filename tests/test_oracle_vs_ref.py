"""Pins oracle/bpe_oracle.c against the UNMODIFIED reference (oracle/_ref, built from /root/reference by
oracle/Makefile).  Train parity target = the -DDETERMINISTIC_QUEUE build; encode parity =
any build; dropout at n_threads=1 in a fresh process is bit-exact.

Every answer of the reference is also committed as a digest (tests/golden/oracle_vs_ref_digests.json: md5 of the model file or of
the ids, or the error message; written by tests/golden/make_ref_digests.py): the oracle is always compared with the digest, and where
oracle/_ref is built the reference binary runs too and must give the committed digest."""
import hashlib
import json
import os
import random

import pytest

import gen
import oracle_lib as O
import refbin

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref_digests.json")
PINNED = json.load(open(DIGESTS)) if os.path.exists(DIGESTS) else {}
LIVE = refbin.available("det")
RECORDED = {}  # what the live reference answered, by case (make_ref_digests.py writes it out)


def _digest(fn):
    """md5 of what fn returns (bytes, or ids as their repr), or the message of the ValueError it raises."""
    try:
        v = fn()
    except ValueError as e:
        return "err:" + str(e)
    return "md5:" + hashlib.md5(v if isinstance(v, bytes) else repr(v).encode()).hexdigest()


def _reference(key, fn):
    """The reference's answer to case `key`: the live binary where oracle/_ref is built (it must agree with the committed digest), else the digest."""
    if LIVE:
        got = RECORDED[key] = _digest(fn)
        assert PINNED.get(key, got) == got, "the reference binary's answer to %s differs from the committed digest" % key
        return got
    assert key in PINNED, "no committed digest for %s (tests/golden/make_ref_digests.py)" % key
    return PINNED[key]


def _cmp_train(tmp_path, text, vocab, coverage=1.0, ids=(0, 1, 2, 3), n_threads=1, name="c"):
    corpus = str(tmp_path / f"{name}.txt")
    with open(corpus, "wb") as f:
        f.write(text)
    m_ref = str(tmp_path / f"{name}.ref.model")
    m_ora = str(tmp_path / f"{name}.ora.model")
    pad, unk, bos, eos = ids

    def ref():
        refbin.train(corpus, m_ref, vocab, coverage, n_threads, pad, unk, bos, eos, kind="det")
        return open(m_ref, "rb").read()

    def ora():
        O.train(text, m_ora, vocab, coverage, pad, unk, bos, eos)
        return open(m_ora, "rb").read()
    want = _reference("train/" + name, ref)
    got = _digest(ora)
    assert got == want, f"model files (or errors) differ for {name}: {got} vs {want}"
    return m_ora if got.startswith("md5:") else None


def _cmp_encode(key, want_fn, got_fn):
    want = _reference("encode/" + key, want_fn)
    got = _digest(got_fn)
    assert got == want, f"encode {key}: {got} vs {want}"


def test_readme_corpus_c1(tmp_path):
    text = gen.readme_corpus()
    _cmp_train(tmp_path, text, 5000, name="c1")


def test_stress_texts(tmp_path):
    rng = random.Random(1234)
    for it in range(120):
        text = gen.stress_text(rng, 1000, True).encode()
        vocab = len(set(text.decode()) | {" "}) + 4 + rng.randint(0, 40)
        cov = 1.0 if rng.randint(0, 1) == 0 else 1 - rng.random() * 0.4
        _cmp_train(tmp_path, text, vocab, cov, n_threads=rng.choice([1, 3, 8]), name=f"s{it}")


def test_unicode_and_special_ids(tmp_path):
    rng = random.Random(99)
    layouts = [(0, 1, 2, 3), (-1, 0, -1, -1), (5, 7, -1, 2), (3, 2, 1, 0), (-1, 3, 1, -1), (0, 40, 29, 35)]
    for it in range(60):
        kind = rng.choice(list(gen.UNICODE_ALPHABETS))
        text = gen.unicode_text(rng, rng.randint(50, 3000), kind)
        cov = rng.choice([1.0, 1.0, 0.9, 0.7, 0.999])
        ids = rng.choice(layouts)
        vocab = rng.randint(45, 120)
        _cmp_train(tmp_path, text, vocab, cov, ids, n_threads=rng.choice([1, 8]), name=f"u{it}")


def test_invalid_utf8_with_coverage(tmp_path):
    # with coverage < 1 removing something, the reference drops invalid bytes (bpe.cpp:357-380)
    rng = random.Random(5)
    for it in range(20):
        text = gen.unicode_text(rng, 2000, "mix", p_invalid=0.05)
        _cmp_train(tmp_path, text, 80, 0.8, name=f"inv{it}")


def test_config_errors(tmp_path):
    text = b"aaa bbb abab"
    for i, kw in enumerate([dict(coverage=0.0), dict(coverage=1.5), dict(ids=(0, 300, 2, 3)), dict(ids=(0, 1, 1, 3)),
                            dict(ids=(-2, 1, 2, 3)), dict(vocab=5)]):
        vocab = kw.pop("vocab", 50)
        _cmp_train(tmp_path, text, vocab, kw.get("coverage", 1.0), kw.get("ids", (0, 1, 2, 3)), name=f"err{i}")


def _sentences(rng, n, alphabet="abcde  "):
    out = []
    for _ in range(n):
        k = rng.randint(0, 60)
        out.append("".join(rng.choice(alphabet) for _ in range(k)).encode())
    return out


def test_encode_ids_vs_ref(tmp_path):
    rng = random.Random(7)
    text = gen.readme_corpus(2000, 100)
    cases = [((0, 1, 2, 3), 800), ((5, 7, -1, 2), 300), ((-1, 0, -1, -1), 200), ((0, 60, 29, 35), 500)]
    for ci, (ids, vocab) in enumerate(cases):
        model = _cmp_train(tmp_path, text, vocab, ids=ids, name=f"e{ci}")
        sents = _sentences(rng, 300) + [b"", b"   ", b"a", b" a ", "жж a ж".encode(), b"\xff\xfea b\x80"]
        lines = str(tmp_path / f"e{ci}.lines")
        # the reference driver reads lines with getline: no newlines inside sentences
        with open(lines, "wb") as f:
            f.write(b"\n".join(sents) + b"\n")
        m = O.Model(model)
        pad, unk, bos_id, eos_id = ids
        for bos, eos, rev in [(0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 1, 1)]:
            if (bos and bos_id == -1) or (eos and eos_id == -1):
                want = _reference(f"encode/e{ci}/{bos}{eos}{rev}", lambda: refbin.encode(model, lines, 1, bos, eos, rev))
                assert want.startswith("err:")
                assert _digest(lambda: m.encode(sents, bos, eos, rev)) == want
                continue
            _cmp_encode(f"e{ci}/{bos}{eos}{rev}", lambda: refbin.encode(model, lines, 1, bos, eos, rev), lambda: m.encode(sents, bos, eos, rev))
            _cmp_encode(f"e{ci}/{bos}{eos}{rev}/8", lambda: refbin.encode(model, lines, 8, bos, eos, rev), lambda: m.encode(sents, bos, eos, rev))


def test_encode_dropout_bit_exact_single_thread(tmp_path):
    rng = random.Random(11)
    text = gen.readme_corpus(2000, 100)
    model = _cmp_train(tmp_path, text, 1000, name="d")
    sents = _sentences(rng, 300, "abcd  ")
    lines = str(tmp_path / "d.lines")
    with open(lines, "wb") as f:
        f.write(b"\n".join(sents) + b"\n")
    m = O.Model(model)
    for p in [0.1, 0.5, 1.0]:
        O.rng_reset()
        _cmp_encode(f"dropout/{p}", lambda: refbin.encode(model, lines, 1, dropout=p),  # fresh process: mt19937 default seed 5489
                    lambda: m.encode(sents, dropout_prob=p))
