"""GPU tests of mrg_vocab_from_text (a vocabulary from its "word count\\n" text, on any device) and
mrg_vocab_decode (k_decode.hip: id sequences -> text on the device).

No expectation comes from the library: words and ranks come from the C oracle (oracle_lib.tokens /
oracle_lib.wc) exactly as tests/test_gpu_encode.py builds them (helpers in tests/vocab_util.py), the
expected id of a token is rank.get(token, 0xFFFFFFFF), and decoded text is built in Python as
b"".join(word[id] + separator).  The decoder takes 256 ids per chunk (one wave, 4 ids per lane) and
stages its output in 2048-byte windows; the boundary sweep below is sized by those two numbers."""
import ctypes as C
import gzip
import os
import random

import numpy as np
import pytest

from vocab_util import (BYTE_SENTINEL, NO_COMPAT, UNI, UNK, cat, check, count_lines, decode, decode_dev, encode,
                        encode_dev, expected, expected_text, ids_to_device, rank_of, ranked, start_job, tie_words,
                        words_of)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEC_CHUNK = 256   # MRG_DEC_CHUNK: ids of one decoder chunk
DEC_WIN = 2048    # bytes of one LDS window of the emit pass


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


@pytest.fixture(scope="module")
def corpus_tokens(corpus):
    import oracle_lib as O
    return [O.tokens(d) for d in corpus]


@pytest.fixture(scope="module")
def corpus_ranked(corpus_tokens):
    return ranked(count_lines(corpus_tokens))


@pytest.fixture(scope="module")
def corpus_index(corpus_tokens):
    """Every token of the corpus as an index into its distinct words: expected ids by one numpy lookup."""
    words = {}
    inv = [np.array([words.setdefault(x, len(words)) for x in t], dtype=np.int64) for t in corpus_tokens]
    return words, inv


def whole(doc, n):
    """the first n bytes of doc, cut back to the end of a token (never inside a UTF-8 sequence)"""
    return doc[:doc.rindex(b" ", 0, n)]


def corpus_expected(corpus_index, lines):
    words, inv = corpus_index
    lut = np.full(len(words), UNK, dtype=np.uint32)
    for w, i in rank_of(lines).items():
        lut[words[w]] = i
    off = [0]
    for a in inv:
        off.append(off[-1] + len(a))
    return lut[np.concatenate(inv)], off


# ================================================================ from_text

# ---- 1. no job at all

@pytest.mark.parametrize("order", ["ranked", "sorted"])
def test_from_text_without_a_job(corpus, corpus_ranked, corpus_index, order):
    import mapreduce_rust_amd as M
    lines = corpus_ranked if order == "ranked" else sorted(corpus_ranked)
    with M.Context(0) as c:                                  # a fresh context: no job was ever begun on it
        text = cat(lines)
        with c.vocab_from_text(text) as v:
            assert v.text() == text
            assert v.size() == (len(lines), len(text))
            assert v.words() == words_of(lines)
            exp, off = corpus_expected(corpus_index, lines)
            assert not (exp == UNK).any()
            got, tok = encode(c, v, corpus)
            assert tok == off and (got == exp).all()
        with c.vocab_from_text(cat(lines[:1000])) as v:
            exp, off = corpus_expected(corpus_index, lines[:1000])
            assert (exp == UNK).any() and (exp != UNK).any()
            got, tok = encode(c, v, corpus)
            assert tok == off and (got == exp).all()


# ---- 2. round trip through the text, other contexts, files

def test_round_trip(ctx, corpus, corpus_ranked, tmp_path):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    t = start_job(ctx, corpus, 10, NO_COMPAT)
    kept = [l for l in corpus_ranked[:1000] if int(l.rsplit(b" ", 1)[1]) >= 5]
    docs = [whole(corpus[2], 300_000), whole(corpus[5], 100_000)]
    with ctx.vocab(1000, 5) as v:
        text = v.text()
        assert text == cat(kept)
        ids, tok = encode(ctx, v, docs)
        v.save(str(tmp_path / "vocab.txt"))
    exp, off = expected([O.tokens(d) for d in docs], rank_of(kept))
    assert tok == off and (ids == exp).all()
    with ctx.vocab_from_text(text) as v2:
        assert v2.text() == text and v2.size() == (len(kept), len(text))
        ids2, tok2 = encode(ctx, v2, docs)
        assert tok2 == tok and (ids2 == ids).all()
    with M.Context(0) as other:                              # made and used on a second context
        with other.vocab_from_text(text) as v3:
            assert v3.text() == text
            ids3, tok3 = encode(other, v3, docs)
            assert tok3 == tok and (ids3 == ids).all()
    maker = M.Context(0)
    v4 = maker.vocab_load(str(tmp_path / "vocab.txt"))
    maker.close()                                            # the vocabulary outlives the context that made it
    ctx.job_begin(M.APP_WC, 3, 0)
    assert v4.text() == text
    ids4, tok4 = encode(ctx, v4, docs)
    assert tok4 == tok and (ids4 == ids).all()
    v4.close()
    assert (tmp_path / "vocab.txt").read_bytes() == text
    del t


# ---- 3. accepted forms

def test_accepted_forms(ctx):
    uni_words = sorted({w for _, ts in UNI for w in ts})
    lines = [b"b 1", b"a 5", b"zero 0", b"big 99999999999999999999", b"mid 3", b"na\xc3\xafve 2"]
    lines += [w + b" " + str(7 * i % 5).encode() for i, w in enumerate(uni_words) if w not in (b"a", b"b")]
    assert len(rank_of(lines)) == len(lines)
    text = cat(lines)
    with ctx.vocab_from_text(text) as v:
        assert v.text() == text and v.size() == (len(lines), len(text)) and v.words() == words_of(lines)
        docs = [s.encode() for s, _ in UNI] + [b"zero big  a b mid nope na\xc3\xafve"]
        check(ctx, v, docs, rank_of(lines))


# ---- 4. long words and forced collisions

def test_long_words(ctx):
    w16, w17, w30, w300 = "k" * 16, "m" * 17, "n" * 30, "q" * 150 + "\u00e9" * 75
    assert len(w300.encode()) == 300
    p30a, p30b = "s" * 16 + "A" * 14, "s" * 16 + "B" * 14       # same first 16 bytes, same length
    o17 = w17[:-1] + "z"                                        # differs from a vocabulary word in its last byte
    lines = [w.encode() + b" 1" for w in (w16, w17, w30, w300, p30a, p30b, "x")]
    text = cat(lines)
    with ctx.vocab_from_text(text) as v:
        assert v.text() == text
        rank = rank_of(lines)
        doc = " ".join([p30b, w300, o17, w16, p30a, w17, w16 + "k", w30, "n" * 31, w300 + "q", p30b, "k" * 15, "x"]).encode()
        check(ctx, v, [doc, doc[:400], doc], rank)
        got, _ = encode(ctx, v, [doc])
        assert list(got[:5]) == [rank[p30b.encode()], rank[w300.encode()], UNK, rank[w16.encode()], rank[p30a.encode()]]


def test_forced_collisions(ctx):
    import mapreduce_rust_amd as M
    rng = random.Random(2026)
    words = tie_words()
    rng.shuffle(words)
    lines = [w.encode() + b" " + str(rng.choice((1, 2, 3, 7))).encode() for w in words]
    text = cat(lines)
    flags = M.debug_hash_bits(3)
    with ctx.vocab_from_text(text, flags) as v:
        assert v.text() == text
        doc = " ".join(words + ["x" * 31, "x" * 30 + "\u00ea", "abcdefgh3"] + words[::-1]).encode()
        check(ctx, v, [doc, doc[:doc.index(b" ", len(doc) // 2)]], rank_of(lines))
    dup = lines + [("x" * 30 + "\u00e9").encode() + b" 9"]       # a long word again, under the truncated hash
    with pytest.raises(M.MrgError) as ei:
        ctx.vocab_from_text(cat(dup), flags)
    assert ei.value.code == M.native.EINVAL and "duplicate" in str(ei.value)
    first = words.index("x" * 30 + "\u00e9")
    assert any("line %d:" % n in str(ei.value) for n in (first, len(lines)))


# ---- 5. errors

W30 = b"t" * 30
GOOD = b"alpha 3\nbeta 2\n"     # two good lines first: the bad one is line 2
BAD = [
    ("no final newline", GOOD + b"c 1", "EINVAL", (2,)),
    ("empty line", GOOD + b"\nc 1\n", "EINVAL", (2,)),
    ("no count", GOOD + b"abc\n", "EINVAL", (2,)),
    ("two spaces", GOOD + b"a  1\n", "EINVAL", (2,)),
    ("count not digits", GOOD + b"a 1x\n", "EINVAL", (2,)),
    ("21 digits", GOOD + b"a " + b"1" * 21 + b"\n", "EINVAL", (2,)),
    ("empty word", GOOD + b" 1\n", "EINVAL", (2,)),
    ("apostrophe", GOOD + b"don't 3\n", "EINVAL", (2,)),
    ("U+2014", GOOD + "a\u2014b 3\n".encode(), "EINVAL", (2,)),
    ("U+2003", GOOD + "a\u2003b 3\n".encode(), "EINVAL", (2,)),
    ("space in the word", GOOD + b"a b 3\n", "EINVAL", (2,)),
    ("NUL", GOOD + b"a\x00b 3\n", "EINVAL", (2,)),
    ("invalid UTF-8", GOOD + b"a\xffb 3\nc 1\n", "EUTF8", (2,)),
    ("truncated UTF-8", GOOD + b"a\xe2\x80 3\n", "EUTF8", (2,)),
    ("duplicate short word", GOOD + b"gamma 1\nx 1\ngamma 5\n", "EINVAL", (2, 4)),
    ("duplicate 30-byte word", GOOD + W30 + b" 1\nx 1\n" + W30 + b" 5\n", "EINVAL", (2, 4)),
    ("stray flag bit", GOOD, "EINVAL", None),
]


@pytest.mark.parametrize("what,text,code,lines", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_from_text_errors(ctx, what, text, code, lines):
    import mapreduce_rust_amd as M
    L = M.native.load()
    with ctx.vocab_from_text(GOOD) as keep:                      # another vocabulary stays usable
        ctx.vocab_from_text(b"warm 1\nup 2\n").close()
        before = ctx.pool_stats()
        flags = 0x1 if lines is None else 0
        h = C.c_void_p(0xDEAD)
        rc = L.mrg_vocab_from_text(ctx.h, text, len(text), flags, C.byref(h))
        assert rc == getattr(M.native, code), (what, rc)
        assert h.value is None, "*out must be NULL on failure"
        msg = L.mrg_last_error().decode()
        if lines is not None:
            assert any("line %d:" % n in msg for n in lines), msg
        if "duplicate" in what:
            assert "duplicate" in msg
        assert ctx.pool_stats() == before, "scratch not returned"
        with ctx.vocab_from_text(b"after 1\nthe 2\nerror 3\n") as v:      # a following successful call
            assert v.words() == [b"after", b"the", b"error"]
            assert ctx.pool_stats() == before
            check(ctx, v, [b"the error after x"], {b"after": 0, b"the": 1, b"error": 2})
        assert ctx.pool_stats()[0] == before[0]
        check(ctx, keep, [b"beta alpha gamma"], {b"alpha": 0, b"beta": 1})


def test_empty_text(ctx):
    before = ctx.pool_stats()[0]
    for text in (b"", None):
        h = C.c_void_p(0xDEAD)
        import mapreduce_rust_amd as M
        assert M.native.load().mrg_vocab_from_text(ctx.h, text, 0, 0, C.byref(h)) == 0
        v = M.Vocab(h)
        assert v.size() == (0, 0) and v.text() == b"" and v.words() == []
        got, tok = encode(ctx, v, [b"a b a", b"", b"c a"])
        assert tok == [0, 3, 3, 5] and (got == UNK).all()
        v.close()
    assert ctx.pool_stats()[0] == before


# ---- 6. the files of mrg_run_job: the source of a multi-GPU job's vocabulary

def test_run_job_files(ctx, corpus, corpus_ranked, tmp_path):
    import mapreduce_rust_amd as M
    d = tmp_path / "data"
    d.mkdir()
    files = []
    for m in range(6):
        (d / f"gut-{m}.txt").write_bytes(corpus[m])
        files.append(f"data/gut-{m}.txt")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        M.native.run_job(files, 10, M.APP_WC, ".", NO_COMPAT | M.FLAG_FINAL_TXT | M.native.flag_top(500), 1)
    finally:
        os.chdir(cwd)
    top = (tmp_path / "top.txt").read_bytes()
    fin = (tmp_path / "final.txt").read_bytes()
    assert top == cat(corpus_ranked[:500])
    with ctx.vocab_load(str(tmp_path / "top.txt")) as v:
        assert v.text() == top
        t = start_job(ctx, corpus, 10, NO_COMPAT)
        with ctx.vocab(500) as vj:
            assert vj.text() == v.text()
        del t
    with ctx.vocab_from_text(fin) as v:
        assert v.words() == sorted(words_of(corpus_ranked))
        assert v.text() == fin


# ================================================================ decode

# ---- 7. the corpus

def test_decode_corpus(ctx, corpus_ranked, corpus_index):
    import mapreduce_rust_amd as M
    import torch
    lines = corpus_ranked[:1000]
    words = words_of(lines)
    ids, tok = corpus_expected(corpus_index, lines)          # from the oracle, UNK included: not encode's output
    assert (ids == UNK).any()
    exp, exp_off = expected_text(words, ids, tok, b"UNK_")
    with ctx.vocab_from_text(cat(lines)) as v:
        t = ids_to_device(ids)
        before = ctx.pool_stats()[0]
        got, off, out = decode_dev(ctx, v, t.data_ptr(), tok, b"UNK_")
        assert off == exp_off
        assert got == exp
        assert ctx.pool_stats()[0] == before
        out.fill_(BYTE_SENTINEL)
        with pytest.raises(M.MrgError) as ei:
            ctx.decode(v, t.data_ptr(), tok, out.data_ptr(), off[-1] - 1, unk=b"UNK_")
        assert ei.value.code == M.native.EINVAL
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == BYTE_SENTINEL).all(), "a refused call wrote to the destination"
        got3, off3 = decode(ctx, v, ids[tok[3]:tok[4]], [0, tok[4] - tok[3]], b"UNK_")      # document 3 alone
        assert got3 == exp[exp_off[3]:exp_off[4]] and off3 == [0, exp_off[4] - exp_off[3]]


# ---- 8. every position of a lane, chunk and window boundary

SWEEP_WORDS = [b"a", b"b" * 8, b"c" * 16, b"d" * 17, b"e" * 30, b"q" * 150 + "\u00e9".encode() * 75]


@pytest.fixture(scope="module")
def sweep():
    """Documents of 0, 1, 2, ..., N ids in one call, N = 2 chunks + 2: document ends (the '\\n'), every word
    length and the 300-byte word fall at every lane and chunk position; then 3000 copies of the 300-byte
    word (903000 bytes from 12 chunks: 75 windows per chunk)."""
    assert [len(w) for w in SWEEP_WORDS] == [1, 8, 16, 17, 30, 300]
    N = 2 * DEC_CHUNK + 2
    rng = random.Random(20261019)
    tok = [0]
    for n in range(N + 1):
        tok.append(tok[-1] + n)
    ids = rng.choices(range(6), weights=[3, 3, 3, 3, 3, 1], k=tok[-1])
    ids += [5] * 3000
    tok.append(len(ids))
    ids = np.array(ids, dtype=np.uint32)
    exp, exp_off = expected_text(SWEEP_WORDS, ids, tok)
    assert 3000 * 301 > 400 * DEC_WIN and len(exp) < 10_000_000
    return ids, tok, exp, exp_off


def test_decode_boundary_sweep(ctx, sweep):
    ids, tok, exp, exp_off = sweep
    with ctx.vocab_from_text(cat(w + b" 1" for w in SWEEP_WORDS)) as v:
        got, off = decode(ctx, v, ids, tok)
        assert off == exp_off
        assert got == exp


def test_decode_unaligned_buffers(ctx, sweep):
    """ids that do not start on a 16-byte boundary (and a first offset that is not 0), a destination that
    starts at every byte of a 16-byte granule"""
    import torch
    ids, tok, exp, exp_off = sweep
    first = 300                                              # documents 300..340
    sub_tok = tok[first:first + 42]
    sub_exp = exp[exp_off[first]:exp_off[first + 41]]
    sub_off = [x - exp_off[first] for x in exp_off[first:first + 42]]
    with ctx.vocab_from_text(cat(w + b" 1" for w in SWEEP_WORDS)) as v:
        t = ids_to_device(ids)
        for k in range(16):
            skip = k % 4                                     # ids pointer at 4, 8, 12 bytes past a boundary too
            ptr = t.data_ptr() + 4 * skip
            toks = [x - skip for x in sub_tok]
            assert toks[0] > 0
            out = torch.full((len(sub_exp) + 96,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda:0")
            off = ctx.decode(v, ptr, toks, out.data_ptr() + 16 + k, len(sub_exp))
            torch.cuda.synchronize()
            got = out.cpu().numpy().tobytes()
            assert off == sub_off
            assert got[16 + k:16 + k + len(sub_exp)] == sub_exp, k
            assert got[:16 + k] == bytes([BYTE_SENTINEL]) * (16 + k), k
            assert got[16 + k + len(sub_exp):] == bytes([BYTE_SENTINEL]) * (80 - k), k


# ---- 9. round trip through the encoder

def test_decode_encode_round_trip(ctx, corpus, corpus_ranked):
    import oracle_lib as O
    import torch
    lines = corpus_ranked[:300] + [b"y" * 40 + b" 1"]
    docs = [b"", whole(corpus[0], 50_000), b"", b"", b"zzzunknownzzz " + b"y" * 40, whole(corpus[4], 20_000), b""]
    ids, tok = expected([O.tokens(d) for d in docs], rank_of(lines))
    assert (ids == UNK).any() and tok[1] == 0 and tok[-1] == tok[-2]
    unk = b"UNK_"                                            # \w only, and not a word of the vocabulary
    assert unk not in rank_of(lines)
    with ctx.vocab_from_text(cat(lines)) as v:
        t = ids_to_device(ids)
        text, off, out = decode_dev(ctx, v, t.data_ptr(), tok, unk)
        assert (text, off) == expected_text(words_of(lines), ids, tok, unk)
        ids2, tok2 = encode_dev(ctx, v, out.data_ptr(), off)          # the decoded text, on the device, re-encoded
        assert tok2 == tok and (ids2 == ids).all()
        # no ids at all
        empty = np.zeros(0, dtype=np.uint32)
        assert decode(ctx, v, empty, [0, 0]) == (b"", [0, 0])
        assert decode(ctx, v, empty, [0, 0, 0, 0]) == (b"", [0, 0, 0, 0])
        assert decode(ctx, v, empty, [0]) == (b"", [0])                # n_docs = 0
        assert ctx.decode(v, None, [0]) == [0] and ctx.decode(v, None, [5, 5, 5]) == [0, 0, 0]
        ids1, tok1 = encode(ctx, v, [b""])
        assert tok1 == [0, 0] and decode(ctx, v, ids1, tok1) == (b"", [0, 0])


# ---- 10. errors and state

def test_decode_errors_and_state(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import to_device
    lines = [b"w%d 1" % i for i in range(10)]
    n = 700
    rng = random.Random(5)
    base = np.array([rng.randrange(10) for _ in range(n)], dtype=np.uint32)
    tok = [0, 100, 100, n]
    with ctx.vocab_from_text(cat(lines)) as v:
        decode(ctx, v, base, tok)                            # (the pool has seen these sizes)
        before = ctx.pool_stats()
        for bad_id, unk in ((10, b""), (10, b"U"), (UNK, b""), (UNK - 1, b"U")):
            for at in (0, n // 2, n - 1):
                ids = base.copy()
                ids[at] = bad_id
                if at:
                    ids[at + 1:at + 3] = bad_id              # later bad ids: the first one is named
                t = ids_to_device(ids)
                with pytest.raises(M.MrgError) as ei:
                    ctx.decode(v, t.data_ptr(), tok, unk=unk)
                assert ei.value.code == M.native.EINVAL and "index %d " % at in str(ei.value), str(ei.value)
                assert ctx.pool_stats() == before
        with pytest.raises(M.MrgError) as ei:
            ctx.decode(v, ids_to_device(base).data_ptr(), [0, 100, 99, n])
        assert ei.value.code == M.native.EINVAL and "non-decreasing" in str(ei.value)
        assert ctx.pool_stats() == before
        got, off = decode(ctx, v, base, tok, b"U")           # context and vocabulary still usable
        assert (got, off) == expected_text(words_of(lines), base, tok, b"U")
    with ctx.vocab_from_text(b"") as v0:                       # the empty vocabulary: all-UNK input
        ids = np.full(600, UNK, dtype=np.uint32)
        assert decode(ctx, v0, ids, [0, 1, 600], b"unk") == (b"unk\n" + b"unk " * 598 + b"unk\n", [0, 4, 2400])
        long_unk = bytes(range(65, 91)) * 9 + b"0123456789" * 2 + b"x"
        assert len(long_unk) == 255
        assert decode(ctx, v0, ids[:3], [0, 3], long_unk)[0] == long_unk + b" " + long_unk + b" " + long_unk + b"\n"
        with pytest.raises(M.MrgError):
            ctx.decode(v0, ids_to_device(ids).data_ptr(), [0, 600])
    # between two map_add batches: the job does not notice
    docs = [whole(d, 100_000) for d in corpus[:4]]
    ctx.job_begin(M.APP_WC, 10, 0)
    keep = []
    with ctx.vocab_from_text(cat(lines)) as v:
        for first, batch in ((0, docs[:2]), (2, docs[2:])):
            tb, off = to_device(batch)
            keep.append(tb)
            ctx.set_input(tb.data_ptr(), off, list(range(first, first + len(batch))))
            ctx.map_add()
            got, o = decode(ctx, v, base, tok)
            assert (got, o) == expected_text(words_of(lines), base, tok)
    ctx.reduce()
    assert ctx.outputs() == O.wc(docs, 10, O.FAST)
    del keep
