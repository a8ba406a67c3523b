"""GPU tests of mrg_job_vocab / mrg_vocab_encode (k_encode.hip): a frozen word -> id table and text ->
id sequences on the device.

No expectation comes from the library: the tokens of every document come from the C oracle
(oracle_lib.tokens), the ranks from a Counter over them sorted by (count descending, key bytes
ascending) -- under flags 0 from the oracle's mr-{r}.txt lines, as tests/test_gpu_topk.py does -- and
the expected id of a token is rank.get(token, 0xFFFFFFFF).  Every case also checks that h_tok_off is
the prefix sum of the per-document token counts."""
import collections
import gzip
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_COMPAT = 0x1
UNK = 0xFFFFFFFF
SENTINEL = 0xFFFFFFFE  # never an id here (vocabularies are far smaller) and not UNK


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


def ranked(lines):
    def order(ln):
        key, c = ln.rsplit(b" ", 1)
        return (-int(c), key)
    return sorted(lines, key=order)


def cat(lines):
    return b"".join(l + b"\n" for l in lines)


def count_lines(doc_tokens):
    cnt = collections.Counter()
    for t in doc_tokens:
        cnt.update(t)
    return [k + b" " + str(c).encode() for k, c in cnt.items()]


def cut(lines, max_words, min_count):
    """The vocabulary's lines: the ranked lines, at most max_words (0: all), up to the first count below min_count."""
    out = []
    for ln in lines if not max_words else lines[:max_words]:
        if int(ln.rsplit(b" ", 1)[1]) < min_count:
            break
        out.append(ln)
    return out


def rank_of(lines):
    return {ln.rsplit(b" ", 1)[0]: i for i, ln in enumerate(lines)}


def expected(doc_tokens, rank):
    ids, off = [], [0]
    for t in doc_tokens:
        ids += [rank.get(x, UNK) for x in t]
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), off


def start_job(ctx, blobs, R=1, flags=NO_COMPAT):
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    t, off = to_device(blobs)
    ctx.job_begin(M.APP_WC, R, flags)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    return t


def encode(ctx, v, blobs):
    """count-only call, then the full call into a sentinel-filled buffer; returns (ids, tok_off)"""
    import torch
    from gpu_util import to_device
    t, off = to_device(blobs)
    tok = ctx.encode(v, t.data_ptr(), off)
    assert len(tok) == len(blobs) + 1 and tok[0] == 0
    n = tok[-1]
    out = torch.full((n + 3,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    tok2 = ctx.encode(v, t.data_ptr(), off, out.data_ptr(), n)
    assert tok2 == tok, "the count-only call and the full call disagree on the offsets"
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == SENTINEL).all(), "wrote past the last token"
    del t
    return got[:n], tok


def check(ctx, v, blobs, rank, doc_tokens=None):
    import oracle_lib as O
    if doc_tokens is None:
        doc_tokens = [O.tokens(b) for b in blobs]
    exp, off = expected(doc_tokens, rank)
    got, tok = encode(ctx, v, blobs)
    assert tok == off
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), bad.size)


# ---- 1. the bundled corpus

@pytest.fixture(scope="module")
def corpus_tokens(corpus):
    import oracle_lib as O
    return [O.tokens(d) for d in corpus]


@pytest.fixture(scope="module")
def corpus_lines(corpus, corpus_tokens):
    import oracle_lib as O
    return {NO_COMPAT: ranked(count_lines(corpus_tokens)),
            0: ranked([l for o in O.wc(corpus, 10, O.FAST) for l in o.split(b"\n") if l])}


@pytest.fixture(scope="module")
def corpus_index(corpus_tokens):
    """Every token of the corpus as an index into its distinct words: expected ids by one numpy lookup."""
    words = {}
    inv = [np.array([words.setdefault(x, len(words)) for x in t], dtype=np.int64) for t in corpus_tokens]
    return words, inv


@pytest.mark.parametrize("min_count", [1, 5])
@pytest.mark.parametrize("max_words", [1, 1000, 0])
@pytest.mark.parametrize("flags", [0, NO_COMPAT])
def test_corpus(ctx, corpus, corpus_lines, corpus_index, flags, max_words, min_count):
    t = start_job(ctx, corpus, 10, flags)
    exp_lines = cut(corpus_lines[flags], max_words, min_count)
    with ctx.vocab(max_words, min_count) as v:
        text = v.text()
        assert text == cat(exp_lines)
        top = [l for l in ctx.topk(max_words if max_words else 10**9).split(b"\n") if l]
        assert text == cat(cut(top, 0, min_count))
        assert v.size() == (len(exp_lines), len(text))
        assert v.words() == [l.rsplit(b" ", 1)[0] for l in exp_lines]
        words, inv = corpus_index
        lut = np.full(len(words), UNK, dtype=np.uint32)
        for w, i in rank_of(exp_lines).items():
            lut[words[w]] = i
        got, tok = encode(ctx, v, corpus)           # all six documents in one call
        off = [0]
        for a in inv:
            off.append(off[-1] + len(a))
        assert tok == off
        assert (got == lut[np.concatenate(inv)]).all()
        got3, tok3 = encode(ctx, v, [corpus[3]])    # document 3 alone
        assert tok3 == [0, len(inv[3])]
        assert (got3 == lut[inv[3]]).all()
    del t


# ---- 2. every position of a chunk boundary: the same tail text shifted by 0..4160 bytes

def make_filler(n):
    rng = random.Random(20261019)
    out = []
    size = 0
    while size < n:
        w = "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(rng.randint(1, 20)))
        if len(w) > 2 and rng.random() < 0.2:
            i = rng.randrange(1, len(w))
            w = w[:i] + rng.choice("'-") + w[i:]
        sep = rng.choice([" ", " ", " ", "  ", "\t", "\n"])
        out.append(w + sep)
        size += len(w) + len(sep)
    return "".join(out).encode()


CORE = ("na\u00efve\u2014x\u2003\U00010400bc don't " + "y" * 17 + "\u00e9 zz").encode()


def test_shift_sweep(ctx):
    """One call, 4161 documents filler[:s] + CORE for s = 0..4160: the chunk is 1 KiB per wave (4 KiB per
    workgroup), so CORE's multi-byte whitespace, 4-byte letter, long key and document end cross every
    lane, chunk and workgroup boundary."""
    import oracle_lib as O
    filler = make_filler(4200)
    docs = [filler[:s] + CORE for s in range(4161)]
    assert 8_000_000 < sum(map(len, docs)) < 10_000_000
    doc_tokens = [O.tokens(d) for d in docs]
    lines = ranked(count_lines(doc_tokens))
    half = len(lines) // 2
    t = start_job(ctx, docs, 4, NO_COMPAT)
    with ctx.vocab(half) as v:
        assert v.text() == cat(lines[:half])
        rank = rank_of(lines[:half])
        exp, _ = expected(doc_tokens, rank)
        assert (exp == UNK).any() and (exp != UNK).any()
        check(ctx, v, docs, rank, doc_tokens)
    del t


# ---- 3. Unicode whitespace and classes

UNI = [
    ("don't a\u2014b -- x", [b"dont", b"ab", b"x"]),
    ("p\u0085q\u00a0r\u2003s\u3000t\u2028u", [b"p", b"q", b"r", b"s", b"t", b"u"]),   # each one White_Space
    ("a\u200bb", [b"ab"]),                                     # ZERO WIDTH SPACE is neither \s nor \w
    ("''' \u2014 ...", []),
    ("e\u0301 x", ["e\u0301".encode(), b"x"]),                  # the combining mark is \w
    ("\U00010400bc \U00010400", ["\U00010400bc".encode(), "\U00010400".encode()]),   # a 4-byte letter starts a token
]


def oracle_ranked(docs):
    import oracle_lib as O
    return ranked(count_lines([O.tokens(d) for d in docs]))


def unicode_case(ctx, v, rank):
    import oracle_lib as O
    docs = [s.encode() for s, _ in UNI]
    for d, (_, toks) in zip(docs, UNI):
        assert O.tokens(d) == toks           # the table above restates the oracle
    check(ctx, v, docs, rank)
    check(ctx, v, [b" ".join(docs)], rank)


def test_unicode_classes(ctx):
    docs = [s.encode() for s, _ in UNI]
    lines = oracle_ranked(docs)
    assert sorted(rank_of(lines)) == sorted({w for _, ts in UNI for w in ts})
    t = start_job(ctx, docs)
    for k in (0, 3):                          # all words; then only three, the others UNK
        with ctx.vocab(k) as v:
            kept = lines[:k] if k else lines
            assert v.text() == cat(kept)
            unicode_case(ctx, v, rank_of(kept))
    del t


# ---- 4. document edges

def test_document_edges(ctx):
    import mapreduce_rust_amd as M
    import torch
    docs = [b"", b"  \n\t ", b"xy ab", b"cd ef", b"", b"", b"a", b"b", b"c", b" ", b"ab cd", b""]
    t = start_job(ctx, docs)
    import oracle_lib as O
    lines = ranked(count_lines([O.tokens(d) for d in docs]))
    with ctx.vocab() as v:
        assert v.text() == cat(lines)
        rank = rank_of(lines)
        assert b"abcd" not in rank and rank[b"ab"] != rank[b"cd"]
        check(ctx, v, docs, rank)
        check(ctx, v, [b"a"], rank)
        check(ctx, v, [b""], rank)
        check(ctx, v, [b"", b""], rank)
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
        assert ctx.encode(v, buf.data_ptr(), [0]) == [0]            # n_docs = 0
        assert ctx.encode(v, buf.data_ptr(), [0], buf.data_ptr(), 0) == [0]
    del t


# ---- 5. long keys

def test_long_keys(ctx):
    w16, w17, w30, w300 = "k" * 16, "m" * 17, "n" * 30, "q" * 150 + "\u00e9" * 75
    assert len(w300.encode()) == 300
    p30a, p30b = "s" * 16 + "A" * 14, "s" * 16 + "B" * 14       # same first 16 bytes, same length
    o17 = w17[:-1] + "z"                                        # differs from a vocabulary word in its last byte
    voc_doc = " ".join([w16, w17, w30, w300, p30a] * 2).encode()
    t = start_job(ctx, [voc_doc])
    lines = oracle_ranked([voc_doc])
    with ctx.vocab() as v:
        assert v.text() == cat(lines)
        rank = rank_of(lines)
        assert sorted(rank) == sorted(x.encode() for x in (w16, w17, w30, w300, p30a))
        text = " ".join([p30b, w300, o17, w16, p30a, w17, w16 + "k", w30, "n" * 31, w300 + "q", p30b, "k" * 15]).encode()
        check(ctx, v, [text, voc_doc, text], rank)
        got, _ = encode(ctx, v, [text])
        assert list(got[:3]) == [UNK, rank[w300.encode()], UNK]
    del t


# ---- 6. hash collisions and ties

def tie_words():
    words = ["abcdefgh", "abcdefgh1", "abcdefgh2", "abcdefghi", "abcdefghij1", "abcdefghij2"]
    words += [w + s for w in ("x" * 16, "x" * 16 + "a", "x" * 17, "x" * 30) for s in ("", "é")]
    words += ["naïve", "ſong", "Ærø", "a"]
    words += ["w%02d" % i for i in range(42)]
    return words


@pytest.mark.parametrize("flags", [NO_COMPAT | (3 << 8), 3 << 8])   # 3 << 8 = MRG_FLAG_DEBUG_HASH_BITS(3)
def test_collisions_and_ties(ctx, flags):
    import oracle_lib as O
    rng = random.Random(2026)
    toks = []
    for w in tie_words():
        toks += [w] * rng.choice((1, 2, 3, 7))
    rng.shuffle(toks)
    text = " ".join(toks).encode()
    if flags & NO_COMPAT:
        lines = ranked(count_lines([O.tokens(text)]))
    else:
        lines = ranked([l for o in O.wc([text], 5, O.FAST) for l in o.split(b"\n") if l])
    counts = [int(l.rsplit(b" ", 1)[1]) for l in lines]
    inside = [k for k in range(1, len(lines)) if counts[k - 1] == counts[k]]   # cuts inside a run of equal counts
    t = start_job(ctx, [text], 5, flags)
    for k in (inside[0], inside[len(inside) // 2], inside[-1], len(lines)):
        with ctx.vocab(k) as v:
            assert v.text() == cat(lines[:k])
            check(ctx, v, [text, text[: len(text) // 2]], rank_of(lines[:k]))
    del t


# ---- 7. a streamed job

def test_streamed_job(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import to_device
    docs = [d[:200_000] for d in corpus]
    batches = [docs[0:2], docs[2:3], docs[3:6]]
    t = start_job(ctx, docs, 10, 0)
    with ctx.vocab(500) as v_one:
        one = v_one.text()
    lines = ranked([l for o in O.wc(docs, 10, O.FAST) for l in o.split(b"\n") if l])
    assert one == cat(lines[:500])
    ctx.job_begin(M.APP_WC, 10, 0)
    keep = []
    first = 0
    for b in batches:
        tb, off = to_device(b)
        keep.append(tb)
        ctx.set_input(tb.data_ptr(), off, list(range(first, first + len(b))))
        ctx.map_add()
        first += len(b)
        with ctx.vocab(500) as v_mid:                       # between batches: a vocabulary and an encode
            mid = ranked([l for o in O.wc(docs[:first], 10, O.FAST) for l in o.split(b"\n") if l])[:500]
            assert v_mid.text() == cat(mid)
            check(ctx, v_mid, [docs[5][:5000]], rank_of(mid))
    with ctx.vocab(500) as v:
        assert v.text() == one
        check(ctx, v, docs[:2], rank_of(lines[:500]))
    ctx.reduce()
    assert ctx.outputs() == O.wc(docs, 10, O.FAST)
    del t, keep


# ---- 8. lifetime

def test_lifetime(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    a, b = corpus[0][:100_000], corpus[1][:100_000]
    la, lb = ranked(count_lines([O.tokens(a)])), ranked(count_lines([O.tokens(b)]))
    t = start_job(ctx, [a])
    va = ctx.vocab(300)
    t = start_job(ctx, [b])                                 # job_begin + an unrelated job
    vb = ctx.vocab(200, 2)
    ctx.reduce()
    ctx.job_begin(M.APP_WC, 3, 0)
    assert va.text() == cat(la[:300]) and vb.text() == cat(cut(lb, 200, 2))
    before = ctx.pool_stats()[0]
    check(ctx, va, [a, b], rank_of(la[:300]))
    check(ctx, vb, [a, b], rank_of(cut(lb, 200, 2)))
    assert ctx.pool_stats()[0] == before
    with M.Context(0) as other:                             # a second context on the same device
        check(other, va, [b, a], rank_of(la[:300]))
    check(ctx, va, [b], rank_of(la[:300]))
    va.close()
    check(ctx, vb, [b], rank_of(cut(lb, 200, 2)))
    vb.close()
    vb.close()                                              # idempotent
    del t


# ---- 9. errors

def test_errors(ctx):
    import mapreduce_rust_amd as M
    import torch
    from gpu_util import to_device
    ctx.job_begin(M.APP_INDEXER, 2, 0)
    with pytest.raises(M.MrgError) as ei:
        ctx.vocab()
    assert ei.value.code == M.native.EINVAL
    docs = [s.encode() for s, _ in UNI]
    t = start_job(ctx, docs)
    lines = oracle_ranked(docs)
    with ctx.vocab() as v:
        assert v.text() == cat(lines)
        rank = rank_of(lines)
        tb, off = to_device(docs)
        n = ctx.encode(v, tb.data_ptr(), off)[-1]
        out = torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
        with pytest.raises(M.MrgError) as ei:
            ctx.encode(v, tb.data_ptr(), off, out.data_ptr(), n - 1)
        assert ei.value.code == M.native.EINVAL
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        for bad, at in (([b"ok", b"ab \xff cd"], (1, 3)), ([b"ab cd \xe2\x80", b"x"], (0, 6)),
                        ([b"x" * 2000 + b" \xe2\x80", b"\x83 y"], (0, 2001))):
            tb2, off2 = to_device(bad)
            with pytest.raises(M.MrgError) as ei:
                ctx.encode(v, tb2.data_ptr(), off2)
            assert ei.value.code == M.native.EUTF8
            assert "document %d" % at[0] in str(ei.value) and "byte offset %d" % at[1] in str(ei.value)
        unicode_case(ctx, v, rank)                          # context and vocabulary still usable
    del t


# ---- 10. the empty vocabulary

def test_empty_vocabulary(ctx):
    docs = [b"a b a", b"", b"c a"]
    t = start_job(ctx, docs)
    with ctx.vocab(0, 4) as v:
        assert v.size() == (0, 0) and v.text() == b"" and v.words() == []
        got, tok = encode(ctx, v, docs)
        assert tok == [0, 3, 3, 5] and (got == UNK).all()
    with ctx.vocab(0, 3) as v:
        assert v.text() == b"a 3\n"
    del t
