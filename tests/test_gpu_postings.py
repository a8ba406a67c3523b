"""GPU tests of mrg_vocab_postings (k_postings.hip): the inverted index over ids, the transpose of the CSR
that mrg_vocab_term_counts writes.

No expectation comes from the library: the expected index is built in numpy from the CSR arrays
(tests/postings_util.py expected_postings, itself checked against a dict of lists by
tests/test_postings_cpu.py); for the corpus the ids come from the C oracle's tokens ranked as
tests/vocab_util.py ranks them, and the index is also compared with the oracle's indexer output.  Every
call goes df-only first, then full with cap exact into sentinel-filled buffers with slack
(postings_util.postings_dev).  Terms below POST_LDS_WORDS are counted in LDS, the others with global
atomics; the radix sort runs one pass per byte that n_words - 1 can set; one workgroup finds the rows of
POST_TILE entries: the sweeps below are sized by those numbers.  Every bad input here is one the contract
answers with a status code."""
import gzip
import os
import random

import numpy as np
import pytest

from postings_util import SENTINEL, SENTINEL64, check, check_dev, expected_postings, postings_dev, to_device_u32
from terms_util import expected_rows, make_vocab

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
UNK = 0xFFFFFFFF


def consts():
    from mapreduce_rust_amd import native
    return native.POST_LDS_WORDS, native.POST_TILE


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


N_WORDS = 10_000  # above POST_LDS_WORDS: both counting paths; two byte passes


@pytest.fixture(scope="module")
def vocab(ctx):
    assert N_WORDS > consts()[0] + 1
    v = make_vocab(ctx, N_WORDS)
    yield v
    v.close()


def offsets(lengths, first=0):
    return np.concatenate([[first], first + np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64).tolist()


def mixed_terms(rng, n, n_words):
    """half Zipf (small ids hot), half uniform over the vocabulary"""
    z = np.minimum(rng.zipf(1.3, n) - 1, n_words - 1)
    u = rng.integers(0, n_words, n)
    return np.where(rng.random(n) < 0.5, z, u).astype(np.uint32)


def skew_input():
    """200 000 rows of 1 to 3 entries: term 0 in every row, term 7 in every second one"""
    n = 200_000
    rng = np.random.default_rng(3)
    m = np.zeros((n, 3), dtype=np.uint32)
    m[:, 1] = 7
    m[:, 2] = rng.integers(8, N_WORDS, n)
    mask = np.ones((n, 3), dtype=bool)
    mask[1::2, 1] = False
    mask[:, 2] = rng.random(n) < 0.5
    terms = m[mask]                                          # row-major: the rows' entries in order
    counts = rng.integers(1, 50, len(terms)).astype(np.uint32)
    return terms, counts, offsets(mask.sum(axis=1)), n


# ---- 1. vocabulary sizes across the byte-pass and the LDS / global boundaries

def sweep_sizes():
    lds = consts()[0]
    return sorted({1, 2, 255, 256, 257, 65535, 65536, 65537, lds - 1, lds, lds + 1})


@pytest.mark.parametrize("n_words", [1, 2, 255, 256, 257, 8191, 8192, 8193, 65535, 65536, 65537])
def test_vocabulary_size_sweep(ctx, n_words):
    lds = consts()[0]
    assert n_words in sweep_sizes() and len(sweep_sizes()) == 11
    rng = np.random.default_rng(n_words)
    lens = rng.integers(0, 134, 300)
    lens[[0, 17, 299]] = 0
    n = int(lens.sum())
    assert 15_000 < n < 25_000
    terms = mixed_terms(rng, n, n_words)
    must = [t for t in (0, n_words - 1, lds - 1, lds) if t < n_words]
    terms[rng.permutation(n)[:len(must)]] = must             # 0, the last word, both sides of the LDS bound
    counts = rng.integers(0, 1000, n).astype(np.uint32)
    with make_vocab(ctx, n_words) as v:
        check(ctx, v, terms, counts, offsets(lens))
        info = ctx.postings_info()
    assert info["passes"] == (0 if n_words == 1 else 1 if n_words <= 256 else 2 if n_words <= 65536 else 3)
    assert info["entries"] == n and info["words"] == n_words and info["scratch_bytes"] > 0
    assert info["lds_entries"] == int((terms < lds).sum()) and info["global_entries"] == int((terms >= lds).sum())
    assert info["max_df"] == int(np.bincount(terms).max())


# ---- 2. tiles and rows

def row_layout(kind, E, T):
    if kind == "one_row":
        return [0, E, 0]
    if kind == "rows_of_one":
        return [0] + [1] * E + [0]
    if kind == "long_row":                                   # a row of 2.5 tiles between rows of 1
        long = min(E, 5 * T // 2)
        front = (E - long) // 2
        return [0] + [1] * front + [long] + [1] * (E - long - front) + [0]
    a = E // 2                                               # 5000 empty rows inside one tile
    return [0, a] + [0] * 5000 + [E - a, 0]


@pytest.mark.parametrize("kind", ["one_row", "rows_of_one", "long_row", "empty_rows"])
def test_tile_and_row_shapes(ctx, vocab, kind):
    T = consts()[1]
    for E in (1, T - 1, T, T + 1, 3 * T + 5):
        rng = np.random.default_rng(E)
        lens = row_layout(kind, E, T)
        assert sum(lens) == E and lens[0] == 0 and lens[-1] == 0
        terms = mixed_terms(rng, E, N_WORDS)
        counts = rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(np.uint32)
        check(ctx, vocab, terms, counts, offsets(lens), doc_base=11)


# ---- 3. skew: a term in every row

def test_skew(ctx, vocab):
    terms, counts, row_off, n_docs = skew_input()
    base = 1000
    off, docs, tf = check(ctx, vocab, terms, counts, row_off, doc_base=base)
    assert off[1] == n_docs and (docs[:n_docs] == base + np.arange(n_docs)).all()
    assert off[8] - off[7] == n_docs // 2
    info = ctx.postings_info()
    assert info["max_df"] == n_docs and info["lds_entries"] + info["global_entries"] == len(terms)
    assert info["global_entries"] > 0 and info["passes"] == 2


# ---- 4. any order inside a row, duplicated terms, counts of 0 and 0xFFFFFFFF

@pytest.mark.parametrize("order", ["descending", "random"])
def test_any_input_order(ctx, vocab, order):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 40, 400)
    rows = []
    for n in lens:
        r = mixed_terms(rng, n, N_WORDS)
        if n >= 4:
            r[n // 2] = r[0]                                 # a term twice in the row: two postings
            r[n - 1] = r[0]
        rows.append(np.sort(r)[::-1] if order == "descending" else r)
    terms = np.concatenate(rows).astype(np.uint32)
    counts = rng.choice(np.array([0, 1, 0xFFFFFFFF, 77], dtype=np.uint32), len(terms))
    off, docs, tf = check(ctx, vocab, terms, counts, offsets(lens))
    assert (tf == 0).any() and (tf == 0xFFFFFFFF).any()
    for w in np.unique(terms)[:200]:                         # documents never descend, and repeat for a duplicate
        d = docs[off[w]:off[w + 1]].astype(np.int64)
        assert (np.diff(d) >= 0).all()
    assert any((np.diff(docs[off[w]:off[w + 1]].astype(np.int64)) == 0).any() for w in np.unique(terms))


# ---- 5. a sub-range of a bigger CSR, an unaligned pointer, the last documents of the id space

@pytest.mark.parametrize("first", [1, 2, 3, 5])
def test_sub_range_and_doc_base(ctx, vocab, first):
    T = consts()[1]
    rng = np.random.default_rng(first)
    lens = [3, 0, 70, T + 9, 1, 0, 258]
    n = sum(lens)
    body, cnt = mixed_terms(rng, n, N_WORDS), rng.integers(0, 9, n).astype(np.uint32)
    poison = np.full(8, N_WORDS, dtype=np.uint32)            # not in the vocabulary: reading one is an error
    buf = np.concatenate([poison[:first], body, poison])
    cbuf = np.concatenate([poison[:first], cnt, poison])
    t, c = to_device_u32(buf), to_device_u32(cbuf)
    base = 2**32 - len(lens)                                 # the last document is 2^32 - 1
    a = check_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), buf, cbuf, offsets(lens, first), doc_base=base)
    assert int(a[1].max()) == 2**32 - 1
    # the same through pointers that are not 16-byte aligned, offsets from 0
    b = check_dev(ctx, vocab, t.data_ptr() + 4 * first, c.data_ptr() + 4 * first, body, cnt, offsets(lens), doc_base=base)
    for x, y in zip(a, b):
        assert (x == y).all()


# ---- 6. batches: rows [0, a) and [a, n) transposed separately

def test_batches(ctx, vocab):
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 30, 1000)
    terms = mixed_terms(rng, int(lens.sum()), N_WORDS)
    counts = rng.integers(1, 9, len(terms)).astype(np.uint32)
    row_off = offsets(lens)
    t, c = to_device_u32(terms), to_device_u32(counts)
    off, docs, tf = check_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), terms, counts, row_off)
    for a in (1, 377, 999):
        o1, d1, f1 = postings_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), row_off[:a + 1], 0)
        o2, d2, f2 = postings_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), row_off[a:], a)
        assert ((o1 + o2) == off).all()
        # per word: the first batch's list, then the second's
        n1 = (o1[1:] - o1[:-1]).astype(np.int64)
        n2 = (o2[1:] - o2[:-1]).astype(np.int64)
        which = np.repeat(np.tile([0, 1], N_WORDS), np.stack([n1, n2], 1).ravel())   # every posting's batch
        cat_d, cat_f = np.empty(len(docs), dtype=np.uint32), np.empty(len(docs), dtype=np.uint32)
        cat_d[which == 0], cat_d[which == 1] = d1, d2
        cat_f[which == 0], cat_f[which == 1] = f1, f2
        assert (cat_d == docs).all() and (cat_f == tf).all(), a


# ---- 7. determinism

def test_determinism(ctx, vocab):
    terms, counts, row_off, n_docs = skew_input()
    t, c = to_device_u32(terms), to_device_u32(counts)
    a = postings_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), row_off, 5)
    b = postings_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), row_off, 5)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- 8. the corpus: against numpy on the oracle's ids, and against the oracle's indexer

@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


def test_corpus(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    import torch
    from gpu_util import to_device
    from vocab_util import count_lines, expected, rank_of, ranked
    doc_tokens = [O.tokens(d) for d in corpus]
    lines = ranked(count_lines(doc_tokens))                  # the full vocabulary
    rank = rank_of(lines)
    exp_ids, exp_tok = expected(doc_tokens, rank)             # from the oracle: not encode's output
    assert not (exp_ids == UNK).any()
    t, off = to_device(corpus)
    ctx.job_begin(M.APP_WC, 1, M.FLAG_NO_COMPAT_DROP_LAST)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    with ctx.vocab(max_words=0) as v:
        n_words = v.size()[0]
        assert n_words == len(lines)
        tok = ctx.encode(v, t.data_ptr(), off)
        assert tok == exp_tok
        d_ids = torch.empty((tok[-1],), dtype=torch.int32, device="cuda:0")
        ctx.encode(v, t.data_ptr(), off, d_ids.data_ptr(), tok[-1])

        def index(cut):
            e_off, e_terms, e_counts, _ = expected_rows(exp_ids, cut)
            d_terms = torch.empty((max(e_off[-1], 1),), dtype=torch.int32, device="cuda:0")
            d_counts = torch.empty_like(d_terms)
            row_off, _ = ctx.term_counts(v, d_ids.data_ptr(), cut, d_terms.data_ptr(), d_counts.data_ptr(), e_off[-1])
            assert row_off == e_off
            return check_dev(ctx, v, d_terms.data_ptr(), d_counts.data_ptr(), e_terms, e_counts, row_off)

        post_off, docs, tf = index(tok)                      # (a) numpy on the oracle's ids
        # (b) the oracle's indexer: only its lines (the reference drops a partition's last group)
        seen = 0
        for line in O.indexer(corpus, ["d%d" % i for i in range(6)], 1)[0].split(b"\n"):
            if not line:
                continue
            word, n, names = line.split(b" ")
            w = rank[word]
            mine = docs[post_off[w]:post_off[w + 1]]
            assert len(mine) == int(n), (word, len(mine), int(n))
            assert {b"d%d" % d for d in mine.tolist()} == set(names.split(b",")), word
            seen += 1
        assert seen >= n_words - 1
        # the same ids as documents of about 700 ids
        rng = random.Random(700)
        cut = [0]
        while cut[-1] < tok[-1]:
            cut.append(min(tok[-1], cut[-1] + rng.randrange(350, 1050)))
        index(cut)
    del t


# ---- 9. errors

def test_bad_terms(ctx, vocab):
    import mapreduce_rust_amd as M
    import torch
    T = consts()[1]
    E = 3 * T + 5
    rng = np.random.default_rng(9)
    lens = [0, 5, T, 0, T - 5, T, 5]
    row_off = offsets(lens)
    base, counts = mixed_terms(rng, E, N_WORDS), rng.integers(0, 9, E).astype(np.uint32)
    good = check(ctx, vocab, base, counts, row_off)
    c = to_device_u32(counts)
    po = torch.zeros((N_WORDS + 1,), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((2, E), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                 # the context runs on a stream of its own
    tiles = [(0, T), (T, 2 * T), (3 * T, E)]                 # the first, a middle and the last tile
    k = 0
    for lo, hi in tiles:
        for at in (lo, (lo + hi) // 2, hi - 1):
            for bad in (N_WORDS, 0xFFFFFFFE, UNK):
                terms = base.copy()
                terms[at] = bad
                t = to_device_u32(terms)
                with pytest.raises(M.MrgError) as ei:
                    if k % 2:                                # the full call fails in its count pass too
                        ctx.postings(vocab, t.data_ptr(), c.data_ptr(), row_off, po.data_ptr(), out[0].data_ptr(),
                                     out[1].data_ptr(), E)
                    else:
                        ctx.postings(vocab, t.data_ptr(), None, row_off, po.data_ptr())
                assert ei.value.code == M.native.EINVAL and "index %d " % at in str(ei.value), (at, str(ei.value))
                k += 1
    # two bad terms: the smaller index is named
    for a, b in ((0, 1), (5, 3 * T + 4), (T - 1, T), (2 * T + 77, 3 * T)):
        terms = base.copy()
        terms[a], terms[b] = 0xFFFFFFFE, N_WORDS
        t = to_device_u32(terms)
        with pytest.raises(M.MrgError) as ei:
            ctx.postings(vocab, t.data_ptr(), None, row_off, po.data_ptr())
        assert "index %d " % a in str(ei.value), (a, b, str(ei.value))
    again = check(ctx, vocab, base, counts, row_off)
    for x, y in zip(good, again):
        assert (x == y).all()


def test_refused_before_device_work(ctx, vocab):
    import mapreduce_rust_amd as M
    import torch
    rng = np.random.default_rng(10)
    lens = [4, 0, 300, 41]
    E = sum(lens)
    row_off = offsets(lens)
    terms, counts = mixed_terms(rng, E, N_WORDS), rng.integers(0, 9, E).astype(np.uint32)
    good = check(ctx, vocab, terms, counts, row_off)
    t, c = to_device_u32(terms), to_device_u32(counts)
    po = torch.full((N_WORDS + 1,), SENTINEL64 - (1 << 64), dtype=torch.int64, device="cuda:0")
    docs = torch.full((E + 8,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    tf = docs.clone()
    torch.cuda.synchronize()                                 # the context runs on a stream of its own

    def refused(*args, needle=None, **kw):
        with pytest.raises(M.MrgError) as ei:
            ctx.postings(*args, **kw)
        assert ei.value.code == M.native.EINVAL and (needle is None or needle in str(ei.value)), str(ei.value)
        torch.cuda.synchronize()
        assert (po.cpu().numpy().view(np.uint64) == SENTINEL64).all(), "a refused call wrote to d_post_off"
        assert (docs.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to d_docs"
        assert (tf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to d_tf"
        again = check_dev(ctx, vocab, t.data_ptr(), c.data_ptr(), terms, counts, row_off)
        for x, y in zip(good, again):
            assert (x == y).all()

    P = (t.data_ptr(), c.data_ptr())
    refused(vocab, *P, row_off, po.data_ptr(), docs.data_ptr(), tf.data_ptr(), E - 1, needle="too small")
    refused(vocab, *P, row_off, po.data_ptr(), None, tf.data_ptr(), E)               # d_tf without d_docs
    refused(vocab, t.data_ptr(), None, row_off, po.data_ptr(), docs.data_ptr(), tf.data_ptr(), E)  # d_tf without d_counts
    refused(vocab, *P, row_off, None, docs.data_ptr(), tf.data_ptr(), E)             # d_post_off = NULL
    refused(vocab, *P, [0, 100, 99, E], po.data_ptr(), docs.data_ptr(), tf.data_ptr(), E, needle="non-decreasing")
    refused(vocab, *P, row_off, po.data_ptr(), docs.data_ptr(), tf.data_ptr(), E, doc_base=2**32 - len(lens) + 1)
    # the documents-only mode is not an error: d_tf stays untouched
    d2 = torch.empty((E,), dtype=torch.int32, device="cuda:0")
    po2 = torch.empty((N_WORDS + 1,), dtype=torch.int64, device="cuda:0")
    assert ctx.postings(vocab, t.data_ptr(), None, row_off, po2.data_ptr(), d2.data_ptr(), None, E, 3) == E
    torch.cuda.synchronize()
    assert (d2.cpu().numpy().view(np.uint32) == good[1] + 3).all()
    assert (po2.cpu().numpy().view(np.uint64) == good[0]).all()


def test_empty_vocabulary_and_empty_input(ctx, vocab):
    import mapreduce_rust_amd as M
    import torch
    some = to_device_u32(np.zeros(8, dtype=np.uint32))
    with ctx.vocab_from_text(b"") as v0:
        for row_off in ([0], [0, 0, 0], [3, 3]):
            off, docs, tf = postings_dev(ctx, v0, some.data_ptr(), some.data_ptr(), row_off)
            assert off.tolist() == [0] and len(docs) == 0
        po = torch.zeros((4,), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(M.MrgError) as ei:                # term 0 is not in an empty vocabulary
            ctx.postings(v0, some.data_ptr(), None, [0, 1], po.data_ptr())
        assert ei.value.code == M.native.EINVAL and "index 0 " in str(ei.value)
    for row_off in ([0], [5], [0, 0], [0, 0, 0, 0], [5, 5, 5]):   # n_docs = 0, E = 0
        off, docs, tf = postings_dev(ctx, vocab, some.data_ptr(), some.data_ptr(), row_off)
        assert (off == 0).all() and len(off) == N_WORDS + 1 and len(docs) == 0 and len(tf) == 0
    po = torch.full((N_WORDS + 1,), 7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.postings(vocab, None, None, [0, 0], po.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (po.cpu().numpy() == 0).all()


# ---- 10. no side effects: the pool, and a streamed job around the call

def test_pool_is_unchanged(ctx, vocab):
    import mapreduce_rust_amd as M
    import torch
    T = consts()[1]
    rng = np.random.default_rng(12)
    lens = [10, 500, T + 100, 0, 7]
    E = sum(lens)
    terms, counts = mixed_terms(rng, E, N_WORDS), rng.integers(0, 9, E).astype(np.uint32)
    row_off = offsets(lens)
    check(ctx, vocab, terms, counts, row_off)                # (the pool has seen these sizes)
    before = ctx.pool_stats()
    check(ctx, vocab, terms, counts, row_off)
    assert ctx.pool_stats() == before
    c = to_device_u32(counts)
    po = torch.zeros((N_WORDS + 1,), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((2, E), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                 # the context runs on a stream of its own
    for at in (3, 200, E - 1):
        bad = terms.copy()
        bad[at] = N_WORDS
        t = to_device_u32(bad)
        with pytest.raises(M.MrgError):
            ctx.postings(vocab, t.data_ptr(), None, row_off, po.data_ptr())
        assert ctx.pool_stats() == before, "scratch not returned after an error"
        with pytest.raises(M.MrgError):
            ctx.postings(vocab, t.data_ptr(), c.data_ptr(), row_off, po.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), E)
        assert ctx.pool_stats() == before
        with pytest.raises(M.MrgError):                      # refused before any device work
            ctx.postings(vocab, t.data_ptr(), c.data_ptr(), row_off, po.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                         E - 1)
        assert ctx.pool_stats() == before


def test_streamed_job_does_not_notice(ctx, vocab, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import to_device
    T = consts()[1]
    docs = [d[:d.rindex(b" ", 0, 100_000)] for d in corpus[:6]]
    lens = [10, 500, T + 100]
    rng = np.random.default_rng(13)
    terms, counts = mixed_terms(rng, sum(lens), N_WORDS), rng.integers(0, 9, sum(lens)).astype(np.uint32)
    row_off = offsets(lens)
    ctx.job_begin(M.APP_WC, 10, 0)
    keep = []
    for first in (0, 2):
        tb, off = to_device(docs[first:first + 2])
        keep.append(tb)
        ctx.set_input(tb.data_ptr(), off, list(range(first, first + 2)))
        ctx.map_add()
    top = ctx.topk(10)
    check(ctx, vocab, terms, counts, row_off)
    assert ctx.topk(10) == top
    tb, off = to_device(docs[4:6])
    keep.append(tb)
    ctx.set_input(tb.data_ptr(), off, [4, 5])
    ctx.map_add()                                            # a third batch still folds in
    check(ctx, vocab, terms, counts, row_off)
    ctx.reduce()
    assert ctx.outputs() == O.wc(docs, 10, O.FAST)
    del keep


# ---- 11. a vocabulary of another device

def test_vocabulary_of_another_device(ctx):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    with M.Context(1) as other:
        with make_vocab(other, 10) as v1:
            t = to_device_u32(np.arange(5, dtype=np.uint32))
            po = torch.zeros((11,), dtype=torch.int64, device="cuda:0")
            with pytest.raises(M.MrgError) as ei:
                ctx.postings(v1, t.data_ptr(), None, [0, 5], po.data_ptr())
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
