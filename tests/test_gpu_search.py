"""GPU tests of mrg_vocab_search (k_search.hip): BM25 top-k over the inverted index, for a batch of queries.

No expectation comes from the library: the indexes are built on the host (tests/postings_util.py
expected_postings) and uploaded, so a failure here is the search's; the expected scores are the float64 matrix of
tests/search_util.py expected_scores, compared by check_topk with the derived RTOL.  Every call goes twice into
sentinel-filled rows with slack (search_util.search_dev).  One workgroup accumulates the postings of a query
position inside one window of SEARCH_TILE postings, the select works on tiles of 1024 documents, a query's
candidates are ordered by one workgroup: the sweeps below are sized by those numbers.  Every bad input here is
one the contract answers with a status code."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from postings_util import expected_postings
from search_util import (RTOL, SENTINEL, UNK, Index, check, check_topk, dev_u32, expected_scores, lay_queries, scores_f32,
                         search_dev, search_raw)
from terms_util import make_vocab

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_WORDS = 2000


def consts():
    from mapreduce_rust_amd import native
    return native.SEARCH_TILE, native.SEARCH_MAX_K


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vocab(ctx):
    v = make_vocab(ctx, N_WORDS)
    yield v
    v.close()


def random_csr(rng, n_docs, n_words, mean_len):
    """rows of distinct ascending terms, half Zipf and half uniform over words 0 .. n_words - 2 (the last word has
    no postings); counts 1 .. 8; the lengths = the counts of a row + a few ids outside the vocabulary"""
    lens = rng.integers(0, 2 * mean_len + 1, n_docs)
    n = int(lens.sum())
    rows = np.repeat(np.arange(n_docs, dtype=np.int64), lens)
    z = np.minimum(rng.zipf(1.3, n) - 1, n_words - 2)
    t = np.where(rng.random(n) < 0.5, z, rng.integers(0, n_words - 1, n))
    pairs = np.unique(rows * n_words + t)                    # by row, then term; a term once per row
    rows, terms = pairs // n_words, (pairs % n_words).astype(np.uint32)
    counts = rng.integers(1, 9, len(terms)).astype(np.uint32)
    row_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_docs))]).astype(np.int64).tolist()
    doc_len = (np.bincount(rows, weights=counts, minlength=n_docs).astype(np.int64) + rng.integers(0, 5, n_docs))
    return terms, counts, row_off, doc_len.astype(np.uint32)


def random_index(seed, n_docs, n_words=N_WORDS, mean_len=12, doc_base=0, **pads):
    rng = np.random.default_rng(seed)
    terms, counts, row_off, doc_len = random_csr(rng, n_docs, n_words, mean_len)
    post_off, docs, tf = expected_postings(terms, counts, row_off, n_words, doc_base)
    return Index(post_off, docs, tf, doc_len, doc_base, **pads)


@pytest.fixture(scope="module")
def coll():
    ix = random_index(1, 5000)
    df = np.diff(ix.post_off.astype(np.int64))
    assert df[N_WORDS - 1] == 0 and df[0] > 1024 and ix.n_entries > 40_000
    return ix


def mixed_queries(ix, rng):
    """queries of 0, 1, 2, 7 and 64 positions: hot and rare words, repeats, MRG_ID_UNK, a word with no postings"""
    df = np.diff(ix.post_off.astype(np.int64))
    rare = [int(w) for w in np.nonzero((df > 0) & (df < 20))[0][:40]]
    hot = [0, 1, 2, 3]
    none = len(df) - 1
    assert len(rare) >= 10 and df[none] == 0
    long_q = [int(x) for x in rng.integers(0, len(df) - 1, 64)]
    long_q[5] = long_q[6] = long_q[40] = hot[1]
    long_q[9], long_q[63] = UNK, none
    return [[], [hot[0]], [rare[0]], [hot[0], rare[1]], [rare[2], rare[2]], [UNK], [UNK, UNK], [none], [none, UNK, rare[3]],
            [hot[2], UNK, rare[4], hot[2], none, rare[5], hot[3]], rare[:7], long_q, [], hot + hot]


# ---- 1. random collections and queries

@pytest.mark.parametrize("k1,b", [(0.0, 0.0), (1.2, 0.75), (1000.0, 1.0), (0.0, 1.0), (1000.0, 0.0)])
def test_random_queries(ctx, vocab, coll, k1, b):
    rng = np.random.default_rng(2)
    queries = mixed_queries(coll, rng)
    assert sorted({len(q) for q in queries}) == [0, 1, 2, 3, 7, 8, 64]
    ref = coll.ref(queries, k1, b)
    hits = (ref > 0).sum(axis=1)
    assert (hits == 0).sum() >= 5 and ((hits > 0) & (hits < 20)).any() and (hits > 1024).any()
    for k, first in ((1, 0), (2, 3), (10, 0), (1024, 5)):
        docs, scores, top_n = check(ctx, vocab, coll, queries, k, k1, b, first=first, ref=ref)
        assert top_n == [min(k, int(h)) for h in hits]
    info = ctx.search_info()
    assert info["queries"] == len(queries) and info["positions"] == sum(len(q) for q in queries)
    assert info["chunks"] == 1 and 8 <= info["acc_launches"] <= 64 and info["scratch_bytes"] > 4 * coll.n_docs * len(queries)
    df = np.diff(coll.post_off.astype(np.int64))
    assert info["postings"] == sum(int(df[t]) for q in queries for t in q if t != UNK)


# ---- 2. tiles: segment lengths around SEARCH_TILE at every 16-byte misalignment, small collections

def tile_index(n_docs, pad_docs=0, pad_tf=0, doc_base=0):
    """words of T - 1, T, T + 1 and 2.5 T postings, each starting 0, 4, 8 and 12 bytes off a 16-byte boundary
    (fillers of one posting in between), and a word in every document"""
    T = consts()[0]
    rng = np.random.default_rng(n_docs)
    sizes, marks = [], {}
    at = 0
    for S in (T - 1, T, T + 1, 5 * T // 2):
        for m in range(4):
            while at % 4 != m:
                sizes.append(1)
                at += 1
            marks[(S, m)] = len(sizes)
            sizes.append(S)
            at += S
    marks["all"] = len(sizes)
    sizes.append(n_docs)
    post_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    docs = np.concatenate([np.sort(rng.choice(n_docs, S, replace=False)) for S in sizes]).astype(np.uint32) + doc_base
    tf = rng.integers(1, 30, len(docs)).astype(np.uint32)
    doc_len = rng.integers(1, 2000, n_docs).astype(np.uint32)
    for (S, m), w in ((k, v) for k, v in marks.items() if k != "all"):
        assert int(post_off[w + 1] - post_off[w]) == S and int(post_off[w]) % 4 == m
    return Index(post_off, docs, tf, doc_len, doc_base, pad_docs=pad_docs, pad_tf=pad_tf), marks, len(sizes)


@pytest.mark.parametrize("pad_docs,pad_tf", [(0, 0), (1, 1), (2, 3), (3, 0)])
def test_tiles_and_alignment(ctx, pad_docs, pad_tf):
    T = consts()[0]
    n_docs = 5 * T // 2 + 3                                  # 10243: no multiple of the tiles
    ix, marks, n_words = tile_index(n_docs, pad_docs, pad_tf, doc_base=11)
    queries = [[w] for w in marks.values()] + [[marks[(T + 1, 1)], marks["all"], marks[(5 * T // 2, 3)], marks[(T - 1, 2)]]]
    with make_vocab(ctx, n_words) as v:
        for k in (10, 1024):
            check(ctx, v, ix, queries, k)
    assert ctx.search_info()["postings"] == sum(int(ix.post_off[w + 1] - ix.post_off[w]) for q in queries for w in q)


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_small_collections(ctx, vocab, n_docs):
    rng = np.random.default_rng(n_docs)
    terms, counts, row_off, doc_len = random_csr(rng, n_docs, N_WORDS - 1, 6)
    # word N_WORDS - 2 stands in every document, with tf 1 .. 3
    rows = np.repeat(np.arange(n_docs), np.diff(row_off))
    keep = terms != N_WORDS - 2
    terms, counts, rows = terms[keep], counts[keep], rows[keep]
    terms = np.concatenate([terms, np.full(n_docs, N_WORDS - 2, dtype=np.uint32)])
    counts = np.concatenate([counts, rng.integers(1, 4, n_docs).astype(np.uint32)])
    rows = np.concatenate([rows, np.arange(n_docs)])
    order = np.lexsort((terms, rows))
    terms, counts, rows = terms[order], counts[order], rows[order]
    row_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_docs))]).tolist()
    post_off, docs, tf = expected_postings(terms, counts, row_off, N_WORDS, 0)
    ix = Index(post_off, docs, tf, doc_len)
    queries = [[N_WORDS - 2], [0, 1, N_WORDS - 2], [int(terms[0])], [N_WORDS - 1]]
    for k in (1, 10, 1024):
        docs_, scores, top_n = check(ctx, vocab, ix, queries, k)
        assert top_n[0] == min(k, n_docs) and top_n[3] == 0


# ---- 3. exact ties

def test_exact_ties(ctx, vocab):
    n_docs, base = 5000, 7
    # every document: words 3 (tf 2) and 9 (tf 1), the same length: every score is bit-equal
    post_off = np.zeros(N_WORDS + 1, dtype=np.uint64)
    post_off[4:] += n_docs
    post_off[10:] += n_docs
    # two levels: word 20 only in the documents i % 10 == 3
    high = np.arange(3, n_docs, 10)
    post_off[21:] += len(high)
    docs = np.concatenate([np.arange(n_docs), np.arange(n_docs), high]).astype(np.uint32) + base
    tf = np.concatenate([np.full(n_docs, 2), np.full(n_docs, 1), np.full(len(high), 4)]).astype(np.uint32)
    ix = Index(post_off, docs, tf, np.full(n_docs, 37, dtype=np.uint32), base)
    for k in (1, 7, 1024):
        d, s, top_n = check(ctx, vocab, ix, [[3, 9], [9], [3, 3, UNK, 9]], k)
        assert top_n == [k, k, k]
        for q in range(3):
            assert d[q].tolist() == list(range(base, base + k)), (k, q)
            assert len(set(s[q].view(np.uint32).tolist())) == 1
    rest = np.setdiff1d(np.arange(n_docs), high)
    for k in (len(high) - 1, len(high), len(high) + 1, 700, 1024):   # k cuts inside the lower level
        d, s, top_n = check(ctx, vocab, ix, [[3, 20], [20, 9, 3]], k)
        want = np.concatenate([high, rest])[:k] + base
        assert top_n == [k, k] and d[0].tolist() == want.tolist() and d[1].tolist() == want.tolist(), k


# ---- 4. score bits

def test_scores_in_the_lowest_byte(ctx, vocab):
    """Two score levels whose float32 bits differ only in the lowest byte, over 50 documents with one very long
    one: word 0 stands in the first 40 with tf 3, the lengths of the levels are 3000 apart at an average length of
    4.3e7, which separates the levels by 2.2e-5 to 2.5e-5 relative (more than 2 RTOL, fewer than 256 bit patterns
    where the mantissa is small).  k1 is scanned on the CPU for a value at which the float32 evaluation puts both
    levels into one block of 256 consecutive bit patterns, and at which the float64 reference separates them."""
    n_docs, n_in = 50, 40
    high = np.array([2, 5, 11, 17, 23, 30, 38])
    doc_len = np.full(n_docs, 50_000 + 3_000, dtype=np.uint32)
    doc_len[high] = 50_000
    doc_len[0] = 2**31                                       # the skew: avgdl = 4.3e7
    post_off = np.zeros(N_WORDS + 1, dtype=np.uint64)
    post_off[1:] = n_in
    docs, tf = np.arange(n_in, dtype=np.uint32), np.full(n_in, 3, dtype=np.uint32)
    low = np.setdiff1d(np.arange(1, n_in), high)
    found = None
    for k1 in np.arange(0.8, 3.0, 0.001):
        args = (post_off, docs, tf, doc_len, 0, [[0]], float(np.float32(k1)), 0.75)
        bits = scores_f32(*args)[0].view(np.uint32)
        hb, lb = int(bits[high[0]]), int(bits[low[0]])
        if hb >> 8 == lb >> 8 and 8 <= (lb & 255) and (hb & 255) <= 247:   # (a few patterns of room on both sides)
            ref = expected_scores(*args)
            if ref[0, high[0]] > (1 + 2.2 * RTOL) * ref[0, low[0]]:
                found = float(np.float32(k1))
                break
    assert found is not None
    ix = Index(post_off, docs, tf, doc_len)
    for k in (3, len(high), 10, 39, 40, 1024):
        d, s, top_n = check(ctx, vocab, ix, [[0]], k, k1=found)
        n = min(k, n_in)
        want = np.concatenate([high, low, [0]])[:n]          # the levels are exact ties inside
        assert top_n == [n] and d[0, :n].tolist() == want.tolist(), k
        got = s[0, :n].view(np.uint32)
        if n > len(high):
            last = min(n, n_in - 1) - 1                      # a document of the lower level
            assert got[0] >> 8 == got[last] >> 8 and got[0] > got[last]


def test_scores_in_the_top_byte(ctx, vocab):
    """Scores idf, idf / 4 and idf / 16, exactly: tf = 1, k1 = 1, b = 1 and lengths of 1, 7 and 31 times the average
    (64) give w = 2 idf / (1 + dl / avgdl) = 2 idf / 2, / 8, / 32.  Their bits differ in the top byte only."""
    n_a, n_b, n_c = 5, 9, 20
    n_docs = n_a + 7 * n_b + 31 * n_c                        # the others have length 0: the average is 64
    rng = np.random.default_rng(4)
    who = rng.permutation(n_docs)
    a, b_, c = np.sort(who[:n_a]), np.sort(who[n_a:n_a + n_b]), np.sort(who[n_a + n_b:n_a + n_b + n_c])
    doc_len = np.zeros(n_docs, dtype=np.uint32)
    doc_len[a], doc_len[b_], doc_len[c] = 64, 7 * 64, 31 * 64
    assert int(doc_len.sum()) == 64 * n_docs
    members = np.sort(np.concatenate([a, b_, c]))
    post_off = np.zeros(N_WORDS + 1, dtype=np.uint64)
    post_off[6:] = len(members)
    ix = Index(post_off, members.astype(np.uint32), np.ones(len(members), dtype=np.uint32), doc_len)
    order = np.concatenate([a, b_, c])
    for k in (1, n_a, n_a + 4, n_a + n_b, n_a + n_b + 1, 1024):
        d, s, top_n = check(ctx, vocab, ix, [[5]], k, k1=1.0, b=1.0)
        n = min(k, len(order))
        assert top_n == [n] and d[0, :n].tolist() == order[:n].tolist(), k
    bits = s[0, :len(order)].view(np.uint32)
    assert len(set((bits & 0xFFFFFF).tolist())) == 1 and len(set((bits >> 24).tolist())) == 3
    assert s[0, 0] == 4 * s[0, n_a] == 16 * s[0, n_a + n_b]


# ---- 5. chunks

def test_chunks_give_identical_bytes(ctx, vocab, monkeypatch):
    ix = random_index(5, 3000)
    rng = np.random.default_rng(5)
    queries = [[int(x) for x in rng.integers(0, 60, rng.integers(0, 6))] for _ in range(40)]
    queries[7], queries[39] = [], [0, 1, 2]
    row_bytes = 4 * 3000
    monkeypatch.delenv("MRG_SEARCH_ACC_BYTES", raising=False)
    d0, s0, n0 = search_dev(ctx, vocab, ix, queries, 10)
    assert ctx.search_info()["chunks"] == 1
    check_topk(d0, s0, n0, ix.ref(queries), 10, 0)
    for acc, chunks in ((40 * row_bytes, 1), (14 * row_bytes + 100, 3), (1, 40)):
        monkeypatch.setenv("MRG_SEARCH_ACC_BYTES", str(acc))
        d, s, n = search_dev(ctx, vocab, ix, queries, 10)
        info = ctx.search_info()
        assert info["chunks"] == chunks, (acc, info)
        assert n == n0 and d.tobytes() == d0.tobytes() and s.tobytes() == s0.tobytes(), acc


# ---- 6. doc_base

@pytest.mark.parametrize("base", [0, 5, "top"])
def test_doc_base(ctx, vocab, base):
    n_docs = 1500
    base = 2**32 - n_docs if base == "top" else base
    ix = random_index(6, n_docs, doc_base=base)
    queries = [[0], [1, 2, 3], [50, 51, UNK, 52]]
    d, s, top_n = check(ctx, vocab, ix, queries, 10)
    assert top_n[0] == 10 and int(d[0, :10].min()) >= base and int(d[0, :10].max()) <= base + n_docs - 1


# ---- 7. the pipeline from text

def test_pipeline_from_text(ctx):
    import mapreduce_rust_amd as M
    import torch
    from gpu_util import to_device
    text = gzip.open(os.path.join(HERE, "golden", "corpus", "gut-0.txt.gz")).read()
    t, off = to_device([text])
    ctx.job_begin(M.APP_WC, 1, M.FLAG_NO_COMPAT_DROP_LAST)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    with ctx.vocab(max_words=0) as v:
        n_words = v.size()[0]
        tok = ctx.encode(v, t.data_ptr(), off)
        n_ids = tok[-1]
        d_ids = torch.empty((n_ids,), dtype=torch.int32, device="cuda:0")
        ctx.encode(v, t.data_ptr(), off, d_ids.data_ptr(), n_ids)
        cut = list(range(0, n_ids, 256)) + [n_ids]           # documents of 256 ids
        n_docs = len(cut) - 1
        row_off, _ = ctx.term_counts(v, d_ids.data_ptr(), cut)
        E = row_off[-1]
        d_terms = torch.empty((E,), dtype=torch.int32, device="cuda:0")
        d_counts = torch.empty_like(d_terms)
        ctx.term_counts(v, d_ids.data_ptr(), cut, d_terms.data_ptr(), d_counts.data_ptr(), E)
        d_po = torch.empty((n_words + 1,), dtype=torch.int64, device="cuda:0")
        d_docs = torch.empty((E,), dtype=torch.int32, device="cuda:0")
        d_tf = torch.empty_like(d_docs)
        assert ctx.postings(v, d_terms.data_ptr(), d_counts.data_ptr(), row_off, d_po.data_ptr(), d_docs.data_ptr(),
                            d_tf.data_ptr(), E) == E
        torch.cuda.synchronize()
        doc_len = np.diff(np.array(cut, dtype=np.int64)).astype(np.uint32)
        ix = Index(d_po.cpu().numpy().view(np.uint64), d_docs.cpu().numpy().view(np.uint32),
                   d_tf.cpu().numpy().view(np.uint32), doc_len)   # the host copies of the device arrays
        assert ix.n_docs == n_docs > 100 and ix.n_entries == E
        texts = [b"Elizabeth Darcy", b"truth universally acknowledged", b"Pemberley love heart night", b"zzzunknownzzz white", b""]
        words = v.words()
        known = set(words)
        qt, qoff = to_device(texts)
        qtok = ctx.encode(v, qt.data_ptr(), qoff)
        d_q = torch.empty((max(qtok[-1], 1),), dtype=torch.int32, device="cuda:0")
        ctx.encode(v, qt.data_ptr(), qoff, d_q.data_ptr(), qtok[-1])
        torch.cuda.synchronize()
        q_ids = d_q.cpu().numpy().view(np.uint32)
        queries = [q_ids[qtok[i]:qtok[i + 1]].tolist() for i in range(len(texts))]
        assert [len(q) for q in queries] == [2, 3, 4, 2, 0]
        for q, txt in zip(queries, texts):                   # the ids are those of the query's words
            assert [UNK if i == UNK else words[i] for i in q] == [w if w in known else UNK for w in txt.split()]
        assert UNK in queries[3] and sum(i != UNK for q in queries for i in q) >= 6
        # the search reads the arrays postings() wrote and the ids encode() wrote: nothing in between
        k = 10
        fill = SENTINEL - (1 << 32)
        o_d = torch.full((len(texts) * k,), fill, dtype=torch.int32, device="cuda:0")
        o_s = torch.full((len(texts) * k,), fill, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        top_n = ctx.search(v, d_po.data_ptr(), d_docs.data_ptr(), d_tf.data_ptr(), E, ix.d_doc_len.data_ptr(), n_docs,
                           d_q.data_ptr(), qtok, k, o_d.data_ptr(), o_s.data_ptr())
        torch.cuda.synchronize()
        got_d = o_d.cpu().numpy().view(np.uint32).reshape(len(texts), k)
        got_s = o_s.cpu().numpy().view(np.float32).reshape(len(texts), k)
        ref = ix.ref(queries)
        check_topk(got_d, got_s, top_n, ref, k, 0)
        assert top_n[4] == 0 and top_n[0] == k
        best = int(got_d[1, 0])                              # the best document of query 1 holds one of its words
        ids_host = d_ids.cpu().numpy().view(np.uint32)
        assert set(queries[1]) & set(ids_host[cut[best]:cut[best + 1]].tolist())
    del t, qt


# ---- 8. refusals

def raw_call(context, voc, ix, offsets, **over):
    """mrg_vocab_search through ctypes with any argument replaced (NULL host pointers included)"""
    from mapreduce_rust_amd import native
    L = native.load()
    n = len(offsets) - 1
    a = dict(ctx=context.h, v=voc.h, post_off=ix.d_post_off.data_ptr(), docs=ix.p_docs, tf=ix.p_tf, n_entries=ix.n_entries,
             doc_len=ix.d_doc_len.data_ptr(), n_docs=ix.n_docs, doc_base=ix.doc_base, q_ids=None,
             q_off=(C.c_uint64 * len(offsets))(*offsets), n_queries=n, k1=1.2, b=0.75, k=10, top_docs=None, top_scores=None, top=None)
    a.update(over)
    rc = L.mrg_vocab_search(a["ctx"], a["v"], a["post_off"], a["docs"], a["tf"], a["n_entries"], a["doc_len"], a["n_docs"],
                            a["doc_base"], a["q_ids"], a["q_off"], a["n_queries"], a["k1"], a["b"], a["k"], a["top_docs"],
                            a["top_scores"], a["top"])
    return rc, L.mrg_last_error().decode()


def test_refused_before_any_device_work(ctx, vocab, coll):
    import mapreduce_rust_amd as M
    import torch
    EINVAL = M.native.EINVAL
    queries = [[0, 1], [2]]
    ids, q_off = lay_queries(queries)
    t = dev_u32(ids)
    k = 10
    fill = SENTINEL - (1 << 32)
    out = torch.full((2, 2 * k + 4), fill, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    base = dict(q_ids=t.data_ptr(), top_docs=out[0].data_ptr(), top_scores=out[1].data_ptr())
    cases = [
        (dict(v=None), "vocabulary"),
        (dict(post_off=None), "d_post_off"),
        (dict(q_off=None), "offsets"),
        (dict(top_docs=None), "output"),
        (dict(top_scores=None), "output"),
        (dict(top=None), "output"),
        (dict(docs=None), "null d_docs"),
        (dict(tf=None), "null d_docs"),
        (dict(doc_len=None), "null d_docs"),
        (dict(docs=coll.p_docs + 2), "aligned"),
        (dict(tf=coll.p_tf + 1), "aligned"),
        (dict(doc_len=coll.d_doc_len.data_ptr() + 2), "aligned"),
        (dict(q_ids=t.data_ptr() + 1), "aligned"),
        (dict(top_docs=out[0].data_ptr() + 2), "aligned"),
        (dict(top_scores=out[1].data_ptr() + 3), "aligned"),
        (dict(post_off=coll.d_post_off.data_ptr() + 4), "8-byte"),
        (dict(q_off=(C.c_uint64 * 3)(0, 3, 2)), "non-decreasing"),
        (dict(doc_base=2**32 - coll.n_docs + 1), "32 bits"),
        (dict(n_entries=2**32), "entries"),
        (dict(k=0), "k = 0"),
        (dict(k=1025), "k = 1025"),
        (dict(k1=-0.5), "k1"),
        (dict(k1=1000.5), "k1"),
        (dict(k1=float("nan")), "k1"),
        (dict(b=-0.1), "b ="),
        (dict(b=1.01), "b ="),
        (dict(b=float("nan")), "b ="),
        (dict(q_off=(C.c_uint64 * 3)(0, 2, 2**20 + 1)), "query ids"),
    ]
    for over, what in cases:
        top = (C.c_uint32 * 2)(77, 77)
        args = dict(base)
        args.update(over)
        if "top" not in over:
            args["top"] = top
        rc, msg = raw_call(ctx, vocab, coll, q_off, **args)
        assert rc == EINVAL and what in msg, (over, rc, msg)
        assert list(top) == [77, 77], over
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "an output was written by a refused call"
    top = (C.c_uint32 * 2)(77, 77)
    rc, msg = raw_call(ctx, vocab, coll, q_off, top=top, **base)   # then a good call on the same context
    assert rc == 0 and list(top) == [10, 10]
    del t


def broken(ix, docs=None, post_off=None):
    return Index(ix.post_off if post_off is None else post_off, ix.docs if docs is None else docs, ix.tf, ix.doc_len,
                 ix.doc_base)


def test_refused_on_the_device(ctx, vocab):
    import mapreduce_rust_amd as M
    T = consts()[0]
    EINVAL = M.native.EINVAL
    n_docs, base = 3 * T, 100
    ix = random_index(8, n_docs, mean_len=4, doc_base=base)
    # word 0 gets a long list: every document but the last few, so that its segment spans three tiles
    keep = ix.docs[int(ix.post_off[1]):]
    w0 = np.arange(n_docs - 5, dtype=np.uint32) + base
    post_off = np.concatenate([[0], ix.post_off[1:] - ix.post_off[1] + len(w0)]).astype(np.uint64)
    docs = np.concatenate([w0, keep]).astype(np.uint32)
    tf = np.concatenate([np.ones(len(w0), dtype=np.uint32), ix.tf[int(ix.post_off[1]):]])
    good = Index(post_off, docs, tf, ix.doc_len, base)
    queries = [[5, 0, 7], [UNK], [0, 9]]
    check(ctx, vocab, good, queries, 10)                     # (the pool has seen these sizes)
    before = ctx.pool_stats()

    def refused(ixb, qs, what, first=0):
        ids, q_off = lay_queries(qs, first)
        t = dev_u32(ids)
        with pytest.raises(M.MrgError) as ei:
            search_raw(ctx, vocab, ixb, t, q_off, 10)
        assert ei.value.code == EINVAL and what in str(ei.value), (what, str(ei.value))
        assert ctx.pool_stats()[0] == before[0], "scratch not returned after an error"
        del t

    # a bad query id: the smallest index, counted from the start of d_q_ids
    refused(good, [[5, N_WORDS + 3], [0xFFFFFFFE, 1]], "index 4 ", first=3)
    refused(good, [[], [0], [UNK, N_WORDS]], "index 2 ")
    # a posting out of the document range: the smallest position; above and below the collection
    p1, p2 = T + 17, 2 * T + 3
    for bad in (base + n_docs, base - 1, 0xFFFFFFFF):
        d = docs.copy()
        d[p2], d[p1] = bad, bad
        refused(broken(good, docs=d), queries, "posting %d:" % p1)
    # documents that repeat or descend, inside a tile and at a tile's first posting
    for p, val in ((p1, docs[p1 - 1]), (T, docs[T - 1]), (2 * T, docs[2 * T - 2]), (5, docs[3])):
        d = docs.copy()
        d[p] = val
        later = min(p + 1000, len(w0) - 1)
        d[later] = d[later - 1]
        refused(broken(good, docs=d), queries, "posting %d:" % p)
    # the first posting of a word is compared with nothing: word 1's list may start below word 0's last document
    assert docs[len(w0)] < docs[len(w0) - 1]
    # d_post_off descending, or past the entries, for a queried word
    po = post_off.copy()
    po[8] = po[7] - 1
    refused(broken(good, post_off=po), queries, "d_post_off of word 7")
    po = post_off.copy()
    po[10] = len(docs) + 1
    refused(broken(good, post_off=po), queries, "d_post_off of word 9")
    check(ctx, vocab, broken(good, post_off=po), [[5, 0, 7]], 10, ref=good.ref([[5, 0, 7]]))   # word 9 not queried: not read
    # then good calls on the same context succeed, and nothing is outstanding
    check(ctx, vocab, good, queries, 10)
    assert ctx.pool_stats()[0] == before[0]


def test_empty_cases(ctx, vocab, coll):
    import mapreduce_rust_amd as M
    import torch
    some = dev_u32(np.array([0, 1, UNK, UNK], dtype=np.uint32))
    out = torch.full((2, 64), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    o = (out[0].data_ptr(), out[1].data_ptr())
    p = (coll.d_post_off.data_ptr(), coll.p_docs, coll.p_tf)
    dl = coll.d_doc_len.data_ptr()
    assert ctx.search(vocab, *p, coll.n_entries, dl, coll.n_docs, some.data_ptr(), [0], 10, *o) == []          # no queries
    assert ctx.search(vocab, *p, coll.n_entries, dl, coll.n_docs, some.data_ptr(), [2, 2, 2], 10, *o) == [0, 0]  # all empty
    assert ctx.search(vocab, *p, coll.n_entries, dl, coll.n_docs, None, [0, 0], 10, *o) == [0]
    assert ctx.search(vocab, *p, coll.n_entries, dl, coll.n_docs, some.data_ptr(), [2, 4], 10, *o) == [0]        # all UNK
    assert ctx.search(vocab, *p, coll.n_entries, dl, 0, some.data_ptr(), [0, 2], 10, *o) == [0]                  # no documents
    zero = torch.zeros((N_WORDS + 1,), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.search(vocab, zero.data_ptr(), None, None, 0, None, coll.n_docs, some.data_ptr(), [0, 2, 4], 10, *o) == [0, 0]
    with ctx.vocab_from_text(b"") as v0:                     # an empty vocabulary: every id must be MRG_ID_UNK
        assert ctx.search(v0, zero.data_ptr(), None, None, 0, None, 5, some.data_ptr(), [2, 4], 10, *o) == [0]
        with pytest.raises(M.MrgError) as ei:
            ctx.search(v0, zero.data_ptr(), None, None, 0, None, 5, some.data_ptr(), [0, 2], 10, *o)
        assert ei.value.code == M.native.EINVAL and "index 0 " in str(ei.value)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()


# ---- 9. a vocabulary of another device

def test_vocabulary_of_another_device(ctx, coll):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    with M.Context(1) as other:
        with make_vocab(other, N_WORDS) as v1:
            ids, q_off = lay_queries([[0, 1]])
            t = dev_u32(ids)
            with pytest.raises(M.MrgError) as ei:
                search_raw(ctx, v1, coll, t, q_off, 10)
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
            assert (search_raw.last[0] == SENTINEL).all() and (search_raw.last[1] == SENTINEL).all()
