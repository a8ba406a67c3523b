"""GPU tests of the sharded search: mrg_vocab_stats_add, mrg_vocab_search_shard and mrg_search_merge (k_merge.hip,
the collection-statistics path of k_search.hip's host layer).

The claim under test is an identity: the shards of a collection, scored with the collection's statistics and
merged, give the bytes -- documents, score bits, top_n -- of mrg_vocab_search over the index in one piece, which
tests/test_gpu_search.py holds to the float64 reference.  The shards are cut on the host (shard_util.split_index);
the merge alone is checked against shard_util.merge_twin, a numpy.lexsort.  Every call goes twice into
sentinel-filled rows with slack and must give identical bytes.  The merge stages a query's rows in LDS when
n_shards * k_in is at most native.MERGE_LDS_KEYS and reads global memory otherwise; the select of the search works
on tiles of 1024 documents: the sweeps below are sized by those numbers.  Every bad input here is one the
contract answers with a status code."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from postings_util import expected_postings
from search_util import SENTINEL, SLACK, UNK, Index, check_topk, dev_u32, lay_queries, search_dev
from shard_util import (coll_stats, filled, host_u32, merge_dev, merge_raw, merge_twin, shards_search_raw, split_index,
                        stats_dev)
from terms_util import make_vocab

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_WORDS = 2000
CUTS = [0, 1, 64, 1025, 1025, 3000, 5000]


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
    row_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_docs))]).astype(np.int64)
    doc_len = (np.bincount(rows, weights=counts, minlength=n_docs).astype(np.int64) + rng.integers(0, 5, n_docs))
    return terms, counts, row_off, doc_len.astype(np.uint32)


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


class Coll:
    """the collection of the tests: its CSR, the index in one piece, the queries, and the one-piece results by k"""

    def __init__(self, ctx, vocab):
        self.csr = random_csr(np.random.default_rng(1), 5000, N_WORDS, 12)
        terms, counts, row_off, doc_len = self.csr
        self.whole = Index(*expected_postings(terms, counts, row_off, N_WORDS, 0), doc_len, 0)
        self.queries = mixed_queries(self.whole, np.random.default_rng(2))
        self.ids, self.q_off = lay_queries(self.queries)
        self.d_ids = dev_u32(self.ids)
        self.ref = self.whole.ref(self.queries)
        self.one = {k: search_dev(ctx, vocab, self.whole, self.queries, k) for k in (1, 10, 1024)}
        hits = (self.ref > 0).sum(axis=1)
        assert (hits == 0).sum() >= 5 and ((hits > 0) & (hits < 20)).any() and (hits > 1024).any()


@pytest.fixture(scope="module")
def coll(ctx, vocab):
    return Coll(ctx, vocab)


def shards_dev(ctx, v, shards, df, stats, d_ids, q_off, k, k1=1.2, b=0.75):
    """every shard searched twice into its slice: identical bytes, nothing written from top_n on or into the slack;
    returns the device buffers and the counts, ready for the merge"""
    d1, s1, n1 = shards_search_raw(ctx, v, shards, df, stats, d_ids, q_off, k, k1, b)
    d2, s2, n2 = shards_search_raw(ctx, v, shards, df, stats, d_ids, q_off, k, k1, b)
    a, bb = host_u32(d1), host_u32(s1)
    assert n1 == n2 and (a == host_u32(d2)).all() and (bb == host_u32(s2)).all(), "two calls differ"
    rows = len(n1)
    assert (a[rows * k:] == SENTINEL).all() and (bb[rows * k:] == SENTINEL).all(), "wrote past the last row"
    for r in range(rows):
        assert 0 <= n1[r] <= k
        assert (a[r * k + n1[r]:(r + 1) * k] == SENTINEL).all() and (bb[r * k + n1[r]:(r + 1) * k] == SENTINEL).all(), r
    return d1, s1, n1


def same_rows(got, want):
    """(docs, scores or bits, top_n) of two paths: the same bytes"""
    gd, gs, gn = got
    wd, ws, wn = want
    assert list(gn) == list(wn), ("top_n", list(gn), list(wn))
    assert np.asarray(gd).view(np.uint32).tobytes() == np.asarray(wd).view(np.uint32).tobytes(), "documents differ"
    assert np.asarray(gs).view(np.uint32).tobytes() == np.asarray(ws).view(np.uint32).tobytes(), "score bits differ"


# ---- 1. one shard is the search

def test_one_shard_is_the_search(ctx, vocab, coll):
    ix = coll.whole
    df, stats = stats_dev(ctx, vocab, [ix])
    assert (host_u32(df).view(np.uint64)[:N_WORDS] == np.diff(ix.post_off)).all()
    assert stats == (ix.n_docs, int(ix.doc_len.astype(np.int64).sum()))
    nq = len(coll.queries)
    for k in (1, 10, 1024):
        d, s, n = shards_dev(ctx, vocab, [ix], df, stats, coll.d_ids, coll.q_off, k)
        same_rows((host_u32(d)[:nq * k], host_u32(s)[:nq * k], n), coll.one[k])
    info = ctx.search_info()                                 # the diagnostics are those of the last search of either kind
    assert info["queries"] == nq and info["positions"] == sum(len(q) for q in coll.queries)


# ---- 2. split = whole

def test_split_equals_whole(ctx, vocab, coll):
    shards = split_index(coll.csr, CUTS, N_WORDS)
    assert [s.n_docs for s in shards] == [1, 63, 961, 0, 1975, 2000]
    want_df, want_n, want_sum = coll_stats([coll.whole])
    assert sum(s.n_entries for s in shards) == coll.whole.n_entries
    for order in (None, [4, 0, 5, 3, 2, 1]):
        df, stats = stats_dev(ctx, vocab, shards, order)
        assert (host_u32(df).view(np.uint64)[:N_WORDS].astype(np.int64) == want_df).all(), order
        assert stats == (want_n, want_sum), order
    nq = len(coll.queries)
    for k in (1, 10, 1024):
        d, s, n = shards_dev(ctx, vocab, shards, df, stats, coll.d_ids, coll.q_off, k)
        assert n[3 * nq:4 * nq] == [0] * nq                  # the empty shard
        got = merge_dev(ctx, len(shards), nq, k, d, s, n, k)
        one_d, one_s, one_n = coll.one[k]
        same_rows(got, (one_d, one_s, one_n))
        check_topk(got[0], got[1].view(np.float32), got[2], coll.ref, k, 0)
    # a shard searched with its own statistics gives other bytes: the identity above rests on the statistics
    big = shards[5]
    df5, st5 = stats_dev(ctx, vocab, [big])
    d, s, n = shards_dev(ctx, vocab, [big], df, stats, coll.d_ids, coll.q_off, 10)
    d5, s5, n5 = shards_dev(ctx, vocab, [big], df5, st5, coll.d_ids, coll.q_off, 10)
    assert n == n5 and host_u32(s).tobytes() != host_u32(s5).tobytes()


# ---- 3. ties across shards

def test_ties_across_shards(ctx, vocab):
    n_docs, base = 5000, 7
    # the collection of test_exact_ties: every document holds words 3 (tf 2) and 9 (tf 1) and has the same length;
    # word 20 (tf 4) stands only in the documents i % 10 == 3
    high = np.arange(3, n_docs, 10)
    is_high = np.zeros(n_docs, dtype=bool)
    is_high[high] = True
    lens = np.where(is_high, 3, 2)
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    terms = np.concatenate([[3, 9, 20] if h else [3, 9] for h in is_high]).astype(np.uint32)
    counts = np.concatenate([[2, 1, 4] if h else [2, 1] for h in is_high]).astype(np.uint32)
    csr = (terms, counts, row_off, np.full(n_docs, 37, dtype=np.uint32))
    whole = Index(*expected_postings(terms, counts, row_off, N_WORDS, base), csr[3], base)
    shards = split_index(csr, [0, 333, 1501, 4999, 5000], N_WORDS, base)
    assert [s.doc_base for s in shards] == [7, 340, 1508, 5006]
    df, stats = stats_dev(ctx, vocab, shards)
    rest = np.setdiff1d(np.arange(n_docs), high)

    def run(queries, k):
        ids, q_off = lay_queries(queries)
        t = dev_u32(ids)
        d, s, n = shards_dev(ctx, vocab, shards, df, stats, t, q_off, k)
        got = merge_dev(ctx, len(shards), len(queries), k, d, s, n, k)
        same_rows(got, search_dev(ctx, vocab, whole, queries, k))
        del t
        return got

    for k in (1, 7, 1024):
        d, s, n = run([[3, 9], [9], [3, 3, UNK, 9]], k)
        assert n == [k, k, k]
        for q in range(3):
            assert d[q].tolist() == list(range(base, base + k)), (k, q)
            assert len(set(s[q].tolist())) == 1
    for k in (len(high) - 1, len(high), len(high) + 1, 700, 1024):   # k cuts inside a level
        d, s, n = run([[3, 20], [20, 9, 3]], k)
        want = np.concatenate([high, rest])[:k] + base
        assert n == [k, k] and d[0].tolist() == want.tolist() and d[1].tolist() == want.tolist(), k


# ---- 4. the merge alone

LEVELS = np.sort(np.concatenate([np.float32([1e-38, 1e-30, 0.5, 1.0, 3.25, 7e20, np.inf]),
                                 np.float32(1.0) + np.arange(1, 30, dtype=np.float32) * np.float32(2.0 ** -23)])
                 .astype(np.float32).view(np.uint32))[::-1]   # score bits, descending
N_DOCS_M = 60                                                # few documents: the same (score, document) in many shards


def host_rows(seed, n_shards, nq, k_in, counts=None):
    """rows in the order of the search over LEVELS x N_DOCS_M: (docs, bits, counts), unused cells SENTINEL; the
    counts cycle through 0, partial and full unless given"""
    rng = np.random.default_rng(seed)
    combos = len(LEVELS) * N_DOCS_M
    assert k_in <= combos
    docs = np.full((n_shards * nq, k_in), SENTINEL, dtype=np.uint32)
    bits = np.full((n_shards * nq, k_in), SENTINEL, dtype=np.uint32)
    cnt = []
    for r in range(n_shards * nq):
        n = (0, int(rng.integers(0, k_in + 1)), k_in)[(r + seed) % 3] if counts is None else counts[r]
        c = np.sort(rng.choice(combos, n, replace=False))    # level ascending = score descending, then document
        docs[r, :n], bits[r, :n] = c % N_DOCS_M + 100, LEVELS[c // N_DOCS_M]
        cnt.append(n)
    return docs, bits, cnt


def merge_case(ctx, docs, bits, cnt, n_shards, nq, k_in, k_out):
    t_d, t_b = dev_u32(docs.ravel()), dev_u32(bits.ravel())
    got = merge_dev(ctx, n_shards, nq, k_in, t_d, t_b, cnt, k_out)
    want = merge_twin(docs, bits, cnt, n_shards, nq, k_in, k_out)
    same_rows(got, want)
    total = [sum(cnt[s * nq + q] for s in range(n_shards)) for q in range(nq)]
    assert got[2] == [min(k_out, t) for t in total]
    del t_d, t_b
    return got


@pytest.mark.parametrize("n_shards", [1, 2, 3, 64])
def test_merge_alone(ctx, n_shards):
    nq = 3
    for k_in in (1, 7, 1024):
        docs, bits, cnt = host_rows(n_shards + k_in, n_shards, nq, k_in)
        if n_shards * nq >= 3:
            assert 0 in cnt and k_in in cnt
        for k_out in (1, 10, 1024):
            merge_case(ctx, docs, bits, cnt, n_shards, nq, k_in, k_out)
    # all rows empty, and rows of one entry
    docs, bits, _ = host_rows(5, n_shards, nq, 7, counts=[7] * (n_shards * nq))
    assert merge_case(ctx, docs, bits, [0] * (n_shards * nq), n_shards, nq, 7, 10)[2] == [0, 0, 0]
    merge_case(ctx, docs, bits, [1] * (n_shards * nq), n_shards, nq, 7, 1024)


def test_merge_ties_decided_by_shard(ctx):
    # three shards hold the same two (score, document) pairs: the merged row repeats each pair, the shards in order
    one = np.float32(1.0).view(np.uint32)
    docs = np.array([[5, 9]] * 3, dtype=np.uint32)
    bits = np.full((3, 2), one, dtype=np.uint32)
    d, b, n = merge_case(ctx, docs, bits, [2, 2, 2], 3, 1, 2, 5)
    assert n == [5] and d[0].tolist() == [5, 5, 5, 9, 9] and (b[0] == one).all()
    # equal scores across shards: by document, wherever it stands
    docs = np.array([[8, 30], [2, 31], [1, 8]], dtype=np.uint32)
    d, b, n = merge_case(ctx, docs, bits, [2, 2, 2], 3, 1, 2, 1024)
    assert n == [6] and d[0, :6].tolist() == [1, 2, 8, 8, 30, 31]
    # the output of a merge is a valid input row: six shards that share no (score, document), merged in two stages
    rng = np.random.default_rng(11)
    rows_d, rows_b = np.zeros((12, 40), dtype=np.uint32), np.zeros((12, 40), dtype=np.uint32)
    for q in range(2):
        c = np.sort(rng.permutation(len(LEVELS) * N_DOCS_M)[:6 * 40].reshape(6, 40), axis=1)
        rows_d[q::2], rows_b[q::2] = c % N_DOCS_M + 100, LEVELS[c // N_DOCS_M]
    cnt = [40, 40, 17, 40, 40, 0, 40, 3, 40, 40, 1, 40]
    t_d, t_b = dev_u32(rows_d.ravel()), dev_u32(rows_b.ravel())
    all_d, all_b, all_n = merge_dev(ctx, 6, 2, 40, t_d, t_b, cnt, 64)
    half = [merge_dev(ctx, 3, 2, 40, dev_u32(rows_d[6 * h:6 * h + 6].ravel()), dev_u32(rows_b[6 * h:6 * h + 6].ravel()),
                      cnt[6 * h:6 * h + 6], 64) for h in (0, 1)]
    st_d = np.concatenate([half[0][0], half[1][0]])
    st_b = np.concatenate([half[0][1], half[1][1]])
    got = merge_dev(ctx, 2, 2, 64, dev_u32(st_d.ravel()), dev_u32(st_b.ravel()), half[0][2] + half[1][2], 64)
    same_rows(got, (all_d, all_b, all_n))


def test_merge_on_both_sides_of_the_lds_limit(ctx):
    from mapreduce_rust_amd import native
    lim, max_k, max_s = native.MERGE_LDS_KEYS, native.SEARCH_MAX_K, native.SEARCH_MAX_SHARDS
    assert lim % max_k == 0 and lim % max_s == 0
    shapes = [(lim // max_k, max_k), (lim // max_k, max_k - 1), (lim // max_k + 1, max_k),
              (max_s, lim // max_s), (max_s, lim // max_s - 1), (max_s, lim // max_s + 1), (max_s, max_k)]
    assert sorted({s * k > lim for s, k in shapes}) == [False, True]
    for n_shards, k_in in shapes:
        docs, bits, cnt = host_rows(n_shards * k_in, n_shards, 2, k_in)
        full = host_rows(1 + n_shards * k_in, n_shards, 2, k_in, counts=[k_in] * (2 * n_shards))
        for k_out in (10, 1024):
            merge_case(ctx, docs, bits, cnt, n_shards, 2, k_in, k_out)
            merge_case(ctx, *full, n_shards, 2, k_in, k_out)


# ---- 5. refusals

def raw(name, order, args, **over):
    from mapreduce_rust_amd import native
    L = native.load()
    a = dict(args)
    a.update(over)
    rc = getattr(L, name)(*[a[key] for key in order])
    return rc, L.mrg_last_error().decode()


STATS_ARGS = ("ctx", "v", "post_off", "doc_len", "n_docs", "df", "coll")
SHARD_ARGS = ("ctx", "v", "post_off", "docs", "tf", "n_entries", "doc_len", "n_docs", "doc_base", "df", "coll_docs",
              "coll_sum_len", "q_ids", "q_off", "n_queries", "k1", "b", "k", "top_docs", "top_scores", "top")
MERGE_ARGS = ("ctx", "n_shards", "n_queries", "k_in", "in_docs", "in_scores", "in_top_n", "k_out", "top_docs", "top_scores", "top")


def test_refused_before_any_device_work(ctx, vocab, coll):
    import mapreduce_rust_amd as M
    import torch
    EINVAL = M.native.EINVAL
    ix = coll.whole
    df, stats = stats_dev(ctx, vocab, [ix])
    queries = [[0, 1], [2]]
    ids, q_off = lay_queries(queries)
    t = dev_u32(ids)
    k = 10
    out = torch.full((2, 2 * k + 4), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    zero_df = torch.zeros((N_WORDS,), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    # mrg_vocab_stats_add
    s_args = dict(ctx=ctx.h, v=vocab.h, post_off=ix.d_post_off.data_ptr(), doc_len=ix.d_doc_len.data_ptr(), n_docs=ix.n_docs,
                  df=zero_df.data_ptr(), coll=None)
    for over, what in [(dict(ctx=None), "context"), (dict(v=None), "vocabulary"), (dict(post_off=None), "d_post_off"),
                       (dict(df=None), "d_df"), (dict(coll=None), "h_coll"), (dict(doc_len=None), "d_doc_len"),
                       (dict(post_off=ix.d_post_off.data_ptr() + 4), "8-byte"), (dict(df=zero_df.data_ptr() + 4), "8-byte"),
                       (dict(doc_len=ix.d_doc_len.data_ptr() + 2), "4-byte")]:
        h = (C.c_uint64 * 2)(5, 6)
        a = dict(s_args, coll=h)
        a.update(over)
        rc, msg = raw("mrg_vocab_stats_add", STATS_ARGS, a)
        assert rc == EINVAL and what in msg, (over, rc, msg)
        assert list(h) == [5, 6], over
    torch.cuda.synchronize()
    assert (zero_df.cpu().numpy() == 0).all(), "d_df was written by a refused call"
    h = (C.c_uint64 * 2)(5, 6)
    assert raw("mrg_vocab_stats_add", STATS_ARGS, s_args, coll=h)[0] == 0 and list(h) == [5 + stats[0], 6 + stats[1]]
    assert raw("mrg_vocab_stats_add", STATS_ARGS, s_args, coll=h, n_docs=0, doc_len=None)[0] == 0   # no documents: valid
    assert list(h) == [5 + stats[0], 6 + stats[1]]

    # mrg_vocab_search_shard: the refusals of the search, and its own
    sh_args = dict(ctx=ctx.h, v=vocab.h, post_off=ix.d_post_off.data_ptr(), docs=ix.p_docs, tf=ix.p_tf, n_entries=ix.n_entries,
                   doc_len=ix.d_doc_len.data_ptr(), n_docs=ix.n_docs, doc_base=0, df=df.data_ptr(), coll_docs=stats[0],
                   coll_sum_len=stats[1], q_ids=t.data_ptr(), q_off=(C.c_uint64 * 3)(*q_off), n_queries=2, k1=1.2, b=0.75, k=k,
                   top_docs=out[0].data_ptr(), top_scores=out[1].data_ptr(), top=None)
    cases = [
        (dict(ctx=None), "context"), (dict(v=None), "vocabulary"), (dict(post_off=None), "d_post_off"),
        (dict(q_off=None), "offsets"), (dict(top_docs=None), "output"), (dict(top_scores=None), "output"),
        (dict(top=None), "output"), (dict(docs=None), "null d_docs"), (dict(doc_len=None), "null d_docs"),
        (dict(docs=ix.p_docs + 2), "aligned"), (dict(top_scores=out[1].data_ptr() + 3), "aligned"),
        (dict(post_off=ix.d_post_off.data_ptr() + 4), "8-byte"), (dict(q_off=(C.c_uint64 * 3)(0, 3, 2)), "non-decreasing"),
        (dict(doc_base=2**32 - ix.n_docs + 1), "32 bits"), (dict(n_entries=2**32), "entries"),
        (dict(k=0), "k = 0"), (dict(k=1025), "k = 1025"), (dict(k1=float("nan")), "k1"), (dict(b=1.01), "b ="),
        (dict(q_off=(C.c_uint64 * 3)(0, 2, 2**20 + 1)), "query ids"),
        (dict(df=None), "d_df"), (dict(df=df.data_ptr() + 4), "d_df"),
        (dict(coll_docs=ix.n_docs - 1), "coll_docs"), (dict(coll_docs=0), "coll_docs"), (dict(coll_docs=2**32 + 1), "coll_docs"),
    ]
    for over, what in cases:
        top = (C.c_uint32 * 2)(77, 77)
        a = dict(sh_args, top=top)
        a.update(over)
        rc, msg = raw("mrg_vocab_search_shard", SHARD_ARGS, a)
        assert rc == EINVAL and what in msg, (over, rc, msg)
        assert list(top) == [77, 77], over
    torch.cuda.synchronize()
    assert (host_u32(out) == SENTINEL).all(), "an output was written by a refused call"
    top = (C.c_uint32 * 2)(77, 77)
    assert raw("mrg_vocab_search_shard", SHARD_ARGS, sh_args, top=top)[0] == 0 and list(top) == [10, 10]
    top = (C.c_uint32 * 2)(77, 77)                           # a collection of 2^32 documents is in range
    assert raw("mrg_vocab_search_shard", SHARD_ARGS, sh_args, top=top, coll_docs=2**32)[0] == 0 and list(top) == [10, 10]

    # mrg_search_merge
    rows_d, rows_b, _ = host_rows(3, 2, 2, k, counts=[k] * 4)
    in_d, in_b = dev_u32(rows_d.ravel()), dev_u32(rows_b.ravel())
    out.fill_(SENTINEL - (1 << 32))
    torch.cuda.synchronize()
    m_args = dict(ctx=ctx.h, n_shards=2, n_queries=2, k_in=k, in_docs=in_d.data_ptr(), in_scores=in_b.data_ptr(),
                  in_top_n=(C.c_uint32 * 4)(k, 3, 0, 0), k_out=k, top_docs=out[0].data_ptr(), top_scores=out[1].data_ptr(), top=None)
    cases = [
        (dict(ctx=None), "context"), (dict(in_docs=None), "input"), (dict(in_scores=None), "input"), (dict(in_top_n=None), "input"),
        (dict(top_docs=None), "output"), (dict(top_scores=None), "output"), (dict(top=None), "output"),
        (dict(in_docs=in_d.data_ptr() + 2), "aligned"), (dict(in_scores=in_b.data_ptr() + 1), "aligned"),
        (dict(top_docs=out[0].data_ptr() + 2), "aligned"), (dict(top_scores=out[1].data_ptr() + 3), "aligned"),
        (dict(n_shards=0), "n_shards = 0"), (dict(n_shards=65), "n_shards = 65"),
        (dict(k_in=0), "k_in = 0"), (dict(k_in=1025), "k_in = 1025"), (dict(k_out=0), "k_out = 0"), (dict(k_out=1025), "k_out = 1025"),
        (dict(in_top_n=(C.c_uint32 * 4)(k, 3, k + 1, k)), "h_in_top_n[2] = 11"),
        (dict(n_shards=64, n_queries=2**16, k_in=1024), "input entries"),
    ]
    for over, what in cases:
        top = (C.c_uint32 * 2)(77, 77)
        a = dict(m_args, top=top)
        a.update(over)
        rc, msg = raw("mrg_search_merge", MERGE_ARGS, a)
        assert rc == EINVAL and what in msg, (over, rc, msg)
        assert list(top) == [77, 77], over
    torch.cuda.synchronize()
    assert (host_u32(out) == SENTINEL).all(), "an output was written by a refused call"
    top = (C.c_uint32 * 2)(77, 77)
    assert raw("mrg_search_merge", MERGE_ARGS, m_args, top=top)[0] == 0 and list(top) == [10, 3]
    assert ctx.search_merge(2, 0, k, in_d.data_ptr(), in_b.data_ptr(), [], k, out[0].data_ptr(), out[1].data_ptr()) == []
    del t, in_d, in_b


def test_refused_on_the_device(ctx, vocab, coll):
    import mapreduce_rust_amd as M
    import torch
    EINVAL = M.native.EINVAL
    ix = coll.whole
    df, stats = stats_dev(ctx, vocab, [ix])
    queries = [[5, 0, 7], [UNK], [0, 9]]
    ids, q_off = lay_queries(queries)
    t = dev_u32(ids)
    shards_dev(ctx, vocab, [ix], df, stats, t, q_off, 10)    # (the pool has seen these sizes)
    before = ctx.pool_stats()

    def refused(call, what):
        with pytest.raises(M.MrgError) as ei:
            call()
        assert ei.value.code == EINVAL and what in str(ei.value), (what, str(ei.value))
        assert ctx.pool_stats()[0] == before[0], "scratch not returned after an error"

    # mrg_vocab_stats_add: offsets that descend, the smallest word
    po = ix.post_off.copy()
    po[8], po[31] = po[7] - 1, po[30] - 2
    bad = torch.from_numpy(po.view(np.int64).copy()).to("cuda:0")
    scratch_df = torch.zeros((N_WORDS,), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    refused(lambda: ctx.stats_add(vocab, bad.data_ptr(), ix.d_doc_len.data_ptr(), ix.n_docs, scratch_df.data_ptr()), "word 7:")

    # mrg_vocab_search_shard: d_df of a queried word below the shard's own df, and above the collection's documents
    host_df = host_u32(df).view(np.uint64)[:N_WORDS].copy()

    def with_df(word, value):
        d = host_df.copy()
        d[word] = value
        td = torch.from_numpy(d.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        return lambda: shards_search_raw(ctx, vocab, [ix], td, stats, t, q_off, 10)

    refused(with_df(7, int(host_df[7]) - 1), "d_df of word 7:")
    refused(with_df(9, stats[0] + 1), "d_df of word 9:")
    ok = with_df(11, 0)()                                    # word 11 is not queried: its d_df is not read
    assert ok[2] == shards_search_raw(ctx, vocab, [ix], df, stats, t, q_off, 10)[2]
    refused(lambda: shards_search_raw(ctx, vocab, [ix], df, stats, dev_u32(np.array([3, N_WORDS + 1], dtype=np.uint32)),
                                      [0, 2], 10), "index 1 ")
    d = ix.docs.copy()
    p = int(ix.post_off[0]) + 5
    d[p] = d[p - 1]
    refused(lambda: shards_search_raw(ctx, vocab, [Index(ix.post_off, d, ix.tf, ix.doc_len)], df, stats, t, q_off, 10),
            "posting %d:" % p)

    # mrg_search_merge: rows that are not in the order of the search, scores that are none
    k_in, nq, n_shards = 12, 2, 3
    rows_d, rows_b, cnt = host_rows(4, n_shards, nq, k_in, counts=[k_in, 5, k_in, 0, 9, k_in])
    merge_dev(ctx, n_shards, nq, k_in, dev_u32(rows_d.ravel()), dev_u32(rows_b.ravel()), cnt, 10)
    before = ctx.pool_stats()

    def merge_with(edit):
        dd, bb = rows_d.copy(), rows_b.copy()
        edit(dd, bb)
        t_d, t_b = dev_u32(dd.ravel()), dev_u32(bb.ravel())
        return lambda: merge_raw(ctx, n_shards, nq, k_in, t_d, t_b, cnt, 10)

    def swap(r, i):
        def edit(dd, bb):
            dd[r, [i, i + 1]], bb[r, [i, i + 1]] = dd[r, [i + 1, i]], bb[r, [i + 1, i]]
        return edit

    def put(r, i, doc=None, bits=None):
        def edit(dd, bb):
            if doc is not None:
                dd[r, i] = doc
            if bits is not None:
                bb[r, i] = bits
        return edit

    def both(*edits):
        def edit(dd, bb):
            for e in edits:
                e(dd, bb)
        return edit

    refused(merge_with(swap(2, 6)), "entry %d:" % (2 * k_in + 7))                     # the second of the pair stands wrong
    refused(merge_with(both(swap(5, 3), swap(0, 10))), "entry 11:")                    # two wrong: the smallest index
    refused(merge_with(put(4, 3, doc=rows_d[4, 2], bits=rows_b[4, 2])), "entry %d:" % (4 * k_in + 3))   # an equal pair
    refused(merge_with(put(1, 4, bits=0)), "entry %d:" % (k_in + 4))                  # a zero score, last of its row
    refused(merge_with(put(0, 0, bits=0x7FC00000)), "entry 0:")                        # a NaN
    refused(merge_with(put(2, 0, bits=0xBF800000)), "entry %d:" % (2 * k_in))          # a negative score
    ok = merge_with(both(put(1, 7, bits=0), swap(3, 2)))()   # beyond the counts nothing is read
    assert ok[2] == [10, 10]
    same_rows(merge_dev(ctx, n_shards, nq, k_in, dev_u32(rows_d.ravel()), dev_u32(rows_b.ravel()), cnt, 10),
              merge_twin(rows_d, rows_b, cnt, n_shards, nq, k_in, 10))
    assert ctx.pool_stats()[0] == before[0]
    del t


# ---- 6. the pipeline from text

def test_pipeline_from_text_in_shards(ctx):
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
        doc_len = np.diff(np.array(cut, dtype=np.int64)).astype(np.uint32)
        d_len = dev_u32(doc_len)
        texts = [b"Elizabeth Darcy", b"truth universally acknowledged", b"Pemberley love heart night", b"zzzunknownzzz white", b""]
        qt, qoff = to_device(texts)
        qtok = ctx.encode(v, qt.data_ptr(), qoff)
        d_q = torch.empty((max(qtok[-1], 1),), dtype=torch.int32, device="cuda:0")
        ctx.encode(v, qt.data_ptr(), qoff, d_q.data_ptr(), qtok[-1])
        nq, k = len(texts), 10

        def index(a, e):
            """rows [a, e) through term_counts -> postings(doc_base=a): (post_off, docs, tf, entries)"""
            row_off, _ = ctx.term_counts(v, d_ids.data_ptr(), cut[a:e + 1])
            E = row_off[-1]
            d_terms = torch.empty((max(E, 1),), dtype=torch.int32, device="cuda:0")
            d_counts = torch.empty_like(d_terms)
            ctx.term_counts(v, d_ids.data_ptr(), cut[a:e + 1], d_terms.data_ptr(), d_counts.data_ptr(), E)
            d_po = torch.empty((n_words + 1,), dtype=torch.int64, device="cuda:0")
            d_docs = torch.empty((max(E, 1),), dtype=torch.int32, device="cuda:0")
            d_tf = torch.empty_like(d_docs)
            assert ctx.postings(v, d_terms.data_ptr(), d_counts.data_ptr(), row_off, d_po.data_ptr(), d_docs.data_ptr(),
                                d_tf.data_ptr(), E, doc_base=a) == E
            return d_po, d_docs, d_tf, E

        # the one-piece path of test_pipeline_from_text
        po, dd, tf, E = index(0, n_docs)
        one_d, one_s = filled(nq * k), filled(nq * k)
        torch.cuda.synchronize()
        one_n = ctx.search(v, po.data_ptr(), dd.data_ptr(), tf.data_ptr(), E, d_len.data_ptr(), n_docs, d_q.data_ptr(), qtok, k,
                           one_d.data_ptr(), one_s.data_ptr())
        assert one_n[0] == k and one_n[4] == 0
        # three uneven row ranges, each indexed, counted and searched on its own
        ranges = [(0, 7), (7, n_docs // 2 + 3), (n_docs // 2 + 3, n_docs)]
        parts = [index(a, e) for a, e in ranges]
        assert sum(p[3] for p in parts) == E
        df = torch.zeros((n_words,), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        stats = (0, 0)
        for (a, e), p in zip(ranges, parts):
            stats = ctx.stats_add(v, p[0].data_ptr(), d_len.data_ptr() + 4 * a, e - a, df.data_ptr(), stats)
        assert stats == (n_docs, n_ids)
        in_d, in_s = filled(3 * nq * k), filled(3 * nq * k)
        torch.cuda.synchronize()
        in_n = []
        for i, ((a, e), p) in enumerate(zip(ranges, parts)):
            in_n += ctx.search_shard(v, p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3], d_len.data_ptr() + 4 * a, e - a,
                                     d_q.data_ptr(), qtok, k, in_d.data_ptr() + 4 * i * nq * k, in_s.data_ptr() + 4 * i * nq * k,
                                     df.data_ptr(), stats, doc_base=a)
        got = merge_dev(ctx, 3, nq, k, in_d, in_s, in_n, k)
        torch.cuda.synchronize()
        same_rows(got, (host_u32(one_d).reshape(nq, k), host_u32(one_s).reshape(nq, k), one_n))
    del t, qt


# ---- 7. a vocabulary of another device

def test_vocabulary_of_another_device(ctx, coll):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    ix = coll.whole
    with M.Context(1) as other:
        with make_vocab(other, N_WORDS) as v1:
            df = torch.zeros((N_WORDS,), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            with pytest.raises(M.MrgError) as ei:
                ctx.stats_add(v1, ix.d_post_off.data_ptr(), ix.d_doc_len.data_ptr(), ix.n_docs, df.data_ptr())
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
            torch.cuda.synchronize()
            assert (df.cpu().numpy() == 0).all()
            with pytest.raises(M.MrgError) as ei:
                shards_search_raw(ctx, v1, [ix], df, (ix.n_docs, 1), coll.d_ids, coll.q_off, 10)
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
