"""GPU tests of mrg_vocab_search_bool and mrg_vocab_search_bool_shard (k_search.hip): BM25
top-k with MUST and MUST_NOT positions.

No expectation comes from the code under test.  The predicate comes from the host copies of the postings
(tests/bool_util.py predicate), the scores from search_util.expected_scores over the query without its MUST_NOT
positions, zeroed where the predicate fails, compared by check_topk with its derived RTOL (at most 64 positions
per query).  The byte-exact checks filter the ranking of the plain mrg_vocab_search, which tests/test_gpu_search.py
holds to the float64 reference.  Every call goes twice into sentinel-filled rows with slack (bool_util.bool_dev)."""
import numpy as np
import pytest

from bool_util import (MUST, MUST_NOT, SHOULD, bool_dev, bool_raw, filter_rows, lay_bool, masked_ref, predicate, scoring)
from postings_util import expected_postings
from search_util import MAX_POSITIONS, SENTINEL, UNK, Index, check_topk, dev_u32, lay_queries, search_dev
from shard_util import merge_dev, split_index, stats_dev
from terms_util import make_vocab
from test_gpu_search import N_WORDS, consts, mixed_queries, random_csr, random_index, tile_index

pytestmark = pytest.mark.gpu

NONE = N_WORDS - 1                                           # the word without postings of random_csr
M, S, N = MUST, SHOULD, MUST_NOT


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M_
    c = M_.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vocab(ctx):
    v = make_vocab(ctx, N_WORDS)
    yield v
    v.close()


@pytest.fixture(scope="module")
def coll():
    return random_index(1, 5000)


def members(ix, w):
    return set((ix.docs[int(ix.post_off[w]):int(ix.post_off[w + 1])].astype(np.int64) - ix.doc_base).tolist())


def case_queries(ix):
    """the Boolean queries of case 1, over the hot words 0 .. 3 of a random_index; queries 16, 17, 18 differ only in
    where their MUST_NOT position stands"""
    df = np.diff(ix.post_off.astype(np.int64))
    assert df[NONE] == 0 and (df[:8] > 0).all()
    assert members(ix, 0) & members(ix, 1) & members(ix, 2) & members(ix, 3), "the hot words share no document"
    assert members(ix, 0) - members(ix, 1) and members(ix, 0) - members(ix, 2)
    rng = np.random.default_rng(21)
    mix = [(int(w), S) for w in rng.integers(4, N_WORDS - 1, MAX_POSITIONS)]
    mix[0], mix[33], mix[63] = (0, M), (1, M), (0, M)
    for at in (2, 9, 17, 40, 62):
        mix[at] = (int(rng.integers(4, 40)), N)
    mix[5], mix[50] = (UNK, S), (NONE, N)
    assert len(mix) == MAX_POSITIONS
    return [
        [(0, M)], [(0, M), (1, M)], [(0, M), (1, M), (2, M), (3, M)],        # 0 .. 2: MUST only
        [(0, M), (5, S), (6, S)],                                            # 3: MUST + SHOULD
        [(0, S), (1, S), (2, N)],                                            # 4: SHOULD + MUST_NOT
        [(0, M), (4, S), (1, N)],                                            # 5: all three
        [(1, M), (2, S), (1, M)],                                            # 6: a MUST word twice
        [(0, M), (0, N)],                                                    # 7: MUST and MUST_NOT: nothing
        [(0, S), (1, S), (0, N)],                                            # 8: SHOULD and MUST_NOT
        [(UNK, M), (0, S)], [(NONE, M), (0, S)],                             # 9, 10: an unsatisfiable MUST
        [(UNK, N), (0, S)], [(NONE, N), (0, S)],                             # 11, 12: excludes nothing
        [(0, N), (1, N)],                                                    # 13: MUST_NOT only
        [],                                                                  # 14
        mix,                                                                 # 15
        [(2, N), (0, S), (1, M)], [(0, S), (2, N), (1, M)], [(0, S), (1, M), (2, N)],   # 16 .. 18
    ]


def expected_rows(ctx, vocab, ix, bq, k, plain=None):
    """the plain search's complete ranking of the scoring positions, filtered on the host and cut at k"""
    K = consts()[1]
    d, s, n = plain or search_dev(ctx, vocab, ix, scoring(bq), K)
    assert all(x < K for x in n), "a plain ranking may be cut: it must hold every hit"
    ok = predicate(ix.post_off, ix.docs, ix.n_docs, ix.doc_base, bq)
    return filter_rows(d, s.view(np.uint32), n, ok, k, ix.doc_base), n


# ---- 1. exact against the plain search

def test_exact_against_the_plain_search(ctx, vocab):
    ix = random_index(11, 900)
    bq = case_queries(ix)
    K = consts()[1]
    plain = search_dev(ctx, vocab, ix, scoring(bq), K)
    ref = masked_ref(ix, bq)
    for k in (1, 3, 10, K):
        (want_d, want_b, want_n), plain_n = expected_rows(ctx, vocab, ix, bq, k, plain)
        d, b, n = bool_dev(ctx, vocab, ix, bq, k, first=2 if k == 3 else 0)
        assert n == want_n, k
        assert d.tobytes() == want_d.tobytes() and b.tobytes() == want_b.tobytes(), k
        check_topk(d, b.view(np.float32), n, ref, k, ix.doc_base)
        if k == K:                                           # the set of cases is not vacuous
            assert sum(x > 0 for x in n) >= 5
            assert sum(0 < x < p for x, p in zip(n, plain_n)) >= 5
            assert sum(x == 0 for x in n) >= 4 and [n[q] for q in (7, 9, 10, 13, 14)] == [0] * 5
            assert n[8] > 0 and n[11] == n[12] == plain_n[11] and 0 < n[6] == len(members(ix, 1))
        assert d[16].tobytes() == d[17].tobytes() == d[18].tobytes()
        assert b[16].tobytes() == b[17].tobytes() == b[18].tobytes() and n[16] == n[17] == n[18] > 0
    info = ctx.search_info()
    assert info["queries"] == len(bq) and info["positions"] == sum(len(q) for q in bq) and info["chunks"] == 1
    assert info["scratch_bytes"] > 8 * ix.n_docs * len(bq)   # the rows and the match states
    df = np.diff(ix.post_off.astype(np.int64))               # a query with an unsatisfiable MUST visits nothing
    assert info["postings"] == sum(int(df[w]) for i, q in enumerate(bq) if i not in (9, 10) for w, _ in q if w != UNK)
    # every query of a call unsatisfiable: no tile at all
    dead = [bq[9], bq[10], [(NONE, M), (1, S), (2, N)]]
    d, b, n = bool_dev(ctx, vocab, ix, dead, 10)
    assert n == [0, 0, 0] and ctx.search_info()["postings"] == 0 and ctx.search_info()["acc_launches"] == 0


# ---- 2. all SHOULD, and no roles: the plain search

def test_all_should_is_the_plain_search(ctx, vocab, coll):
    queries = mixed_queries(coll, np.random.default_rng(2))
    bq = [[(w, S) for w in q] for q in queries]
    n_ids = sum(len(q) for q in queries)
    for k, first in ((10, 0), (1024, 5)):
        d0, s0, n0 = search_dev(ctx, vocab, coll, queries, k, first=first)
        plain_info = ctx.search_info()
        for roles in ("given", None, bytes(first + n_ids)):
            d, b, n = bool_dev(ctx, vocab, coll, bq, k, first=first, roles=roles)
            assert n == n0 and d.tobytes() == d0.tobytes() and b.tobytes() == s0.tobytes(), (k, first, roles)
            info = ctx.search_info()
            assert info["scratch_bytes"] == plain_info["scratch_bytes"] and info["acc_launches"] == plain_info["acc_launches"]


# ---- 3. more hits than MAX_K: the k-th place among the hits

def test_the_kth_place_beyond_max_k(ctx, vocab, coll):
    K = consts()[1]
    both = members(coll, 0) & members(coll, 1)
    four = both & members(coll, 2) & members(coll, 3)
    assert len(both) > K and 0 < len(four) < K
    two, all4 = [(0, M), (1, M)], [(w, M) for w in range(4)]
    for bq, k in (([two, all4], K), ([two], 10)):
        d, b, n = bool_dev(ctx, vocab, coll, bq, k)
        check_topk(d, b.view(np.float32), n, masked_ref(coll, bq), k, coll.doc_base)
        assert n[0] == k and (len(bq) == 1 or n[1] == len(four))


# ---- 4. tile edges

@pytest.mark.parametrize("pad_docs,pad_tf", [(0, 0), (1, 1), (2, 3), (3, 0)])
def test_tile_edges(ctx, pad_docs, pad_tf):
    T = consts()[0]
    n_docs = 5 * T // 2 + 3
    ix, marks, n_words = tile_index(n_docs, pad_docs, pad_tf, doc_base=11)
    every = marks["all"]
    words = [w for key, w in marks.items() if key != "all"]
    assert len(words) == 16
    bq = [[(w, M), (every, S)] for w in words] + [[(w, N), (every, S)] for w in words]
    ref = masked_ref(ix, bq)
    with make_vocab(ctx, n_words) as v:
        for k in (10, 1024):
            d, b, n = bool_dev(ctx, v, ix, bq, k)
            check_topk(d, b.view(np.float32), n, ref, k, ix.doc_base)
    hits = (ref > 0).sum(axis=1)
    for i, w in enumerate(words):
        df = int(ix.post_off[w + 1] - ix.post_off[w])
        assert hits[i] == df and hits[16 + i] == n_docs - df


# ---- 5. row ends

@pytest.mark.parametrize("n_docs", [1, 3, 1023, 1024, 1025, 4097])
def test_row_ends(ctx, vocab, n_docs):
    """word 10 (MUST) and word 11 (MUST_NOT) both hold the last document; word 12 stands in every document.  The
    cells of the stride beyond n_docs never become hits: check_topk sees every returned document and the counts."""
    rng = np.random.default_rng(n_docs)
    base, last = 7, n_docs - 1
    pick = lambda frac: np.union1d(np.nonzero(rng.random(n_docs) < frac)[0], [last])
    lists = {10: pick(0.5), 11: pick(0.3), 12: np.arange(n_docs)}
    post_off = np.zeros(N_WORDS + 1, dtype=np.uint64)
    for w, l in lists.items():
        post_off[w + 1:] += len(l)
    docs = np.concatenate([lists[w] for w in (10, 11, 12)]).astype(np.uint32) + base
    tf = rng.integers(1, 6, len(docs)).astype(np.uint32)
    ix = Index(post_off, docs, tf, rng.integers(1, 300, n_docs).astype(np.uint32), base)
    bq = [[(10, M), (12, S)], [(11, N), (12, S)], [(10, M), (11, N), (12, S)], [(10, M)], [(12, S), (10, N), (11, N)]]
    ref = masked_ref(ix, bq)
    assert ref[0, last] > 0 and ref[3, last] > 0 and ref[1, last] == 0 and ref[2, last] == 0
    for k in (1, 10, 1024):
        d, b, n = bool_dev(ctx, vocab, ix, bq, k)
        check_topk(d, b.view(np.float32), n, ref, k, base)
    got = set(d[0, :n[0]].tolist())                          # (k = 1024: with n_docs <= 1024 every hit is returned)
    if len(lists[10]) <= 1024:
        assert got == set((lists[10] + base).tolist())
    assert n[1] == min(1024, n_docs - len(lists[11]))


# ---- 6. a posting with tf = 0 counts as a posting

def test_tf_zero_is_a_posting(ctx, vocab):
    n_docs = 8
    lists = {1: ([0, 1, 2], [2, 0, 1]), 2: ([0, 1, 3, 5], [1, 2, 3, 1]), 3: ([3, 6], [0, 1])}
    post_off = np.zeros(N_WORDS + 1, dtype=np.uint64)
    for w, (l, _) in lists.items():
        post_off[w + 1:] += len(l)
    docs = np.concatenate([lists[w][0] for w in (1, 2, 3)]).astype(np.uint32)
    tf = np.concatenate([lists[w][1] for w in (1, 2, 3)]).astype(np.uint32)
    ix = Index(post_off, docs, tf, np.full(n_docs, 9, dtype=np.uint32))
    # document 1: its only posting of the MUST word has tf 0, a SHOULD word scores it: a hit.  Document 3: its
    # posting of the MUST_NOT word has tf 0: excluded.
    bq = [[(1, M), (2, S)], [(2, S), (3, N)], [(1, M)]]
    ref = masked_ref(ix, bq)
    assert set(np.nonzero(ref[0])[0]) == {0, 1, 2} and set(np.nonzero(ref[1])[0]) == {0, 1, 5}
    assert set(np.nonzero(ref[2])[0]) == {0, 2}              # document 1 passes the filter with a score of 0: no hit
    d, b, n = bool_dev(ctx, vocab, ix, bq, 10)
    check_topk(d, b.view(np.float32), n, ref, 10, 0)
    assert n == [3, 3, 2] and 1 in d[0, :3].tolist() and 3 not in d[1, :3].tolist()
    plain = search_dev(ctx, vocab, ix, [[2]], 10)
    assert 3 in plain[0][0, :plain[2][0]].tolist()


# ---- 7. chunks

def test_chunks_give_identical_bytes(ctx, vocab, monkeypatch):
    ix = random_index(11, 900)
    bq = case_queries(ix)
    cell_bytes = 8 * ix.n_docs                               # a row and its match states
    monkeypatch.delenv("MRG_SEARCH_ACC_BYTES", raising=False)
    d0, b0, n0 = bool_dev(ctx, vocab, ix, bq, 10)
    assert ctx.search_info()["chunks"] == 1
    for acc, chunks in ((7 * cell_bytes + 100, 3), (2 * cell_bytes - 1, len(bq)), (1, len(bq))):
        monkeypatch.setenv("MRG_SEARCH_ACC_BYTES", str(acc))
        d, b, n = bool_dev(ctx, vocab, ix, bq, 10)
        assert ctx.search_info()["chunks"] == chunks, (acc, ctx.search_info())
        assert n == n0 and d.tobytes() == d0.tobytes() and b.tobytes() == b0.tobytes(), acc
    # all SHOULD: the rows of a chunk are counted at 4 bytes per document, as in the plain call
    monkeypatch.setenv("MRG_SEARCH_ACC_BYTES", str(7 * cell_bytes + 100))
    bool_dev(ctx, vocab, ix, [[(w, S) for w, _ in q] for q in bq], 10)
    assert ctx.search_info()["chunks"] == 2
    monkeypatch.delenv("MRG_SEARCH_ACC_BYTES")


# ---- 8. shards

def test_shards_equal_the_whole(ctx, vocab):
    n_docs, cuts = 900, [0, 200, 650, 900]
    terms, counts, row_off, doc_len = random_csr(np.random.default_rng(11), n_docs, N_WORDS, 12)
    rows = np.repeat(np.arange(n_docs), np.diff(row_off))
    keep = ~((terms == 3) & (rows >= cuts[1]) & (rows < cuts[2]))   # word 3 has no postings in the middle shard
    terms, counts, rows = terms[keep], counts[keep], rows[keep]
    row_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_docs))]).astype(np.int64).tolist()
    csr = (terms, counts, row_off, doc_len)
    whole = Index(*expected_postings(terms, counts, row_off, N_WORDS, 0), doc_len)
    shards = split_index(csr, cuts, N_WORDS)
    df3 = [int(s.post_off[4] - s.post_off[3]) for s in shards]
    assert df3[1] == 0 and df3[0] > 0 and df3[2] > 0
    bq = case_queries(whole)
    assert any(w == 3 and r == M for w, r in bq[2])
    ids, roles, q_off = lay_bool(bq)
    nq = len(bq)
    df, stats = stats_dev(ctx, vocab, shards)
    for k in (10, 1024):
        want_d, want_b, want_n = bool_dev(ctx, vocab, whole, bq, k)
        in_d, in_b, in_n = [], [], []
        for s in shards:
            d, b, n = bool_dev(ctx, vocab, s, bq, k, shard=(df.data_ptr(), stats))
            in_d.append(d), in_b.append(b), in_n.extend(n)
        assert in_n[nq + 2] == 0                             # MUST(3) in the shard that lacks it
        got_d, got_b, got_n = merge_dev(ctx, len(shards), nq, k, dev_u32(np.concatenate(in_d).ravel()),
                                        dev_u32(np.concatenate(in_b).ravel()), in_n, k)
        assert got_n == want_n and want_n[2] > 0, k
        for q in range(nq):                                  # (a shard row keeps its sentinels; the merge writes none)
            assert got_d[q, :got_n[q]].tobytes() == want_d[q, :want_n[q]].tobytes(), (k, q)
            assert got_b[q, :got_n[q]].tobytes() == want_b[q, :want_n[q]].tobytes(), (k, q)
            assert (got_d[q, got_n[q]:] == SENTINEL).all() and (got_b[q, got_n[q]:] == SENTINEL).all()
    check_topk(want_d, want_b.view(np.float32), want_n, masked_ref(whole, bq), 1024, 0)


# ---- 9. refusals

def test_refusals(ctx, vocab):
    import mapreduce_rust_amd as M_
    EINVAL = M_.native.EINVAL
    ix = random_index(11, 900)
    bq = [[(0, M), (5, S)], [(1, S), (2, N)], [(3, M), (1, N)]]
    good = bool_dev(ctx, vocab, ix, bq, 10)                  # (the pool has seen these sizes)
    before = ctx.pool_stats()

    def refused(ixb, ids, roles, q_off, what):
        t = dev_u32(ids)
        with pytest.raises(M_.MrgError) as ei:
            bool_raw(ctx, vocab, ixb, t, roles, q_off, 10)
        assert ei.value.code == EINVAL and what in str(ei.value), (what, str(ei.value))
        assert ctx.pool_stats()[0] == before[0], "scratch not returned after an error"
        del t

    # a role above 2: the smallest index, counted like the ids; nothing is written
    ids, roles, q_off = lay_bool(bq, first=3)
    bad = bytearray(roles)
    bad[5], bad[8] = 3, 200
    refused(ix, ids, bytes(bad), q_off, "role at index 5")
    assert all((a == SENTINEL).all() for a in bool_raw.last), "an output was written by a refused call"
    bad = bytearray(roles)
    bad[3] = 3
    refused(ix, ids, bytes(bad), q_off, "role at index 3")
    assert all((a == SENTINEL).all() for a in bool_raw.last)
    # documents that descend inside the list of a MUST_NOT word: its postings are checked like the others
    lo, hi = int(ix.post_off[2]), int(ix.post_off[3])
    assert hi - lo > 20
    p = lo + 9
    d = ix.docs.copy()
    d[p] = d[p - 2]
    refused(Index(ix.post_off, d, ix.tf, ix.doc_len), *lay_bool(bq), "posting %d:" % p)
    # and inside the list of a MUST word
    lo3 = int(ix.post_off[3])
    d = ix.docs.copy()
    d[lo3 + 1] = d[lo3]
    refused(Index(ix.post_off, d, ix.tf, ix.doc_len), *lay_bool(bq), "posting %d:" % (lo3 + 1))
    # then a good call on the same context succeeds, and nothing is outstanding
    again = bool_dev(ctx, vocab, ix, bq, 10)
    assert again[2] == good[2] and again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()
    assert ctx.pool_stats()[0] <= before[0]
    check_topk(again[0], again[1].view(np.float32), again[2], masked_ref(ix, bq), 10, 0)
