"""CPU tests of the Boolean search's host side: native.clause_roles, and the helpers of tests/bool_util.py -- the
numpy predicate and the masked scores the GPU tests expect -- against a brute force over plain Python sets and
dicts."""
import numpy as np
import pytest

from bool_util import MUST, MUST_NOT, SHOULD, filter_rows, lay_bool, masked_scores, predicate, scoring
from postings_util import expected_postings
from search_util import SENTINEL, UNK, expected_scores_dict


def test_clause_roles():
    from mapreduce_rust_amd import native
    assert (native.Q_SHOULD, native.Q_MUST, native.Q_MUST_NOT) == (SHOULD, MUST, MUST_NOT) == (0, 1, 2)
    M, S, N = native.Q_MUST, native.Q_SHOULD, native.Q_MUST_NOT
    # two queries: must "a b", should "c", must-not "d e f"; then must "", should "g h", must-not ""
    roles, q_off = native.clause_roles([0, 2, 3, 6, 6, 8, 8])
    assert roles == bytes([M, M, S, N, N, N, S, S]) and q_off == [0, 6, 8]
    # a first offset above 0: the roles are indexed like the ids, the entries in front belong to no query
    roles, q_off = native.clause_roles([4, 4, 4, 5, 7, 7, 9])
    assert len(roles) == 9 and roles[4:] == bytes([N, M, M, N, N]) and q_off == [4, 5, 9]
    # all clauses empty, and no query at all
    assert native.clause_roles([3, 3, 3, 3]) == (bytes(3), [3, 3])
    assert native.clause_roles([0]) == (b"", [0])
    assert native.clause_roles(np.array([0, 1, 2, 3], dtype=np.uint64)) == (bytes([M, S, N]), [0, 3])
    for bad in ([0, 1], [0, 1, 2], [0, 1, 2, 3, 4], []):
        with pytest.raises(ValueError):
            native.clause_roles(bad)
    with pytest.raises(ValueError):
        native.clause_roles([0, 2, 1, 3])


def test_clause_roles_lay_out_what_lay_bool_does():
    from mapreduce_rust_amd import native
    bq = [[(5, MUST), (6, MUST), (7, SHOULD), (8, MUST_NOT)], [], [(1, SHOULD)], [(2, MUST_NOT), (3, MUST_NOT)]]
    ids, roles, q_off = lay_bool(bq)                         # (every query here is already in clause order)
    tok_off = [0, 2, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 7]
    assert native.clause_roles(tok_off) == (roles, q_off)


def brute(post_off, docs, tf, doc_len, doc_base, bq, k1, b):
    """hits and scores by sets and dicts: {document index: score} per query"""
    post_off, docs = [int(x) for x in post_off], [int(x) for x in docs]
    held = lambda w: set() if w == UNK else {docs[at] - doc_base for at in range(post_off[w], post_off[w + 1])}
    rows = expected_scores_dict(post_off, docs, tf, doc_len, doc_base, scoring(bq), k1, b)
    out = []
    for q, row in zip(bq, rows):
        ok = set(range(len(doc_len)))
        for w, r in q:
            if r == MUST:
                ok &= held(int(w))
            elif r == MUST_NOT:
                ok -= held(int(w))
        out.append((ok, {i: s for i, s in row.items() if i in ok}))
    return out


def test_predicate_and_masked_scores_against_sets():
    from test_gpu_search import random_csr
    n_docs, n_words, base = 200, 40, 13
    rng = np.random.default_rng(3)
    terms, counts, row_off, doc_len = random_csr(rng, n_docs, n_words, 8)
    post_off, docs, tf = expected_postings(terms, counts, row_off, n_words, base)
    tf = tf.copy()
    tf[::7] = 0                                              # a posting counts whatever its tf
    none = n_words - 1
    assert post_off[none] == post_off[none + 1]
    bq = [[(0, MUST)], [(0, MUST), (1, MUST)], [(0, MUST), (2, SHOULD), (1, MUST_NOT)], [(1, MUST_NOT), (0, SHOULD)],
          [(3, MUST), (3, MUST), (4, SHOULD)], [(2, MUST), (2, MUST_NOT)], [(2, SHOULD), (2, MUST_NOT)],
          [(UNK, MUST), (0, SHOULD)], [(none, MUST), (0, SHOULD)], [(UNK, MUST_NOT), (0, SHOULD)],
          [(none, MUST_NOT), (0, SHOULD)], [(0, MUST_NOT), (1, MUST_NOT)], []]
    for _ in range(12):
        n = int(rng.integers(1, 9))
        bq.append([(int(rng.integers(0, 12)), int(rng.integers(0, 3))) for _ in range(n)])
    ok = predicate(post_off, docs, n_docs, base, bq)
    ref = masked_scores(post_off, docs, tf, doc_len, base, bq, 1.2, 0.75)
    want = brute(post_off, docs, tf, doc_len, base, bq, 1.2, 0.75)
    some = 0
    for qi, (ok_set, row) in enumerate(want):
        assert set(np.nonzero(ok[qi])[0].tolist()) == ok_set, qi
        assert set(np.nonzero(ref[qi] > 0)[0].tolist()) == {i for i, s in row.items() if s > 0}, qi
        for i, s in row.items():
            assert abs(ref[qi, i] - s) <= 1e-12 * max(s, 1.0), (qi, i)
        some += bool(row)
    hits = (ref > 0).sum(axis=1)
    assert some >= 10 and hits[5] == hits[7] == hits[8] == hits[11] == hits[12] == 0
    assert hits[9] == hits[10] > 0 and 0 < hits[1] < hits[0] and hits[6] == 0 < int(ok[6].sum()) and 0 < hits[3] < hits[9]
    # a document whose only posting of the MUST word has tf 0 passes the predicate
    zero_tf = {int(docs[at]) - base for at in range(int(post_off[0]), int(post_off[1])) if tf[at] == 0}
    assert zero_tf and all(ok[0, i] for i in zero_tf)


def test_filter_rows():
    docs = np.array([[17, 12, 15, 11, SENTINEL], [10, 11, 12, 13, 14]], dtype=np.uint32)
    bits = np.array([[90, 80, 80, 70, SENTINEL], [5, 4, 3, 2, 1]], dtype=np.uint32)
    ok = np.zeros((2, 8), dtype=bool)
    ok[0, [1, 5, 7]] = True                                  # documents 11, 15, 17
    d, s, n = filter_rows(docs, bits, [4, 5], ok, 2, 10)
    assert n == [2, 0] and d[0].tolist() == [17, 15] and s[0].tolist() == [90, 80] and (d[1] == SENTINEL).all()
    d, s, n = filter_rows(docs, bits, [4, 5], ok, 4, 10)
    assert n == [3, 0] and d[0].tolist() == [17, 15, 11, SENTINEL] and s[0].tolist() == [90, 80, 70, SENTINEL]
