"""CPU tests of mrg_vocab_search at the ABI boundary: the symbol and mrg_search_info are exported and bound, the
header and the Rust declarations carry it with 18 parameters, the constants mirror the device header, a NULL
context comes back as MRG_EINVAL with a message (never a crash); and of the helpers the GPU tests rest on:
expected_scores equals a plain Python evaluation, and check_topk accepts the top-k of a float32 evaluation and
rejects a swapped pair, a missing better document, a wrong tie order and a score that is off.  No GPU is needed:
every call here fails before it reaches the device."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from postings_util import expected_postings
from search_util import RTOL, UNK, check_topk, expected_scores, expected_scores_dict, scores_f32, topk_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    from mapreduce_rust_amd import native
    return native.load()


@pytest.fixture(autouse=True, scope="module")
def the_call_exists():
    """the helpers below are the yardstick of a call: without it they have nothing to measure"""
    import mapreduce_rust_amd as M
    assert hasattr(C.CDLL(M.lib_path()), "mrg_vocab_search")


def test_header_and_rust_declare_it():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_search" in hdr
    assert "#define MRG_ABI_VERSION 6" in hdr and "#define MRG_SEARCH_MAX_K 1024u" in hdr
    c = re.search(r"^int mrg_vocab_search\(([^)]*)\);", hdr, re.M)
    r = re.search(r"pub fn mrg_vocab_search\(([^)]*)\) -> c_int;", rs, re.S)
    assert c and r
    assert c.group(1).count(",") + 1 == 18 == r.group(1).count(",") + 1
    assert "pub const MRG_SEARCH_MAX_K: u32 = 1024;" in rs
    assert "mrg_search_info" not in hdr                      # a diagnostic, like mrg_postings_info


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    assert hasattr(raw, "mrg_vocab_search") and hasattr(raw, "mrg_search_info")
    assert "mrg_vocab_search" in native.exported_symbols()
    assert lib().mrg_vocab_search.restype is C.c_int and len(lib().mrg_vocab_search.argtypes) == 18
    for m in ("search", "search_info"):
        assert callable(getattr(M.Context, m))
    assert b"abi 6" in lib().mrg_version()


def test_constants_mirror_the_device_header():
    from mapreduce_rust_amd import native
    dev = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "mrg_device.h")).read()
    for name in ("SEARCH_TILE", "SEARCH_MAX_K"):
        m = re.search(r"^#define MRG_%s (\d+)u$" % name, dev, re.M)
        assert m and int(m.group(1)) == getattr(native, name), name
    assert native.SEARCH_TILE % 1024 == 0                    # whole rounds of 256 threads x 16 bytes
    assert native.SEARCH_MAX_K * 8 <= 64 * 1024              # a query's candidates fit one workgroup's LDS


def test_null_context():
    from mapreduce_rust_amd import native
    L = lib()
    off = (C.c_uint64 * 2)(0, 3)
    top = (C.c_uint32 * 1)(77)
    args = [None, None, None, None, None, 0, None, 0, 0, None, off, 1, 1.2, 0.75, 10, None, None, top]
    assert L.mrg_vocab_search(*args) == native.EINVAL
    assert "context" in L.mrg_last_error().decode()
    assert top[0] == 77 and list(off) == [0, 3]
    args[10] = args[17] = None
    assert L.mrg_vocab_search(*args) == native.EINVAL and L.mrg_last_error().decode()
    f = L.mrg_search_info
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    assert f(None, None, None) == native.EINVAL and "context" in L.mrg_last_error().decode()


def random_case(rng, big_values=False):
    """a small random collection, its index by expected_postings, and a few queries"""
    n_words = rng.choice((1, 2, 5, 30))
    n_docs = rng.randrange(0, 9)
    doc_base = rng.choice((0, 0, 5, 2**32 - n_docs))
    hi = 2**32 - 1 if big_values else 40
    row_off, terms = [0], []
    for _ in range(n_docs):
        row = sorted(rng.sample(range(n_words), rng.randrange(0, min(n_words, 6) + 1)))
        terms.extend(row)
        row_off.append(len(terms))
    counts = [rng.choice((0, 1, 1, 2, rng.randrange(1, hi + 1))) for _ in terms]
    doc_len = [rng.choice((0, 1, rng.randrange(1, hi + 1))) for _ in range(n_docs)]
    post_off, docs, tf = expected_postings(np.array(terms, dtype=np.uint32), np.array(counts, dtype=np.uint32), row_off,
                                           n_words, doc_base)
    queries = [[rng.choice((UNK, rng.randrange(n_words), rng.randrange(n_words))) for _ in range(rng.choice((0, 1, 2, 7)))]
               for _ in range(rng.randrange(0, 4))]
    return post_off, docs, tf, doc_len, doc_base, queries


def test_numpy_helper_equals_dict():
    rng = random.Random(20261020)
    seen = {"unk": 0, "repeat": 0, "hit": 0, "tf0": 0, "base": 0, "nodocs": 0}
    for case in range(200):
        post_off, docs, tf, doc_len, doc_base, queries = random_case(rng, big_values=case % 2 == 1)
        k1, b = rng.choice((0.0, 0.5, 1.2, 1000.0)), rng.choice((0.0, 0.3, 0.75, 1.0))
        got = expected_scores(post_off, docs, tf, doc_len, doc_base, queries, k1, b)
        want = expected_scores_dict(post_off, docs, tf, doc_len, doc_base, queries, k1, b)
        assert got.shape == (len(queries), len(doc_len)) and got.dtype == np.float64
        for q, row in enumerate(want):
            dense = np.zeros(len(doc_len))
            for i, s in row.items():
                dense[i] = s
            assert np.allclose(got[q], dense, rtol=1e-13, atol=0), (case, q)
            assert ((got[q] > 0) == (dense > 0)).all()
            seen["hit"] += bool(row)
        seen["unk"] += any(UNK in q for q in queries)
        seen["repeat"] += any(len(set(q)) < len(q) for q in queries)
        seen["tf0"] += bool((np.asarray(tf) == 0).any())
        seen["base"] += doc_base > 0
        seen["nodocs"] += not doc_len
    assert all(v > 10 for v in seen.values()), seen


def float32_case():
    """3 queries over 400 documents whose float32 top-k the checks below start from"""
    rng = np.random.default_rng(5)
    n_docs, n_words = 400, 50
    rows = [np.sort(rng.choice(n_words, rng.integers(1, 12), replace=False)) for _ in range(n_docs)]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    terms = np.concatenate(rows).astype(np.uint32)
    counts = rng.integers(1, 9, len(terms)).astype(np.uint32)
    doc_len = rng.integers(5, 300, n_docs).astype(np.uint32)
    post_off, docs, tf = expected_postings(terms, counts, row_off, n_words)
    queries = [[3, 7, 7, UNK, 11], [0], list(rng.integers(0, n_words, 64))]
    args = (post_off, docs, tf, doc_len, 0, queries, 1.2, 0.75)
    return expected_scores(*args), scores_f32(*args)


def test_check_topk_accepts_float32_and_rejects_errors():
    ref, s32 = float32_case()
    rel = np.abs(s32 - ref)[ref > 0] / ref[ref > 0]
    assert rel.max() < RTOL / 2                              # the bound RTOL was derived from holds here
    for k in (1, 10, 1024):
        docs, sc, top_n = topk_f32(s32, k)
        check_topk(docs, sc, top_n, ref, k, 0)
    k = 10
    docs, sc, top_n = topk_f32(s32, k)
    assert top_n == [k, k, k]

    def rejected(d, s, n, what):
        with pytest.raises(AssertionError, match=what):
            check_topk(d, s, n, ref, k, 0)

    d, s = docs.copy(), sc.copy()                            # a swapped pair (documents with their scores)
    assert s[0, 2] > s[0, 3] * (1 + 4 * RTOL)
    d[0, [2, 3]], s[0, [2, 3]] = d[0, [3, 2]], s[0, [3, 2]]
    rejected(d, s, top_n, "scores increase")
    d, s = docs.copy(), sc.copy()                            # the documents swapped, the scores left in order
    d[0, [2, 3]] = d[0, [3, 2]]
    rejected(d, s, top_n, "score")
    d, s = docs.copy(), sc.copy()                            # the best document missing: the 11th in its place
    full_d, full_s, _ = topk_f32(s32, k + 1)
    d[2, :], s[2, :] = full_d[2, 1:], full_s[2, 1:]
    rejected(d, s, top_n, "better document")
    d, s = docs.copy(), sc.copy()                            # a score off by 1e-4 relative
    s[1, 4] = np.float32(s[1, 4] * (1 - 1e-4))
    rejected(d, s, top_n, "score")
    d, s = docs.copy(), sc.copy()                            # a document twice
    d[1, 5], s[1, 5] = d[1, 4], s[1, 4]
    rejected(d, s, top_n, "twice")
    rejected(docs, sc, [k, k - 1, k], "top_n")               # a short row


def test_check_topk_rejects_a_wrong_tie_order():
    ref = np.zeros((1, 8))
    ref[0, [1, 2, 5, 6]] = [2.0, 1.0, 1.0, 1.0]
    sc = np.array([[2.0, 1.0, 1.0]], dtype=np.float32)
    check_topk(np.array([[1, 2, 5]], dtype=np.uint32), sc, [3], ref, 3, 0)
    check_topk(np.array([[101, 102, 105]], dtype=np.uint32), sc, [3], ref, 3, 100)
    with pytest.raises(AssertionError, match="document order"):
        check_topk(np.array([[1, 5, 2]], dtype=np.uint32), sc, [3], ref, 3, 0)
    # ties at the k-th place: check_topk's tolerance cannot tell 2, 5 from 2, 6 (the exact-tie test of the GPU
    # suite compares the documents themselves); a non-hit is never accepted
    with pytest.raises(AssertionError, match="no hit"):
        check_topk(np.array([[1, 2, 3]], dtype=np.uint32), sc, [3], ref, 3, 0)
    with pytest.raises(AssertionError, match="out of range"):
        check_topk(np.array([[1, 2, 8]], dtype=np.uint32), sc, [3], ref, 3, 0)
