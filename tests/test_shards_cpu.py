"""CPU tests of the sharded search (mrg_vocab_stats_add, mrg_vocab_search_shard, mrg_search_merge) at the ABI
boundary -- the three symbols are exported, bound and declared with matching arity, a NULL context comes back as
MRG_EINVAL with a message -- and of the helpers the GPU tests rest on (tests/shard_util.py): the scores of the
shards with the collection's statistics, concatenated, are exactly the scores of the index in one piece, scores
from shard-local statistics are not, and merge_twin agrees with sorted() of tuples.  No GPU is needed: every
call here fails before it reaches the device."""
import ctypes as C
import os
import random
import re

import numpy as np

from postings_util import expected_postings
from search_util import SENTINEL, UNK, expected_scores
from shard_util import coll_stats, expected_scores_coll, merge_twin, split_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"mrg_vocab_stats_add": 7, "mrg_vocab_search_shard": 21, "mrg_search_merge": 11}
N_WORDS = 120
CUTS = [0, 1, 64, 65, 300]


def lib():
    from mapreduce_rust_amd import native
    return native.load()


# ---- the ABI

def test_header_and_rust_declare_them():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_stats_add, mrg_vocab_search_shard, mrg_search_merge" in hdr
    assert "#define MRG_ABI_VERSION 6" in hdr and "#define MRG_SEARCH_MAX_SHARDS 64u" in hdr
    assert "pub const MRG_SEARCH_MAX_SHARDS: u32 = 64;" in rs
    for name, arity in CALLS.items():
        c = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        r = re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % name, rs, re.S)
        assert c and r, name
        assert c.group(1).count(",") + 1 == arity == r.group(1).count(",") + 1, name


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    for name, arity in CALLS.items():
        assert hasattr(raw, name), name
        assert name in native.exported_symbols()
        f = getattr(lib(), name)
        assert f.restype is C.c_int and len(f.argtypes) == arity, name
    for m in ("stats_add", "search_shard", "search_merge"):
        assert callable(getattr(M.Context, m))
    assert b"abi 6" in lib().mrg_version()


def test_constants_mirror_the_device_header():
    from mapreduce_rust_amd import native
    dev = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "mrg_device.h")).read()
    for name, attr in (("SEARCH_MAX_SHARDS", "SEARCH_MAX_SHARDS"), ("MERGE_LDS_KEYS", "MERGE_LDS_KEYS")):
        m = re.search(r"^#define MRG_%s (\d+)u$" % name, dev, re.M)
        assert m and int(m.group(1)) == getattr(native, attr), name
    assert native.MERGE_LDS_KEYS * 8 <= 64 * 1024            # the staged keys of a query
    assert native.SEARCH_MAX_K <= native.MERGE_LDS_KEYS < native.SEARCH_MAX_SHARDS * native.SEARCH_MAX_K   # both paths exist


def test_null_context():
    from mapreduce_rust_amd import native
    L = lib()
    coll = (C.c_uint64 * 2)(5, 6)
    assert L.mrg_vocab_stats_add(None, None, None, None, 0, None, coll) == native.EINVAL
    assert "context" in L.mrg_last_error().decode() and list(coll) == [5, 6]
    off = (C.c_uint64 * 2)(0, 3)
    top = (C.c_uint32 * 1)(77)
    args = [None, None, None, None, None, 0, None, 0, 0, None, 0, 0, None, off, 1, 1.2, 0.75, 10, None, None, top]
    assert L.mrg_vocab_search_shard(*args) == native.EINVAL
    assert "context" in L.mrg_last_error().decode() and top[0] == 77
    args[13] = args[20] = None
    assert L.mrg_vocab_search_shard(*args) == native.EINVAL and L.mrg_last_error().decode()
    cnt = (C.c_uint32 * 2)(1, 1)
    assert L.mrg_search_merge(None, 2, 1, 10, None, None, cnt, 10, None, None, top) == native.EINVAL
    assert "context" in L.mrg_last_error().decode() and top[0] == 77
    assert L.mrg_search_merge(None, 0, 0, 0, None, None, None, 0, None, None, None) == native.EINVAL and L.mrg_last_error().decode()


# ---- the helpers

def random_csr(seed, n_docs=300, n_words=N_WORDS):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n_words - 1, rng.integers(0, 14), replace=False)) for _ in range(n_docs)]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    terms = np.concatenate(rows).astype(np.uint32)
    counts = rng.integers(0, 9, len(terms)).astype(np.uint32)   # 0 included: copied as it is
    doc_len = rng.integers(0, 300, n_docs).astype(np.uint32)
    return terms, counts, row_off, doc_len


def queries_for(rng):
    qs = [[int(x) for x in rng.integers(0, N_WORDS, n)] for n in (0, 1, 2, 7, 64)]
    qs[3][2], qs[4][5], qs[4][6] = UNK, qs[4][7], N_WORDS - 1   # an UNK, a repeat, the word without postings
    return qs


def test_shards_with_collection_statistics_equal_the_whole():
    for seed, base in ((1, 0), (2, 7)):
        csr = random_csr(seed)
        terms, counts, row_off, doc_len = csr
        queries = queries_for(np.random.default_rng(seed))
        whole = expected_postings(terms, counts, row_off, N_WORDS, base)
        shards = split_host(csr, CUTS, N_WORDS, base)
        df, n, total = coll_stats(shards)
        assert n == 300 and total == int(doc_len.astype(np.int64).sum())
        assert (df == np.diff(whole[0].astype(np.int64))).all()
        assert sum(len(s[1]) for s in shards) == len(whole[1])  # a document's postings all stand in its own shard
        for k1, b in ((1.2, 0.75), (0.0, 0.0), (1000.0, 1.0)):
            want = expected_scores(*whole, doc_len, base, queries, k1, b)
            parts = [expected_scores_coll(po, d, f, dl, sb, queries, k1, b, n, total, df) for po, d, f, dl, sb in shards]
            got = np.concatenate(parts, axis=1)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (seed, k1, b)
            assert (want > 0).sum() > 300
            # shard-local statistics give other scores: the GPU tests are sensitive to the statistics
            local = np.concatenate([expected_scores(po, d, f, dl, sb, queries, k1, b) for po, d, f, dl, sb in shards], axis=1)
            hit = want > 0
            assert ((local > 0) == hit).all() and (local[hit] != want[hit]).mean() > 0.9, (seed, k1, b)


def test_one_shard_with_its_own_statistics_is_the_plain_helper():
    csr = random_csr(3)
    terms, counts, row_off, doc_len = csr
    po, d, f = expected_postings(terms, counts, row_off, N_WORDS, 5)
    queries = queries_for(np.random.default_rng(3))
    df = np.diff(po.astype(np.int64))
    got = expected_scores_coll(po, d, f, doc_len, 5, queries, 1.2, 0.75, 300, int(doc_len.astype(np.int64).sum()), df)
    assert got.tobytes() == expected_scores(po, d, f, doc_len, 5, queries, 1.2, 0.75).tobytes()


def test_merge_twin_agrees_with_sorted_tuples():
    rng = random.Random(20261020)
    seen = {"tie": 0, "same": 0, "short": 0, "cut": 0}
    for case in range(200):
        n_shards, nq, k_in, k_out = rng.choice((1, 2, 3, 7)), rng.choice((1, 3)), rng.choice((1, 4, 9)), rng.choice((1, 5, 40))
        levels = [np.float32(x).view(np.uint32).item() for x in (0.5, 1.0, 1.0000001, 3.25, 1e-30, 7e20)]
        docs = np.full((n_shards * nq, k_in), SENTINEL, dtype=np.uint32)
        bits = np.full((n_shards * nq, k_in), SENTINEL, dtype=np.uint32)
        cnt = []
        for r in range(n_shards * nq):
            n = rng.randrange(0, k_in + 1)
            row = sorted({(-rng.choice(levels), rng.randrange(0, 12)) for _ in range(n)})   # distinct, in row order
            cnt.append(len(row))
            for i, (nb, d) in enumerate(row):
                docs[r, i], bits[r, i] = d, -nb
        got_d, got_b, top_n = merge_twin(docs, bits, cnt, n_shards, nq, k_in, k_out)
        for q in range(nq):
            cand = sorted((-int(bits[s * nq + q, i]), int(docs[s * nq + q, i]), s)
                          for s in range(n_shards) for i in range(cnt[s * nq + q]))
            want = cand[:k_out]
            assert top_n[q] == len(want) == min(k_out, len(cand))
            assert got_d[q, :len(want)].tolist() == [d for _, d, _ in want]
            assert got_b[q, :len(want)].tolist() == [-nb for nb, _, _ in want]
            assert (got_d[q, len(want):] == SENTINEL).all() and (got_b[q, len(want):] == SENTINEL).all()
            keys = [(nb, d) for nb, d, _ in cand]
            seen["tie"] += len({nb for nb, _ in keys}) < len(keys)
            seen["same"] += len(set(keys)) < len(keys)
            seen["short"] += len(cand) < k_out
            seen["cut"] += len(cand) > k_out
    assert all(v > 10 for v in seen.values()), seen
