"""Helpers of the sharded-search tests (mrg_vocab_stats_add, mrg_vocab_search_shard, mrg_search_merge).  No
expectation comes from the library alone: the shards are cut on the host from the CSR with
postings_util.expected_postings, the expected scores are search_util.expected_scores with the collection's N,
avgdl and df passed in, and the expected merge is a numpy.lexsort; tests/test_shards_cpu.py checks these helpers
against the one-piece helper and against sorted() of tuples.  The byte-identity checks of the GPU tests compare
the sharded path with the one-piece mrg_vocab_search, which tests/test_gpu_search.py holds to the float64
reference."""
import math

import numpy as np

from postings_util import expected_postings
from search_util import SENTINEL, SLACK, UNK


def expected_scores_coll(post_off, docs, tf, doc_len, doc_base, queries, k1, b, coll_docs, coll_sum_len, df):
    """search_util.expected_scores of one shard with the statistics passed in: N = coll_docs, avgdl =
    coll_sum_len / coll_docs, df[t] the collection's document frequency of word t; float64"""
    post_off = np.asarray(post_off, dtype=np.uint64).astype(np.int64)
    docs = np.asarray(docs, dtype=np.uint32).astype(np.int64)
    tf = np.asarray(tf, dtype=np.uint32).astype(np.float64)
    dl = np.asarray(doc_len, dtype=np.uint32).astype(np.float64)
    n = len(dl)
    out = np.zeros((len(queries), n), dtype=np.float64)
    if n == 0:
        return out
    big_n = int(coll_docs)
    avgdl = int(coll_sum_len) / big_n
    norm = k1 * (1.0 - b + b * (dl / avgdl if avgdl > 0 else np.zeros(n)))
    for qi, q in enumerate(queries):
        for t in q:
            t = int(t)
            if t == UNK:
                continue
            a, e = int(post_off[t]), int(post_off[t + 1])
            if e == a:                                       # no postings in this shard, whatever df says
                continue
            d_f = int(df[t])
            idf = math.log(1.0 + (big_n - d_f + 0.5) / (d_f + 0.5))
            d, f = docs[a:e] - doc_base, tf[a:e]
            den = f + norm[d]
            w = np.where(f > 0, idf * f * (k1 + 1.0) / np.where(den > 0, den, 1.0), 0.0)
            np.add.at(out[qi], d, w)
    return out


def split_host(csr, cuts, n_words, doc_base=0):
    """the shards of a CSR (terms, counts, row_off, doc_len) cut at the rows `cuts` (cuts[0] = 0, cuts[-1] =
    the rows): per shard (post_off, docs, tf, doc_len, base) with base = doc_base + the shard's first row"""
    terms, counts, row_off, doc_len = csr
    assert cuts[0] == 0 and cuts[-1] == len(row_off) - 1 and list(cuts) == sorted(cuts)
    out = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        po, d, f = expected_postings(terms, counts, row_off[a:e + 1], n_words, doc_base + a)
        out.append((po, d, f, np.asarray(doc_len[a:e], dtype=np.uint32), doc_base + a))
    return out


def split_index(csr, cuts, n_words, doc_base=0):
    """the same as search_util.Index objects on the device"""
    from search_util import Index
    return [Index(*s) for s in split_host(csr, cuts, n_words, doc_base)]


def coll_stats(shards):
    """(df, docs, sum_len) of host shards (tuples of split_host, or Index objects): plain integer sums"""
    get = lambda s: (s.post_off, s.doc_len) if hasattr(s, "post_off") else (s[0], s[3])
    df, n, total = None, 0, 0
    for s in shards:
        po, dl = get(s)
        d = np.diff(np.asarray(po, dtype=np.uint64).astype(np.int64))
        df = d if df is None else df + d
        n += len(dl)
        total += int(np.asarray(dl, dtype=np.uint64).sum())
    return df, n, total


def merge_twin(in_docs, in_bits, in_top_n, n_shards, n_queries, k_in, k_out):
    """what mrg_search_merge returns for the rows in_docs / in_bits (uint32, (n_shards * n_queries, k_in)) with
    in_top_n used entries each: (docs, bits, top_n), rows of k_out slots, SENTINEL where nothing is written;
    the order is numpy.lexsort by (score bits descending, document ascending, shard ascending)"""
    in_docs = np.asarray(in_docs, dtype=np.uint32).reshape(n_shards * n_queries, k_in)
    in_bits = np.asarray(in_bits, dtype=np.uint32).reshape(n_shards * n_queries, k_in)
    docs = np.full((n_queries, k_out), SENTINEL, dtype=np.uint32)
    bits = np.full((n_queries, k_out), SENTINEL, dtype=np.uint32)
    top_n = []
    for q in range(n_queries):
        d, s, sh = [], [], []
        for shard in range(n_shards):
            r = shard * n_queries + q
            n = int(in_top_n[r])
            d.append(in_docs[r, :n])
            s.append(in_bits[r, :n])
            sh.append(np.full(n, shard, dtype=np.int64))
        d, s, sh = np.concatenate(d).astype(np.int64), np.concatenate(s).astype(np.int64), np.concatenate(sh)
        order = np.lexsort((sh, d, -s))[:k_out]            # the last key is the primary one
        docs[q, :len(order)] = d[order]
        bits[q, :len(order)] = s[order]
        top_n.append(len(order))
    return docs, bits, top_n


# ---- the device side

def dev_zeros_u64(n):
    import torch
    t = torch.zeros((max(n, 1),), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()                                 # the context runs on a stream of its own
    return t


def stats_dev(ctx, v, shards, order=None):
    """stats_add over the Index shards in the given order: (df as uint64 array, (docs, sum_len))"""
    import torch
    n_words = v.size()[0]
    df = dev_zeros_u64(n_words)
    coll = (0, 0)
    for i in (range(len(shards)) if order is None else order):
        s = shards[i]
        coll = ctx.stats_add(v, s.d_post_off.data_ptr(), s.d_doc_len.data_ptr(), s.n_docs, df.data_ptr(), coll)
    torch.cuda.synchronize()
    return df, coll


def filled(n):
    import torch
    return torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")


def shards_search_raw(ctx, v, shards, df, coll, q_ids_t, q_off, k, k1=1.2, b=0.75):
    """every shard searched with k into its slice of one sentinel-filled buffer with SLACK entries after the last
    row: (docs tensor, scores tensor, in_top_n)"""
    import torch
    nq = len(q_off) - 1
    n = len(shards) * nq * k
    docs, sc = filled(n + SLACK), filled(n + SLACK)
    torch.cuda.synchronize()
    top = []
    for i, s in enumerate(shards):
        at = 4 * i * nq * k
        top += ctx.search_shard(v, s.d_post_off.data_ptr(), s.p_docs, s.p_tf, s.n_entries, s.d_doc_len.data_ptr(), s.n_docs,
                                q_ids_t.data_ptr(), q_off, k, docs.data_ptr() + at, sc.data_ptr() + at, df.data_ptr(), coll,
                                k1=k1, b=b, doc_base=s.doc_base)
    torch.cuda.synchronize()
    return docs, sc, top


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def merge_raw(ctx, n_shards, nq, k_in, d_in_docs, d_in_scores, in_top_n, k_out):
    """one merge into sentinel-filled rows with slack: (docs, bits, top_n), the arrays whole"""
    import torch
    docs, sc = filled(nq * k_out + SLACK), filled(nq * k_out + SLACK)
    torch.cuda.synchronize()
    try:
        top_n = ctx.search_merge(n_shards, nq, k_in, d_in_docs.data_ptr(), d_in_scores.data_ptr(), in_top_n, k_out,
                                 docs.data_ptr(), sc.data_ptr())
    finally:
        torch.cuda.synchronize()
        merge_raw.last = (host_u32(docs), host_u32(sc))
    return merge_raw.last[0], merge_raw.last[1], top_n


def merge_dev(ctx, n_shards, nq, k_in, d_in_docs, d_in_scores, in_top_n, k_out):
    """the merge, twice: identical bytes, nothing written from top_n[q] on or into the slack; returns (docs, bits,
    top_n) with docs and bits as nq x k_out arrays, SENTINEL where nothing was written"""
    d1, s1, n1 = merge_raw(ctx, n_shards, nq, k_in, d_in_docs, d_in_scores, in_top_n, k_out)
    d2, s2, n2 = merge_raw(ctx, n_shards, nq, k_in, d_in_docs, d_in_scores, in_top_n, k_out)
    assert n1 == n2 and (d1 == d2).all() and (s1 == s2).all(), "two calls differ"
    assert (d1[nq * k_out:] == SENTINEL).all() and (s1[nq * k_out:] == SENTINEL).all(), "wrote past the last row"
    docs, bits = d1[:nq * k_out].reshape(nq, k_out), s1[:nq * k_out].reshape(nq, k_out)
    for q in range(nq):
        assert 0 <= n1[q] <= k_out
        assert (docs[q, n1[q]:] == SENTINEL).all() and (bits[q, n1[q]:] == SENTINEL).all(), ("wrote past top_n", q)
    return docs, bits, n1
