"""Helpers of the search tests (mrg_vocab_search).  No expectation comes from the library: the expected scores
are the dense queries x n_docs BM25 matrix in numpy float64, built from the host copies of the index by the
formula of include/mrgpu.h; tests/test_search_cpu.py checks that helper against plain Python floats and dicts.

RTOL = 1e-5 is derived, not measured.  A weight takes at most 16 float32 roundings (the conversions of idf,
avgdl, tf and dl, the arithmetic, a device logf should an implementation use one); a sum of L positive terms
takes L - 1 more; every term is positive, so nothing cancels.  With L <= 64 positions per query the relative
error stays below 80 * 2^-24 = 4.8e-6, and RTOL is twice that."""
import math

import numpy as np

UNK = 0xFFFFFFFF
RTOL = 1e-5
MAX_POSITIONS = 64             # the longest query of the tests: RTOL is derived for it
SENTINEL = 0xFFFFFFFD          # fills both output rows: never a document of the tests, and no score (a NaN)
SLACK = 16                     # sentinel entries after the last row, which the call must leave alone


def expected_scores(post_off, docs, tf, doc_len, doc_base, queries, k1, b):
    """scores[q, i] of document doc_base + i for every query (a sequence of ids, UNK allowed), float64"""
    post_off = np.asarray(post_off, dtype=np.uint64).astype(np.int64)
    docs = np.asarray(docs, dtype=np.uint32).astype(np.int64)
    tf = np.asarray(tf, dtype=np.uint32).astype(np.float64)
    dl = np.asarray(doc_len, dtype=np.uint32).astype(np.float64)
    n = len(dl)
    out = np.zeros((len(queries), n), dtype=np.float64)
    if n == 0:
        return out
    total = int(np.asarray(doc_len, dtype=np.uint32).astype(np.uint64).sum())
    avgdl = total / n
    norm = k1 * (1.0 - b + b * (dl / avgdl if avgdl > 0 else np.zeros(n)))
    for qi, q in enumerate(queries):
        for t in q:
            t = int(t)
            if t == UNK:
                continue
            a, e = int(post_off[t]), int(post_off[t + 1])
            df = e - a
            if df == 0:
                continue
            idf = math.log(1.0 + (n - df + 0.5) / (df + 0.5))
            d, f = docs[a:e] - doc_base, tf[a:e]
            den = f + norm[d]
            w = np.where(f > 0, idf * f * (k1 + 1.0) / np.where(den > 0, den, 1.0), 0.0)
            np.add.at(out[qi], d, w)
    return out


def expected_scores_dict(post_off, docs, tf, doc_len, doc_base, queries, k1, b):
    """the same by plain Python floats and one dict per query: the check of expected_scores itself"""
    post_off, docs, tf, doc_len = ([int(x) for x in a] for a in (post_off, docs, tf, doc_len))
    n = len(doc_len)
    avgdl = sum(doc_len) / n if n else 0.0
    rows = []
    for q in queries:
        row = {}
        for t in q:
            t = int(t)
            if t == UNK or post_off[t + 1] == post_off[t]:
                continue
            df = post_off[t + 1] - post_off[t]
            idf = math.log(1.0 + (n - df + 0.5) / (df + 0.5))
            for at in range(post_off[t], post_off[t + 1]):
                i, f = docs[at] - doc_base, float(tf[at])
                if f == 0.0:
                    continue
                ratio = doc_len[i] / avgdl if avgdl > 0 else 0.0
                row[i] = row.get(i, 0.0) + idf * f * (k1 + 1.0) / (f + k1 * (1.0 - b + b * ratio))
        rows.append(row)
    return rows


def check_topk(got_docs, got_scores, top_n, ref, k, doc_base):
    """the rows the call returned (got_docs, got_scores: queries x k, only the first top_n[q] of a row are read)
    against the float64 scores ref (queries x n_docs)"""
    ref = np.asarray(ref, dtype=np.float64)
    nq, n_docs = ref.shape
    assert len(top_n) == nq
    for q in range(nq):
        hits = int((ref[q] > 0).sum())
        n = int(top_n[q])
        assert n == min(k, hits), ("top_n", q, n, min(k, hits))                                  # (a)
        if n == 0:
            continue
        d = np.asarray(got_docs[q][:n], dtype=np.int64) - doc_base
        s = np.asarray(got_scores[q][:n], dtype=np.float64)
        assert len(set(d.tolist())) == n, ("a document twice", q)                                   # (b)
        assert (d >= 0).all() and (d < n_docs).all(), ("a document out of range", q)
        r = ref[q][d]
        assert (r > 0).all(), ("a document that is no hit", q, d[r <= 0][:4].tolist())
        bad = np.nonzero(np.abs(s - r) > RTOL * r)[0]
        assert bad.size == 0, ("score", q, int(d[bad[0]]), float(s[bad[0]]), float(r[bad[0]]))
        assert (s[1:] <= s[:-1]).all(), ("the scores increase", q)                                  # (c)
        tie = s[1:] == s[:-1]
        assert (d[1:][tie] > d[:-1][tie]).all(), ("equal scores not in document order", q)
        rest = np.ones(n_docs, dtype=bool)                                                          # (d)
        rest[d] = False
        if rest.any():
            worst = float(ref[q][rest].max())
            assert worst <= (1.0 + 2.0 * RTOL) * float(r.min()), ("a better document is missing", q, worst, float(r.min()))


def topk_f32(scores32, k):
    """the rows a float32 evaluation itself would return: (docs, scores, top_n), score descending, document
    ascending, hits only"""
    scores32 = np.asarray(scores32, dtype=np.float32)
    nq, n_docs = scores32.shape
    docs = np.full((nq, k), SENTINEL, dtype=np.uint32)
    sc = np.zeros((nq, k), dtype=np.float32)
    top_n = []
    for q in range(nq):
        order = np.lexsort((np.arange(n_docs), -scores32[q].astype(np.float64)))
        order = order[scores32[q][order] > 0][:k]
        docs[q, :len(order)] = order
        sc[q, :len(order)] = scores32[q][order]
        top_n.append(len(order))
    return docs, sc, top_n


def scores_f32(post_off, docs, tf, doc_len, doc_base, queries, k1, b):
    """the formula evaluated in float32, summed in query order: what an implementation may compute"""
    f32 = np.float32
    post_off = np.asarray(post_off, dtype=np.uint64).astype(np.int64)
    docs = np.asarray(docs, dtype=np.uint32).astype(np.int64)
    tf = np.asarray(tf, dtype=np.uint32).astype(f32)
    dl = np.asarray(doc_len, dtype=np.uint32).astype(f32)
    n = len(dl)
    out = np.zeros((len(queries), n), dtype=f32)
    if n == 0:
        return out
    total = int(np.asarray(doc_len, dtype=np.uint32).astype(np.uint64).sum())
    avgdl = f32(total / n) if total else f32(1)
    k1, b = f32(k1), f32(b)
    norm = k1 * ((f32(1) - b) + b * (dl / avgdl))
    for qi, q in enumerate(queries):
        for t in q:
            t = int(t)
            if t == UNK or post_off[t + 1] == post_off[t]:
                continue
            df = int(post_off[t + 1] - post_off[t])
            idf = f32(math.log(1.0 + (n - df + 0.5) / (df + 0.5)))
            a, e = int(post_off[t]), int(post_off[t + 1])
            d, f = docs[a:e] - doc_base, tf[a:e]
            den = f + norm[d]
            w = np.where(f > 0, idf * (f * (k1 + f32(1))) / np.where(den > 0, den, f32(1)), f32(0)).astype(f32)
            out[qi, d] = out[qi, d] + w                      # (a word's documents are distinct)
    return out


# ---- the device side

def dev_u32(a):
    """uint32 values on the device (at least one element, so that the pointer is real)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.size == 0:
        a = np.zeros(4, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


class Index:
    """an inverted index and its collection on the device, with the host copies the expectations come from;
    pad_docs / pad_tf: uint32 entries in front of the arrays, so that they start 4 * pad bytes off a 16-byte boundary"""

    def __init__(self, post_off, docs, tf, doc_len, doc_base=0, pad_docs=0, pad_tf=0):
        import torch
        self.post_off = np.asarray(post_off, dtype=np.uint64)
        self.docs = np.asarray(docs, dtype=np.uint32)
        self.tf = np.asarray(tf, dtype=np.uint32)
        self.doc_len = np.asarray(doc_len, dtype=np.uint32)
        self.doc_base = doc_base
        self.n_docs = len(self.doc_len)
        self.n_entries = len(self.docs)
        self.d_post_off = torch.from_numpy(self.post_off.view(np.int64).copy()).to("cuda:0")
        self.d_docs = dev_u32(np.concatenate([np.full(pad_docs, SENTINEL, dtype=np.uint32), self.docs]))
        self.d_tf = dev_u32(np.concatenate([np.full(pad_tf, SENTINEL, dtype=np.uint32), self.tf]))
        self.d_doc_len = dev_u32(self.doc_len)
        assert self.d_docs.data_ptr() % 16 == 0 and self.d_tf.data_ptr() % 16 == 0
        self.p_docs, self.p_tf = self.d_docs.data_ptr() + 4 * pad_docs, self.d_tf.data_ptr() + 4 * pad_tf
        torch.cuda.synchronize()                             # the context runs on a stream of its own

    def ref(self, queries, k1=1.2, b=0.75):
        return expected_scores(self.post_off, self.docs, self.tf, self.doc_len, self.doc_base, queries, k1, b)


def lay_queries(queries, first=0):
    """(ids, q_off) of the queries back to back, `first` unrelated ids in front"""
    ids = [7] * first
    off = [first]
    for q in queries:
        ids.extend(int(t) for t in q)
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), off


def search_raw(ctx, v, ix, q_ids_t, q_off, k, k1=1.2, b=0.75, ptrs=None):
    """one call into sentinel-filled output rows that are SLACK entries longer: (docs, scores as bits, top_n),
    the arrays whole (queries * k + SLACK uint32 each)"""
    import torch
    nq = len(q_off) - 1
    fill = SENTINEL - (1 << 32)
    docs = torch.full((nq * k + SLACK,), fill, dtype=torch.int32, device="cuda:0")
    sc = torch.full((nq * k + SLACK,), fill, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = dict(post_off=ix.d_post_off.data_ptr(), docs=ix.p_docs, tf=ix.p_tf,
             doc_len=ix.d_doc_len.data_ptr(), q_ids=q_ids_t.data_ptr(), top_docs=docs.data_ptr(), top_scores=sc.data_ptr(),
             n_entries=ix.n_entries, n_docs=ix.n_docs, doc_base=ix.doc_base)
    p.update(ptrs or {})
    try:
        top_n = ctx.search(v, p["post_off"], p["docs"], p["tf"], p["n_entries"], p["doc_len"], p["n_docs"], p["q_ids"], q_off,
                           k, p["top_docs"], p["top_scores"], k1=k1, b=b, doc_base=p["doc_base"])
    finally:
        torch.cuda.synchronize()
        search_raw.last = (docs.cpu().numpy().view(np.uint32), sc.cpu().numpy().view(np.uint32))
    return search_raw.last[0], search_raw.last[1], top_n


def search_dev(ctx, v, ix, queries, k, k1=1.2, b=0.75, first=0):
    """the call, twice: nothing written from top_n[q] on or into the slack, identical bytes both times; returns
    (docs, scores, top_n) with docs and scores as queries x k arrays"""
    ids, q_off = lay_queries(queries, first)
    t = dev_u32(ids)
    d1, s1, n1 = search_raw(ctx, v, ix, t, q_off, k, k1, b)
    d2, s2, n2 = search_raw(ctx, v, ix, t, q_off, k, k1, b)
    del t
    assert n1 == n2 and (d1 == d2).all() and (s1 == s2).all(), "two calls differ"
    nq = len(queries)
    assert (d1[nq * k:] == SENTINEL).all() and (s1[nq * k:] == SENTINEL).all(), "wrote past the last row"
    docs, bits = d1[:nq * k].reshape(nq, k), s1[:nq * k].reshape(nq, k)
    for q in range(nq):
        assert 0 <= n1[q] <= k
        assert (docs[q, n1[q]:] == SENTINEL).all() and (bits[q, n1[q]:] == SENTINEL).all(), ("wrote past top_n", q)
    return docs, bits.view(np.float32), n1


def check(ctx, v, ix, queries, k, k1=1.2, b=0.75, first=0, ref=None):
    assert max((len(q) for q in queries), default=0) <= MAX_POSITIONS
    docs, scores, top_n = search_dev(ctx, v, ix, queries, k, k1, b, first)
    check_topk(docs, scores, top_n, ix.ref(queries, k1, b) if ref is None else ref, k, ix.doc_base)
    return docs, scores, top_n
