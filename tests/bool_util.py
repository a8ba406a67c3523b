"""Helpers of the Boolean-search tests (mrg_vocab_search_bool, mrg_vocab_search_bool_shard).  No expectation comes
from the library under test: the predicate -- which documents stand in the postings of every MUST word and of no
MUST_NOT word -- is computed from the host copies of the postings, the scores are search_util.expected_scores of
the query without its MUST_NOT positions, zeroed where the predicate fails; tests/test_bool_cpu.py checks both
against plain Python sets and dicts.  The byte-exact checks take the ranking of the plain mrg_vocab_search, which
tests/test_gpu_search.py holds to the float64 reference, and filter it on the host.

A Boolean query is a list of (word, role) pairs."""
import numpy as np

from search_util import SENTINEL, SLACK, UNK, dev_u32, expected_scores

SHOULD, MUST, MUST_NOT = 0, 1, 2      # MRG_Q_SHOULD, MRG_Q_MUST, MRG_Q_MUST_NOT of include/mrgpu.h
UNREAD_ROLE = 9                        # fills the roles below q_off[0]: no role, and never read


def scoring(bq):
    """the ids of every Boolean query without its MUST_NOT positions: what the plain search scores"""
    return [[int(w) for w, r in q if r != MUST_NOT] for q in bq]


def predicate(post_off, docs, n_docs, doc_base, bq):
    """ok[q, i]: document doc_base + i stands in the postings of the word of every MUST position of query q and of
    no MUST_NOT position (whatever the tf; UNK and a word without postings hold no document)"""
    post_off = np.asarray(post_off, dtype=np.uint64).astype(np.int64)
    docs = np.asarray(docs, dtype=np.uint32).astype(np.int64)
    ok = np.ones((len(bq), n_docs), dtype=bool)
    for qi, q in enumerate(bq):
        for w, r in q:
            if r == SHOULD:
                continue
            member = np.zeros(n_docs, dtype=bool)
            if int(w) != UNK:
                member[docs[int(post_off[int(w)]):int(post_off[int(w) + 1])] - doc_base] = True
            ok[qi] &= member if r == MUST else ~member
    return ok


def masked_scores(post_off, docs, tf, doc_len, doc_base, bq, k1=1.2, b=0.75, scores=expected_scores):
    """the float64 scores of the Boolean queries: those of the scoring positions, 0 where the predicate fails"""
    ref = scores(post_off, docs, tf, doc_len, doc_base, scoring(bq), k1, b)
    return np.where(predicate(post_off, docs, len(doc_len), doc_base, bq), ref, 0.0)


def masked_ref(ix, bq, k1=1.2, b=0.75):
    return masked_scores(ix.post_off, ix.docs, ix.tf, ix.doc_len, ix.doc_base, bq, k1, b)


def filter_rows(docs, bits, top_n, ok, k, doc_base):
    """complete plain rankings (docs, bits: queries x K with top_n[q] entries, every hit of the query among them)
    -> the rows a Boolean search with k returns: the entries whose document passes ok[q], the first k of them;
    (docs, bits, top_n) with SENTINEL where nothing is written"""
    nq = len(top_n)
    out_d = np.full((nq, k), SENTINEL, dtype=np.uint32)
    out_b = np.full((nq, k), SENTINEL, dtype=np.uint32)
    out_n = []
    for q in range(nq):
        d, s = docs[q][:top_n[q]], bits[q][:top_n[q]]
        keep = np.nonzero(ok[q][d.astype(np.int64) - doc_base])[0][:k]
        out_d[q, :len(keep)], out_b[q, :len(keep)] = d[keep], s[keep]
        out_n.append(len(keep))
    return out_d, out_b, out_n


def lay_bool(bq, first=0):
    """(ids, roles, q_off) of the queries back to back, `first` unrelated ids, with roles that are none, in front"""
    ids, roles, off = [7] * first, [UNREAD_ROLE] * first, [first]
    for q in bq:
        ids.extend(int(w) for w, _ in q)
        roles.extend(int(r) for _, r in q)
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), bytes(roles), off


# ---- the device side

def bool_raw(ctx, v, ix, q_ids_t, roles, q_off, k, k1=1.2, b=0.75, shard=None):
    """one call into sentinel-filled output rows that are SLACK entries longer: (docs, scores as bits, top_n), the
    arrays whole; shard = (df_ptr, coll): mrg_vocab_search_bool_shard"""
    import torch
    nq = len(q_off) - 1
    fill = SENTINEL - (1 << 32)
    docs = torch.full((nq * k + SLACK,), fill, dtype=torch.int32, device="cuda:0")
    sc = torch.full((nq * k + SLACK,), fill, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    a = (v, ix.d_post_off.data_ptr(), ix.p_docs, ix.p_tf, ix.n_entries, ix.d_doc_len.data_ptr(), ix.n_docs, q_ids_t.data_ptr(),
         roles, q_off, k, docs.data_ptr(), sc.data_ptr())
    try:
        if shard is None:
            top_n = ctx.search_bool(*a, k1=k1, b=b, doc_base=ix.doc_base)
        else:
            top_n = ctx.search_bool_shard(*a, shard[0], shard[1], k1=k1, b=b, doc_base=ix.doc_base)
    finally:
        torch.cuda.synchronize()
        bool_raw.last = (docs.cpu().numpy().view(np.uint32), sc.cpu().numpy().view(np.uint32))
    return bool_raw.last[0], bool_raw.last[1], top_n


def bool_dev(ctx, v, ix, bq, k, k1=1.2, b=0.75, first=0, roles="given", shard=None):
    """the call, twice: nothing written from top_n[q] on or into the slack, identical bytes both times; returns
    (docs, bits, top_n) with docs and bits as queries x k uint32 arrays.  roles: "given", or what to pass instead
    (None, or bytes)"""
    ids, r, q_off = lay_bool(bq, first)
    if roles != "given":
        r = roles
    t = dev_u32(ids)
    d1, s1, n1 = bool_raw(ctx, v, ix, t, r, q_off, k, k1, b, shard)
    d2, s2, n2 = bool_raw(ctx, v, ix, t, r, q_off, k, k1, b, shard)
    del t
    assert n1 == n2 and (d1 == d2).all() and (s1 == s2).all(), "two calls differ"
    nq = len(bq)
    assert (d1[nq * k:] == SENTINEL).all() and (s1[nq * k:] == SENTINEL).all(), "wrote past the last row"
    docs, bits = d1[:nq * k].reshape(nq, k), s1[:nq * k].reshape(nq, k)
    for q in range(nq):
        assert 0 <= n1[q] <= k
        assert (docs[q, n1[q]:] == SENTINEL).all() and (bits[q, n1[q]:] == SENTINEL).all(), ("wrote past top_n", q)
    return docs, bits, n1
