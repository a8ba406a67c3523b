"""Helpers of the postings tests (mrg_vocab_postings).  No expectation comes from the library: the expected
inverted index is built in numpy from the CSR arrays -- rows by np.repeat, order by a stable argsort of the
terms, offsets by np.bincount and a cumulative sum; tests/test_postings_cpu.py checks that helper against a
plain dict of lists."""
import numpy as np

SENTINEL = 0xFFFFFFFD          # fills d_docs and d_tf: never a document or a count of the tests that look for it
SENTINEL64 = 0xFDFDFDFDFDFDFDFD  # fills d_post_off
SLACK = 16                     # sentinel entries after the last one, which the call must leave alone


def expected_postings(terms, counts, row_off, n_words, doc_base=0):
    """(post_off, docs, tf) of the rows terms[row_off[i]:row_off[i + 1]], the document of row i = doc_base + i"""
    terms = np.asarray(terms, dtype=np.uint32)
    counts = np.asarray(counts, dtype=np.uint32)
    row_off = np.asarray(row_off, dtype=np.int64)
    lo, hi = int(row_off[0]), int(row_off[-1])
    t, c = terms[lo:hi], counts[lo:hi]
    rows = np.repeat(np.arange(len(row_off) - 1, dtype=np.int64), np.diff(row_off))
    order = np.argsort(t, kind="stable")
    post_off = np.concatenate([[0], np.cumsum(np.bincount(t, minlength=n_words), dtype=np.int64)]).astype(np.uint64)
    assert len(post_off) == n_words + 1, "a term outside the vocabulary"
    return post_off, (rows[order] + doc_base).astype(np.uint32), c[order].astype(np.uint32)


def expected_postings_dict(terms, counts, row_off, n_words, doc_base=0):
    """the same by a plain dict of lists over Python ints: the check of expected_postings itself"""
    terms, counts = [int(x) for x in terms], [int(x) for x in counts]
    lists = {}
    for i in range(len(row_off) - 1):
        for at in range(row_off[i], row_off[i + 1]):
            lists.setdefault(terms[at], []).append((doc_base + i, counts[at]))
    post_off, docs, tf = [0], [], []
    for w in range(n_words):
        for d, c in lists.get(w, []):
            docs.append(d)
            tf.append(c)
        post_off.append(len(docs))
    return post_off, docs, tf


def to_device_u32(a):
    """uint32 values on the device (at least one element, so that the pointer is real)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.size == 0:
        a = np.zeros(4, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


def postings_dev(ctx, v, terms_ptr, counts_ptr, row_off, doc_base=0):
    """the df-only call, then the full call with cap = the exact size, into sentinel-filled buffers that are
    SLACK entries longer, then the documents-only call; returns (post_off, docs, tf) as numpy arrays"""
    import torch
    n_words = v.size()[0]
    fill64 = SENTINEL64 - (1 << 64)
    po1 = torch.full((n_words + 1 + SLACK,), fill64, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()                                 # the context runs on a stream of its own
    e = ctx.postings(v, terms_ptr, None, row_off, po1.data_ptr())
    assert e == row_off[-1] - row_off[0]
    po2 = torch.full((n_words + 1 + SLACK,), fill64, dtype=torch.int64, device="cuda:0")
    docs = torch.full((e + SLACK,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    tf = torch.full((e + SLACK,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    e2 = ctx.postings(v, terms_ptr, counts_ptr, row_off, po2.data_ptr(), docs.data_ptr(), tf.data_ptr(), e, doc_base)
    assert e2 == e
    torch.cuda.synchronize()
    a, b = po1.cpu().numpy().view(np.uint64), po2.cpu().numpy().view(np.uint64)
    assert (a == b).all(), "the df-only call and the full call disagree"
    assert (a[n_words + 1:] == SENTINEL64).all(), "wrote past the last offset"
    d, t = docs.cpu().numpy().view(np.uint32), tf.cpu().numpy().view(np.uint32)
    assert (d[e:] == SENTINEL).all() and (t[e:] == SENTINEL).all(), "wrote past the last posting"
    assert a[0] == 0 and a[n_words] == e
    # the documents-only mode (d_tf = NULL; d_counts is not read): the same offsets and documents
    po3 = torch.full((n_words + 1 + SLACK,), fill64, dtype=torch.int64, device="cuda:0")
    docs3 = torch.full((e + SLACK,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.postings(v, terms_ptr, None, row_off, po3.data_ptr(), docs3.data_ptr(), None, e, doc_base) == e
    torch.cuda.synchronize()
    assert (po3.cpu().numpy().view(np.uint64) == a).all(), "the documents-only call's offsets differ"
    assert (docs3.cpu().numpy().view(np.uint32) == d).all(), "the documents-only call's documents differ"
    return a[:n_words + 1], d[:e], t[:e]


def first_bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if bad.size == 0 else (int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), int(bad.size))


def check_dev(ctx, v, terms_ptr, counts_ptr, terms, counts, row_off, doc_base=0):
    """postings of the device CSR against the index expected from its host copy"""
    e_off, e_docs, e_tf = expected_postings(terms, counts, row_off, v.size()[0], doc_base)
    off, docs, tf = postings_dev(ctx, v, terms_ptr, counts_ptr, row_off, doc_base)
    assert len(off) == len(e_off) and first_bad(off, e_off) is None, ("post_off", first_bad(off, e_off))
    assert len(docs) == len(e_docs) and first_bad(docs, e_docs) is None, ("docs", first_bad(docs, e_docs))
    assert first_bad(tf, e_tf) is None, ("tf", first_bad(tf, e_tf))
    return off, docs, tf


def check(ctx, v, terms, counts, row_off, doc_base=0):
    t, c = to_device_u32(terms), to_device_u32(counts)
    res = check_dev(ctx, v, t.data_ptr(), c.data_ptr(), terms, counts, row_off, doc_base)
    del t, c
    return res
