"""Helpers of the term-count tests (mrg_vocab_term_counts).  No expectation comes from the library: the
expected rows are built from the id arrays in numpy, per document np.unique(ids[ids != UNK],
return_counts=True) and (ids == UNK).sum(); tests/test_terms_cpu.py checks that helper against a plain
collections.Counter."""
import collections

import numpy as np

UNK = 0xFFFFFFFF
SENTINEL = 0xFFFFFFFD  # fills both destinations: never an id or a count here, not UNK, not decode's poison
SLACK = 16             # sentinel entries after the last row entry, which the call must leave alone


def expected_rows(ids, tok_off):
    """(row_off, terms, counts, unk) of the documents ids[tok_off[i]:tok_off[i + 1]]"""
    ids = np.asarray(ids, dtype=np.uint32)
    row_off, terms, counts, unk = [0], [], [], []
    for d in range(len(tok_off) - 1):
        seg = ids[tok_off[d]:tok_off[d + 1]]
        if len(seg) == 0:
            unk.append(0)
            row_off.append(row_off[-1])
            continue
        t, c = np.unique(seg[seg != UNK], return_counts=True)
        terms.append(t)
        counts.append(c)
        unk.append(int((seg == UNK).sum()))
        row_off.append(row_off[-1] + len(t))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return row_off, cat(terms, np.uint32), cat(counts, np.uint32), unk


def expected_rows_counter(ids, tok_off):
    """the same by collections.Counter over Python ints: the check of expected_rows itself"""
    ids = [int(x) for x in ids]
    row_off, terms, counts, unk = [0], [], [], []
    for d in range(len(tok_off) - 1):
        cnt = collections.Counter(ids[tok_off[d]:tok_off[d + 1]])
        unk.append(cnt.pop(UNK, 0))
        for t in sorted(cnt):
            terms.append(t)
            counts.append(cnt[t])
        row_off.append(len(terms))
    return row_off, terms, counts, unk


def make_vocab(ctx, n):
    """a vocabulary of n words w00000, w00001, ... (no job needed)"""
    return ctx.vocab_from_text(b"".join(b"w%05d 1\n" % i for i in range(n)))


def ids_to_device(ids):
    """uint32 ids on the device (at least one element, so that the pointer is real)"""
    import torch
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    if a.size == 0:
        a = np.zeros(4, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


def term_counts_dev(ctx, v, ids_ptr, tok_off):
    """sizes-only call, then the full call with cap = the exact size into two sentinel-filled buffers that
    are SLACK entries longer; returns (row_off, terms, counts, unk)"""
    import torch
    off, unk = ctx.term_counts(v, ids_ptr, tok_off)
    assert len(off) == len(tok_off) and off[0] == 0 and len(unk) == len(tok_off) - 1
    n = off[-1]
    terms = torch.full((n + SLACK,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    counts = torch.full((n + SLACK,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    off2, unk2 = ctx.term_counts(v, ids_ptr, tok_off, terms.data_ptr(), counts.data_ptr(), n)
    assert off2 == off and unk2 == unk, "the sizes-only call and the full call disagree"
    torch.cuda.synchronize()
    t = terms.cpu().numpy().view(np.uint32)
    c = counts.cpu().numpy().view(np.uint32)
    assert (t[n:] == SENTINEL).all() and (c[n:] == SENTINEL).all(), "wrote past the last row entry"
    return off, t[:n], c[:n], unk


def check_dev(ctx, v, ids_ptr, ids, tok_off):
    """term counts of the device ids at ids_ptr against the rows expected from the host copy `ids`"""
    e_off, e_terms, e_counts, e_unk = expected_rows(ids, tok_off)
    off, terms, counts, unk = term_counts_dev(ctx, v, ids_ptr, tok_off)
    assert off == e_off, first_diff(off, e_off)
    assert unk == e_unk, first_diff(unk, e_unk)
    bad = np.nonzero(terms != e_terms)[0]
    assert bad.size == 0, ("terms", int(bad[0]), int(terms[bad[0]]), int(e_terms[bad[0]]), bad.size)
    bad = np.nonzero(counts != e_counts)[0]
    assert bad.size == 0, ("counts", int(bad[0]), int(counts[bad[0]]), int(e_counts[bad[0]]), bad.size)
    cs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    for d in range(len(tok_off) - 1):                        # sum(counts of row d) + unk[d] = the document's ids
        assert int(cs[off[d + 1]] - cs[off[d]]) + unk[d] == tok_off[d + 1] - tok_off[d], d
    return off, terms, counts, unk


def check(ctx, v, ids, tok_off):
    t = ids_to_device(ids)
    res = check_dev(ctx, v, t.data_ptr(), ids, tok_off)
    del t
    return res


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return (i, x, y)
    return (len(a), len(b))
