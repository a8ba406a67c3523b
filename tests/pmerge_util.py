"""Helpers of the postings-merge tests (mrg_vocab_postings_merge).  No expectation comes from the library: the
expected merge is a per-word concatenation of host copies of the shards in plain numpy (expected_merge), which
tests/test_pmerge_cpu.py holds against postings_util.expected_postings of the CSR in one piece.  The device
wrapper runs the three modes of the call -- offsets only, documents only, everything -- into sentinel-filled
buffers with slack, and the full mode twice."""
import numpy as np

from postings_util import SENTINEL, SENTINEL64, SLACK, first_bad


def expected_merge(shards, n_words):
    """(post_off, docs, tf) of the shards (post_off, docs, tf, ...) merged: the offsets summed, the postings of
    every word those of shard 0, then shard 1, ..."""
    offs = [np.asarray(s[0], dtype=np.uint64).astype(np.int64) for s in shards]
    assert all(len(o) == n_words + 1 for o in offs)
    post_off = np.zeros(n_words + 1, dtype=np.int64)
    docs, tf = [np.zeros(0, dtype=np.uint32)], [np.zeros(0, dtype=np.uint32)]
    for w in range(n_words):
        for s, o in zip(shards, offs):
            docs.append(np.asarray(s[1], dtype=np.uint32)[o[w]:o[w + 1]])
            tf.append(np.asarray(s[2], dtype=np.uint32)[o[w]:o[w + 1]])
        post_off[w + 1] = post_off[w] + sum(int(o[w + 1] - o[w]) for o in offs)
    return post_off.astype(np.uint64), np.concatenate(docs), np.concatenate(tf)


def synth_shard(rng, df, base, span):
    """a shard built directly: word w has df[w] documents out of [base, base + span), ascending, and tf 1 .. 9;
    (post_off, docs, tf)"""
    df = np.asarray(df, dtype=np.int64)
    assert df.max(initial=0) <= span
    post_off = np.concatenate([[0], np.cumsum(df)]).astype(np.uint64)
    docs = [base + np.sort(rng.choice(span, int(n), replace=False)) for n in df if n]
    docs = np.concatenate(docs).astype(np.uint32) if docs else np.zeros(0, dtype=np.uint32)
    return post_off, docs, rng.integers(1, 10, len(docs)).astype(np.uint32)


# ---- the device side

def filled(n):
    import torch
    return torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")


def filled64(n):
    import torch
    return torch.full((n,), SENTINEL64 - (1 << 64), dtype=torch.int64, device="cuda:0")


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


class DevShard:
    """one shard on the device with the host copies the expectations come from; pad_docs / pad_tf: uint32 entries
    in front of the arrays, so that they start 4 * pad bytes off a 16-byte boundary; null: a shard without entries
    whose document and tf pointers are NULL"""

    def __init__(self, post_off, docs, tf, pad_docs=0, pad_tf=0, null=False):
        import torch
        self.post_off = np.asarray(post_off, dtype=np.uint64)
        self.docs = np.asarray(docs, dtype=np.uint32)
        self.tf = np.asarray(tf, dtype=np.uint32)
        self.n = len(self.docs)
        assert len(self.tf) == self.n and int(self.post_off[-1]) == self.n and not (null and self.n)
        self.d_post_off = torch.from_numpy(self.post_off.view(np.int64).copy()).to("cuda:0")
        pad = lambda a, k: np.concatenate([np.full(k, SENTINEL, dtype=np.uint32), a, np.full(4, SENTINEL, dtype=np.uint32)])
        self.d_docs = torch.from_numpy(pad(self.docs, pad_docs).view(np.int32).copy()).to("cuda:0")
        self.d_tf = torch.from_numpy(pad(self.tf, pad_tf).view(np.int32).copy()).to("cuda:0")
        assert self.d_docs.data_ptr() % 16 == 0 and self.d_tf.data_ptr() % 16 == 0
        self.p_docs = None if null else self.d_docs.data_ptr() + 4 * pad_docs
        self.p_tf = None if null else self.d_tf.data_ptr() + 4 * pad_tf
        torch.cuda.synchronize()                             # the context runs on a stream of its own

    def host(self):
        return self.post_off, self.docs, self.tf

    def arg(self, mode=2):
        """(post_off_ptr, docs_ptr, tf_ptr, n_entries) for Context.postings_merge; mode 0: no postings, 1: no tf"""
        return (self.d_post_off.data_ptr(), self.p_docs if mode >= 1 else None, self.p_tf if mode >= 2 else None, self.n)


def merge_raw(ctx, v, shards, mode=2):
    """one call into sentinel-filled buffers that are SLACK entries longer; mode 0: offsets only, 1: documents
    only, 2: everything.  Returns (total, post_off, docs, tf), the arrays whole"""
    import torch
    n_words = v.size()[0]
    e = sum(s.n for s in shards)
    po, docs, tf = filled64(n_words + 1 + SLACK), filled(e + SLACK), filled(e + SLACK)
    torch.cuda.synchronize()
    try:
        total = ctx.postings_merge(v, [s.arg(mode) for s in shards], po.data_ptr(), docs.data_ptr() if mode >= 1 else None,
                                   tf.data_ptr() if mode >= 2 else None, e if mode >= 1 else 0)
    finally:
        torch.cuda.synchronize()
        merge_raw.last = (host_u64(po), host_u32(docs), host_u32(tf))
    return (total,) + merge_raw.last


def merge_dev(ctx, v, shards):
    """the three modes, the full one twice: nothing is written beyond words + 1 offsets or E postings, a mode
    leaves the arrays it does not merge alone, the modes agree, two calls give identical bytes.  Returns
    (post_off, docs, tf)"""
    n_words = v.size()[0]
    e = sum(s.n for s in shards)
    t0, po0, d0, f0 = merge_raw(ctx, v, shards, 0)
    t1, po1, d1, f1 = merge_raw(ctx, v, shards, 1)
    t2, po2, d2, f2 = merge_raw(ctx, v, shards, 2)
    t3, po3, d3, f3 = merge_raw(ctx, v, shards, 2)
    assert t0 == t1 == t2 == t3 == e
    for po in (po0, po1, po2, po3):
        assert (po[n_words + 1:] == SENTINEL64).all(), "wrote past the last offset"
        assert po[0] == 0 and po[n_words] == e
        assert (po == po0).all(), "the modes disagree about the offsets"
    assert (d0 == SENTINEL).all() and (f0 == SENTINEL).all(), "the offsets-only mode wrote postings"
    assert (f1 == SENTINEL).all(), "the documents-only mode wrote term frequencies"
    for d in (d1, d2, d3):
        assert (d[e:] == SENTINEL).all(), "wrote past the last posting"
        assert (d == d2).all(), "the documents differ between two calls or modes"
    assert (f2[e:] == SENTINEL).all() and (f3 == f2).all(), "tf: wrote past the end, or two calls differ"
    return po2[:n_words + 1], d2[:e], f2[:e]


def check(ctx, v, shards, want=None):
    """the merge of the device shards against expected_merge of their host copies (or `want`)"""
    n_words = v.size()[0]
    e_off, e_docs, e_tf = expected_merge([s.host() for s in shards], n_words) if want is None else want
    off, docs, tf = merge_dev(ctx, v, shards)
    assert len(off) == len(e_off) and first_bad(off, e_off) is None, ("post_off", first_bad(off, e_off))
    assert len(docs) == len(e_docs) and first_bad(docs, e_docs) is None, ("docs", first_bad(docs, e_docs))
    assert len(tf) == len(e_tf) and first_bad(tf, e_tf) is None, ("tf", first_bad(tf, e_tf))
    return off, docs, tf
