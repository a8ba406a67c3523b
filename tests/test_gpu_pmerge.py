"""GPU tests of mrg_vocab_postings_merge (k_postings_merge.hip): the indexes of the shards of one collection ->
one index.

The claim under test is an identity: the merge of the indexes of consecutive row ranges of a CSR is, byte for
byte, the index mrg_vocab_postings builds from the CSR in one piece, which tests/test_gpu_postings.py holds to
the numpy reference; shards built directly are held to pmerge_util.expected_merge, a per-word concatenation.
Every merge runs in its three modes into sentinel-filled buffers with slack, the full mode twice
(pmerge_util.merge_dev).  The copy works on tiles of native.PMERGE_TILE source entries of one shard and takes
another path when a tile lies inside one word; a tile's 16-byte stores stand at the aligned output positions and
its loads depend on how the source is aligned against them: the shapes below are sized by the tile and the
arrays start 0, 4, 8 and 12 bytes off a 16-byte boundary.  Every bad input here is one the contract answers with
a status code."""
import ctypes as C

import numpy as np
import pytest

from pmerge_util import (DevShard, check, expected_merge, filled, filled64, host_u32, host_u64, merge_dev, merge_raw,
                         synth_shard)
from postings_util import SENTINEL, SENTINEL64, SLACK, expected_postings, to_device_u32
from search_util import UNK, dev_u32, search_dev
from terms_util import make_vocab

pytestmark = pytest.mark.gpu

N_WORDS = 300
N_DOCS = 5000
CUTS = [0, 1, 64, 1025, 1025, 3000, 5000]


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vocabs(ctx):
    """vocabularies by size, made once"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = make_vocab(ctx, n)
        return made[n]
    yield get
    for v in made.values():
        v.close()


def tile():
    from mapreduce_rust_amd import native
    return native.PMERGE_TILE


class Csr:
    """5000 documents over 300 words: word 0 in every document (its list spans more than two tiles), then 0 .. 13
    of the words 1 .. 298; word 299 has no postings.  On the host and on the device."""

    def __init__(self):
        rng = np.random.default_rng(31)
        rows = [np.concatenate([[0], np.sort(rng.choice(np.arange(1, N_WORDS - 1), rng.integers(0, 14), replace=False))])
                for _ in range(N_DOCS)]
        self.row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        self.terms = np.concatenate(rows).astype(np.uint32)
        self.counts = rng.integers(1, 9, len(self.terms)).astype(np.uint32)
        self.doc_len = (np.add.reduceat(self.counts, self.row_off[:-1]) + rng.integers(0, 5, N_DOCS)).astype(np.uint32)
        self.d_terms, self.d_counts = to_device_u32(self.terms), to_device_u32(self.counts)
        assert N_DOCS > 2 * tile()

    def index(self, ctx, v, a, e, base):
        """rows [a, e) through mrg_vocab_postings with doc_base = base + a, copied to the host: (post_off, docs, tf)"""
        import torch
        off = [int(x) for x in self.row_off[a:e + 1]]
        n = off[-1] - off[0]
        po = torch.empty((v.size()[0] + 1,), dtype=torch.int64, device="cuda:0")
        docs = torch.empty((max(n, 1),), dtype=torch.int32, device="cuda:0")
        tf = torch.empty_like(docs)
        torch.cuda.synchronize()
        assert ctx.postings(v, self.d_terms.data_ptr(), self.d_counts.data_ptr(), off, po.data_ptr(), docs.data_ptr(),
                            tf.data_ptr(), n, doc_base=base + a) == n
        torch.cuda.synchronize()
        return host_u64(po), host_u32(docs)[:n], host_u32(tf)[:n]

    def shards(self, ctx, v, cuts, base):
        return [DevShard(*self.index(ctx, v, a, e, base), pad_docs=i % 4, pad_tf=(i + 3) % 4)
                for i, (a, e) in enumerate(zip(cuts[:-1], cuts[1:]))]


@pytest.fixture(scope="module")
def csr():
    return Csr()


def same(got, want):
    for name, g, w in zip(("post_off", "docs", "tf"), got, want):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes(), name


# ---- 1. from CSRs: the merge of the shards is the index in one piece

@pytest.mark.parametrize("base", [0, 7])
def test_from_csrs(ctx, vocabs, csr, base):
    v = vocabs(N_WORDS)
    whole = csr.index(ctx, v, 0, N_DOCS, base)
    same(whole, expected_postings(csr.terms, csr.counts, csr.row_off, N_WORDS, base))
    assert int(whole[0][1]) == N_DOCS                        # word 0: every document
    for cuts in (CUTS, [0, N_DOCS]):
        shards = csr.shards(ctx, v, cuts, base)
        assert [s.n for s in shards].count(0) == (1 if len(cuts) > 2 else 0)
        same(check(ctx, v, shards), whole)
    info = ctx.postings_merge_info()
    assert info["entries"] == len(whole[1]) and info["words"] == N_WORDS and info["shards"] == 1
    assert info["tiles"] == -(-len(whole[1]) // tile()) and info["scratch_bytes"] > 4 * N_WORDS


# ---- 2. shards built directly

def sized_df(rng, n_words, n):
    """the frequencies of a shard of n entries: runs that end exactly at a tile end, a hot word, a word without
    postings"""
    t = tile()
    if n_words == 1:
        return [n]
    if n_words == 2:
        first = {t - 1: t // 2, t: t - 5, t + 1: t, 2 * t + 1: 2 * t}[n]
        return [first, n - first]
    df = np.zeros(n_words, dtype=np.int64)
    df[0] = n // 2
    df[1:n_words - 1] = rng.multinomial(n - n // 2, np.full(n_words - 2, 1.0 / (n_words - 2)))
    return df


@pytest.mark.parametrize("n_words", [1, 2, 257])
def test_sizes_around_the_tile(ctx, vocabs, n_words):
    v = vocabs(n_words)
    t = tile()
    rng = np.random.default_rng(n_words)
    span = 3 * t
    shards = []
    for i, n in enumerate((t - 1, t, t + 1, 2 * t + 1)):
        sh = synth_shard(rng, sized_df(rng, n_words, n), i * span, span)
        assert len(sh[1]) == n
        shards.append(DevShard(*sh, pad_docs=(i + 1) % 4, pad_tf=(i + 2) % 4))
    check(ctx, v, shards)
    # the diagnostics count the tiles and those inside one word as the host does
    info = ctx.postings_merge_info()
    tiles = single = 0
    for s in shards:
        off = s.post_off.astype(np.int64)
        for t0 in range(0, s.n, t):
            w0, w1 = (int(np.searchsorted(off, p, side="right")) - 1 for p in (t0, min(t0 + t, s.n) - 1))
            tiles, single = tiles + 1, single + (w0 == w1)
    assert (info["tiles"], info["single_word_tiles"], info["shards"]) == (tiles, single, 4)
    assert single == tiles if n_words == 1 else 0 < single < tiles
    # every shard alone, and in the other order of sizes (other output alignments)
    for s in shards:
        check(ctx, v, [s])
    rev = []
    for i, s in enumerate(reversed(shards)):                 # shard 3 - i, moved to the document range of shard i
        docs = (s.docs.astype(np.int64) + (2 * i - 3) * span).astype(np.uint32)
        rev.append(DevShard(s.post_off, docs, s.tf, pad_docs=i % 4, pad_tf=(i + 1) % 4))
    check(ctx, v, rev)


def test_empty_words_inside_a_tile(ctx, vocabs):
    n_words = 5300
    v = vocabs(n_words)
    rng = np.random.default_rng(5)
    df = np.zeros(n_words, dtype=np.int64)
    df[:100], df[5100:] = 3, 5                               # 5000 empty words between two groups, 1300 entries
    other = np.zeros(n_words, dtype=np.int64)
    other[:100], other[2000], other[5299] = 1, 7, 4
    assert df.sum() < tile() and (df[100:5100] == 0).all()
    shards = [DevShard(*synth_shard(rng, df, 0, 50), pad_docs=1), DevShard(*synth_shard(rng, other, 50, 50), pad_tf=3),
              DevShard(*synth_shard(rng, df, 100, 50), pad_docs=2, pad_tf=2)]
    check(ctx, v, shards)


@pytest.mark.parametrize("gap", [0, 1])
def test_words_in_a_tile_around_the_staging_limit(ctx, vocabs, gap):
    """the copy stages the offsets of a tile's words in LDS when the tile spans at most PMERGE_TILE words: the
    first tile here spans exactly that many words (gap 0), and one more, an empty one (gap 1)"""
    n_words, t = 5300, tile()
    v = vocabs(n_words)
    rng = np.random.default_rng(12 + gap)
    df = np.zeros(n_words, dtype=np.int64)
    df[:t - 1], df[t - 1 + gap], df[3000:3010] = 1, 1, 300
    assert df[:t + gap].sum() == t and (df[:t + gap] > 0).sum() == t
    shards = [DevShard(*synth_shard(rng, df, 0, 400), pad_docs=1, pad_tf=2), DevShard(*synth_shard(rng, df, 400, 400), pad_docs=3)]
    check(ctx, v, shards)


def test_64_shards_of_one_posting(ctx, vocabs):
    v = vocabs(257)
    rng = np.random.default_rng(6)
    df = np.zeros(257, dtype=np.int64)
    df[5] = 1
    shards = [DevShard(*synth_shard(rng, df, 10 * s, 10), pad_docs=s % 4, pad_tf=(s // 4) % 4) for s in range(64)]
    off, docs, tf = check(ctx, v, shards)
    assert int(off[5]) == 0 and int(off[6]) == 64 and (np.diff(docs.astype(np.int64)) > 0).all()


def test_all_postings_in_the_last_shard(ctx, vocabs):
    v = vocabs(257)
    rng = np.random.default_rng(7)
    none = synth_shard(rng, np.zeros(257, dtype=np.int64), 0, 1)
    big = synth_shard(rng, sized_df(rng, 257, 2 * tile() + 1), 100, 3 * tile())
    shards = [DevShard(*none, null=True), DevShard(*none), DevShard(*none, null=True), DevShard(*big, pad_docs=3, pad_tf=1)]
    same(check(ctx, v, shards), big)
    same(check(ctx, v, list(reversed(shards))), big)         # ... and in the first, the empty ones after it


# ---- 3. in two stages

def test_two_stages(ctx, vocabs, csr):
    v = vocabs(N_WORDS)
    shards = csr.shards(ctx, v, [0, 700, 2100, 2101, N_DOCS], 7)
    all_four = check(ctx, v, shards)
    same(all_four, expected_postings(csr.terms, csr.counts, csr.row_off, N_WORDS, 7))
    m01 = DevShard(*merge_dev(ctx, v, shards[:2]), pad_docs=2)
    m23 = DevShard(*merge_dev(ctx, v, shards[2:]), pad_tf=1)
    same(check(ctx, v, [m01, m23]), all_four)


# ---- 4. the merged index under mrg_vocab_search

class MergedIndex:
    """the outputs of one merge, left on the device, with what search_util.search_raw reads of an Index"""

    def __init__(self, ctx, v, shards, doc_len, doc_base):
        import torch
        self.n_entries = sum(s.n for s in shards)
        self.d_post_off = filled64(v.size()[0] + 1)
        self.d_docs, self.d_tf = filled(self.n_entries), filled(self.n_entries)
        self.d_doc_len = dev_u32(doc_len)
        self.n_docs, self.doc_base = len(doc_len), doc_base
        torch.cuda.synchronize()
        assert ctx.postings_merge(v, [s.arg() for s in shards], self.d_post_off.data_ptr(), self.d_docs.data_ptr(),
                                  self.d_tf.data_ptr(), self.n_entries) == self.n_entries
        self.p_docs, self.p_tf = self.d_docs.data_ptr(), self.d_tf.data_ptr()


def test_search_over_the_merged_index(ctx, vocabs, csr):
    from search_util import Index
    v = vocabs(N_WORDS)
    base = 7
    whole = Index(*expected_postings(csr.terms, csr.counts, csr.row_off, N_WORDS, base), csr.doc_len, base)
    merged = MergedIndex(ctx, v, csr.shards(ctx, v, CUTS, base), csr.doc_len, base)
    rng = np.random.default_rng(8)
    queries = [[], [0], [17], [0, 17, 40], [UNK], [N_WORDS - 1, UNK, 5], [int(x) for x in rng.integers(0, N_WORDS - 1, 40)],
               [3, 3, 0, 3]]
    for k in (1, 10, 1024):
        d1, s1, n1 = search_dev(ctx, v, whole, queries, k)
        d2, s2, n2 = search_dev(ctx, v, merged, queries, k)
        assert n1 == n2 and n1[1] == k and n1[0] == 0
        assert d1.tobytes() == d2.tobytes() and s1.tobytes() == s2.tobytes(), k


# ---- 5. refusals

ARGS = ("ctx", "v", "n_shards", "post_off", "docs", "tf", "entries", "d_post_off", "d_docs", "d_tf", "cap", "total")


def raw(args, **over):
    from mapreduce_rust_amd import native
    L = native.load()
    a = dict(args)
    a.update(over)
    rc = L.mrg_vocab_postings_merge(*[a[key] for key in ARGS])
    return rc, L.mrg_last_error().decode()


def table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def test_refused_before_any_device_work(ctx, vocabs, csr):
    import mapreduce_rust_amd as M
    import torch
    EINVAL = M.native.EINVAL
    v = vocabs(N_WORDS)
    shards = csr.shards(ctx, v, [0, 2000, 2000, N_DOCS], 0)
    s0, s1, s2 = shards
    e = sum(s.n for s in shards)
    want = check(ctx, v, shards)                             # (the pool has seen these sizes)
    before = ctx.pool_stats()
    po, docs, tf = filled64(N_WORDS + 1 + SLACK), filled(e + SLACK), filled(e + SLACK)
    torch.cuda.synchronize()
    t_po, t_docs, t_tf = (table([a[j] for a in (s.arg() for s in shards)]) for j in range(3))
    ent = (C.c_uint64 * 3)(*[s.n for s in shards])
    args = dict(ctx=ctx.h, v=v.h, n_shards=3, post_off=t_po, docs=t_docs, tf=t_tf, entries=ent, d_post_off=po.data_ptr(),
                d_docs=docs.data_ptr(), d_tf=tf.data_ptr(), cap=e, total=None)
    p = lambda s, j: s.arg()[j]
    cases = [
        (dict(ctx=None), "context"), (dict(v=None), "vocabulary"), (dict(post_off=None), "h_post_off"),
        (dict(entries=None), "h_entries"), (dict(d_post_off=None), "d_post_off"),
        (dict(post_off=table([p(s0, 0), None, p(s2, 0)])), "shard 1: null offsets"),
        (dict(n_shards=0), "n_shards = 0"), (dict(n_shards=65), "n_shards = 65"),
        (dict(d_docs=docs.data_ptr() + 2), "4-byte"), (dict(d_tf=tf.data_ptr() + 1), "4-byte"),
        (dict(d_post_off=po.data_ptr() + 4), "8-byte"),
        (dict(post_off=table([p(s0, 0), p(s1, 0), p(s2, 0) + 4])), "shard 2: the offsets must be 8-byte"),
        (dict(docs=table([p(s0, 1) + 2, p(s1, 1), p(s2, 1)])), "shard 0: the documents"),
        (dict(tf=table([p(s0, 2), p(s1, 2), p(s2, 2) + 3])), "shard 2: the documents"),
        (dict(entries=(C.c_uint64 * 3)(2**31, 0, 2**31), cap=2**33), "4294967295"),
        (dict(entries=(C.c_uint64 * 3)(2**32, 0, 0), cap=2**33), "4294967295"),
        (dict(cap=e - 1), "too small"), (dict(cap=0), "too small"),
        (dict(tf=None), "d_tf without h_tf"), (dict(d_docs=None), "d_tf without d_docs"),
        (dict(docs=None), "d_docs without h_docs"), (dict(docs=None, d_tf=None), "d_docs without h_docs"),
        (dict(docs=table([p(s0, 1), None, None])), "shard 2: null documents"),
        (dict(tf=table([None, None, p(s2, 2)])), "shard 0: null term frequencies"),
        (dict(d_docs=p(s2, 1)), "d_docs overlaps"),
        (dict(d_tf=p(s0, 2) + 4 * (s0.n - 1)), "d_tf overlaps"),
        (dict(d_docs=p(s2, 2) - 4 * (e - 1)), "d_docs overlaps"),
        (dict(d_post_off=p(s0, 0) + 8 * N_WORDS), "d_post_off overlaps"),
        (dict(d_docs=p(s2, 0), d_tf=None), "d_docs overlaps"),
    ]
    for over, what in cases:
        total = C.c_uint64(77)
        rc, msg = raw(args, total=C.byref(total), **over)
        assert rc == EINVAL and what in msg, (over, rc, msg)
        assert total.value == 77, over
        assert ctx.pool_stats()[0] == before[0], over
    torch.cuda.synchronize()
    assert (host_u64(po) == SENTINEL64).all() and (host_u32(docs) == SENTINEL).all() and (host_u32(tf) == SENTINEL).all(), \
        "an output was written by a refused call"
    # pointers of a shard without entries, and of arrays that are not merged, are not looked at
    total = C.c_uint64(77)
    assert raw(args, total=C.byref(total), docs=table([p(s0, 1), None, p(s2, 1)]), tf=table([p(s0, 2), None, p(s2, 2)]))[0] == 0
    assert total.value == e
    assert raw(args, docs=None, tf=None, d_docs=None, d_tf=None, cap=0)[0] == 0
    assert raw(args, tf=None, d_tf=None)[0] == 0
    torch.cuda.synchronize()
    same((host_u64(po)[:N_WORDS + 1], host_u32(docs)[:e], host_u32(tf)[:e]), want)
    assert ctx.pool_stats() == before


def test_refused_on_the_device(ctx, vocabs, csr):
    import mapreduce_rust_amd as M
    v = vocabs(N_WORDS)
    shards = csr.shards(ctx, v, [0, 2000, 2000, N_DOCS], 0)
    s0, s1, s2 = shards
    want = check(ctx, v, shards)
    before = ctx.pool_stats()

    def refused(call, what):
        with pytest.raises(M.MrgError) as ei:
            call()
        assert ei.value.code == M.native.EINVAL and what in str(ei.value), (what, str(ei.value))
        assert ctx.pool_stats()[0] == before[0], "scratch not returned after an error"

    def with_off(s, edit):
        po = s.post_off.copy()
        edit(po)
        out = DevShard(s.post_off, s.docs, s.tf)
        out.post_off = po
        import torch
        out.d_post_off = torch.from_numpy(po.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        return out

    def desc(*words):
        def edit(po):
            for w in words:
                po[w + 1] = po[w] - 1
        return edit

    def put(i, value):
        def edit(po):
            po[i] = value
        return edit

    # the offsets of a shard: descending (the smallest word, for it the smallest shard), the first, the last
    for mode in (0, 1, 2):
        refused(lambda: merge_raw(ctx, v, [s0, s1, with_off(s2, desc(7))], mode), "shard 2 word 7:")
        refused(lambda: merge_raw(ctx, v, [with_off(s0, desc(30)), s1, with_off(s2, desc(7, 12))], mode), "shard 2 word 7:")
        refused(lambda: merge_raw(ctx, v, [with_off(s0, desc(7)), s1, with_off(s2, desc(7))], mode), "shard 0 word 7:")
        refused(lambda: merge_raw(ctx, v, [s0, s1, with_off(s2, put(0, 1))], mode), "shard 2 word 0:")
        refused(lambda: merge_raw(ctx, v, [s0, with_off(s1, put(N_WORDS, 1)), s2], mode), "shard 1 word %d:" % (N_WORDS - 1))
    # ... the last offset against h_entries: one entry more than the offsets say
    import torch
    e = s0.n + s2.n
    po, docs, tf = filled64(N_WORDS + 1), filled(e + SLACK), filled(e + SLACK)
    torch.cuda.synchronize()
    a0, a2 = s0.arg(), s2.arg()
    refused(lambda: ctx.postings_merge(v, [a0, a2[:3] + (s2.n + 1,)], po.data_ptr(), docs.data_ptr(), tf.data_ptr(), e + 1),
            "shard 1 word %d:" % (N_WORDS - 1))
    refused(lambda: ctx.postings_merge(v, [a0[:3] + (s0.n - 1,), a2], po.data_ptr()), "shard 0 word %d:" % (N_WORDS - 1))

    # the seams: shards out of order (word 0 stands in every document), an equal document across a seam
    refused(lambda: merge_raw(ctx, v, [s2, s1, s0]), "shard 2 word 0:")
    refused(lambda: merge_raw(ctx, v, [s2, s0], 1), "shard 1 word 0:")
    assert merge_raw(ctx, v, [s2, s1, s0], 0)[0] == s0.n + s2.n      # the offsets alone know no order of the shards
    rng = np.random.default_rng(9)
    df = np.zeros(N_WORDS, dtype=np.int64)
    df[4], df[9] = 3, 2
    a = synth_shard(rng, df, 0, 50)
    b = synth_shard(rng, df, 50, 50)
    none = synth_shard(rng, np.zeros(N_WORDS, dtype=np.int64), 0, 1)
    check(ctx, v, [DevShard(*a), DevShard(*none), DevShard(*b)])
    b[1][3] = a[1][4]                                        # word 9: b's first document = a's last
    assert int(b[0][9]) == 3 and int(a[0][10]) == 5
    refused(lambda: merge_raw(ctx, v, [DevShard(*a), DevShard(*none, null=True), DevShard(*b)]), "shard 2 word 9:")
    b[1][3] += 1
    check(ctx, v, [DevShard(*a), DevShard(*none, null=True), DevShard(*b)])

    # the context and the vocabulary stay usable
    same(check(ctx, v, shards), want)
    assert ctx.pool_stats()[0] == before[0]


# ---- 6. empty cases, the pool, another device

def test_empty_cases_and_the_pool(ctx, vocabs):
    import mapreduce_rust_amd as M
    import torch
    v0 = vocabs(0)
    assert v0.size()[0] == 0
    zero = np.zeros(1, dtype=np.uint64)
    none = np.zeros(0, dtype=np.uint32)
    off, docs, tf = check(ctx, v0, [DevShard(zero, none, none), DevShard(zero, none, none, null=True)])
    assert off.tolist() == [0] and len(docs) == 0
    po = filled64(1)
    torch.cuda.synchronize()
    sh = DevShard(zero, none, none)
    with pytest.raises(M.MrgError) as ei:                    # entries of an empty vocabulary
        ctx.postings_merge(v0, [sh.arg()[:3] + (1,)], po.data_ptr())
    assert ei.value.code == M.native.EINVAL and "empty vocabulary" in str(ei.value)
    torch.cuda.synchronize()
    assert host_u64(po)[0] == SENTINEL64
    bad = DevShard(zero, none, none)
    bad.d_post_off.fill_(3)
    torch.cuda.synchronize()
    with pytest.raises(M.MrgError) as ei:
        ctx.postings_merge(v0, [bad.arg()], po.data_ptr())
    assert ei.value.code == M.native.EINVAL and "shard 0 word 0:" in str(ei.value)

    v = vocabs(257)
    rng = np.random.default_rng(10)
    empty = synth_shard(rng, np.zeros(257, dtype=np.int64), 0, 1)
    off, docs, tf = check(ctx, v, [DevShard(*empty, null=True), DevShard(*empty), DevShard(*empty, null=True)])
    assert (off == 0).all() and len(off) == 258 and len(docs) == 0

    shards = [DevShard(*synth_shard(rng, sized_df(rng, 257, tile() + 1), i * 3000, 3000), pad_docs=i) for i in range(3)]
    check(ctx, v, shards)                                    # (the pool has seen these sizes)
    before = ctx.pool_stats()
    check(ctx, v, shards)
    assert ctx.pool_stats() == before


def test_vocabulary_of_another_device(ctx, vocabs):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    rng = np.random.default_rng(11)
    sh = DevShard(*synth_shard(rng, np.full(257, 2, dtype=np.int64), 0, 10))
    with M.Context(1) as other:
        with make_vocab(other, 257) as v1:
            po = filled64(258)
            torch.cuda.synchronize()
            with pytest.raises(M.MrgError) as ei:
                ctx.postings_merge(v1, [sh.arg()], po.data_ptr())
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
            torch.cuda.synchronize()
            assert (host_u64(po) == SENTINEL64).all()
