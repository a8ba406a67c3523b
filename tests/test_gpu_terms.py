"""GPU tests of mrg_vocab_term_counts (k_terms.hip): per-document term counts of id sequences, in CSR form.

No expectation comes from the library: expected rows are built in numpy from the id arrays
(tests/terms_util.py expected_rows, itself checked against collections.Counter by tests/test_terms_cpu.py);
for the corpus the ids come from the C oracle's tokens ranked as tests/vocab_util.py ranks them.  Every
call goes sizes-only first, then full with cap exact into sentinel-filled buffers with slack
(terms_util.term_counts_dev).  A document of at most WAVE_MAX ids is sorted by one wave, one of at most
WG_MAX ids by one workgroup, a longer one by the radix sort; the sweeps below are sized by those two
numbers.  Every bad input here is one the contract answers with a status code."""
import gzip
import os
import random

import numpy as np
import pytest

from terms_util import SENTINEL, UNK, check, check_dev, ids_to_device, make_vocab, term_counts_dev

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def consts():
    from mapreduce_rust_amd import native
    return native.TERMS_WAVE_MAX, native.TERMS_WG_MAX


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vocab(ctx):
    """WG_MAX + 2 words: a document of WG_MAX + 1 ids can be all distinct"""
    v = make_vocab(ctx, consts()[1] + 2)
    yield v
    v.close()


def zipf_ids(rng, n, n_words):
    return np.minimum(rng.zipf(1.3, n) - 1, n_words - 1).astype(np.uint32)


def offsets(lengths, first=0):
    off = [first]
    for n in lengths:
        off.append(off[-1] + n)
    return off


# ---- 1. a length sweep across every path boundary, for every id pattern

def sweep_lengths():
    WAVE, WG = consts()
    lens = [0, 1, 2, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1]
    random.Random(7).shuffle(lens)
    out = []
    for n in lens:                                           # empty documents between them
        out += [n, 0]
    paths = (sum(1 for n in lens if 0 < n <= WAVE), sum(1 for n in lens if WAVE < n <= WG), sum(1 for n in lens if n > WG))
    assert paths == (7, 3, 1)
    return out, paths


PATTERNS = ["equal", "distinct", "descending", "all_unk", "unk_alternating", "first_and_last", "zipf"]


def pattern_ids(pattern, T, n_words, rng):
    if pattern == "equal":
        return np.full(T, 5, dtype=np.uint32)
    if pattern == "distinct":
        return rng.permutation(n_words)[:T].astype(np.uint32)
    if pattern == "descending":
        return ((T - 1 - np.arange(T)) // 2).astype(np.uint32)
    if pattern == "all_unk":
        return np.full(T, UNK, dtype=np.uint32)
    if pattern == "unk_alternating":
        a = zipf_ids(rng, T, n_words)
        a[::2] = UNK
        return a
    if pattern == "first_and_last":
        return np.where(rng.random(T) < 0.5, 0, n_words - 1).astype(np.uint32)
    return zipf_ids(rng, T, n_words)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_length_sweep(ctx, vocab, pattern):
    WAVE, WG = consts()
    n_words = WG + 2
    lens, paths = sweep_lengths()
    rng = np.random.default_rng(PATTERNS.index(pattern))
    ids = np.concatenate([pattern_ids(pattern, T, n_words, rng) for T in lens])
    tok = offsets(lens)
    off, terms, counts, unk = check(ctx, vocab, ids, tok)
    info = ctx.terms_info()
    assert (info["wave_docs"], info["wg_docs"], info["large_docs"]) == paths
    assert info["ids"] == len(ids) and info["entries"] == off[-1] and info["unk"] == sum(unk)
    assert info["slices"] == 1 and info["scratch_bytes"] > 0
    if pattern == "distinct":
        assert off[-1] == len(ids)                           # cap = the number of ids is reached
    if pattern == "all_unk":
        assert off[-1] == 0 and sum(unk) == len(ids)


# ---- 2. a sub-range of a buffer: a first offset that is not 0, poison around the range

@pytest.mark.parametrize("first", [1, 2, 3, 5])
def test_sub_range(ctx, vocab, first):
    WAVE, WG = consts()
    n_words = WG + 2
    lens = [3, 0, WAVE, 70, WAVE + 5, WG + 9, 1]
    rng = np.random.default_rng(first)
    body = zipf_ids(rng, sum(lens), n_words)
    body[::7] = UNK
    poison = np.full(8, n_words, dtype=np.uint32)            # not in the vocabulary: reading one is an error
    buf = np.concatenate([poison[:first], body, poison])
    tok = offsets(lens, first)
    t = ids_to_device(buf)
    check_dev(ctx, vocab, t.data_ptr(), buf, tok)
    # the same through a pointer that is not 16-byte aligned, offsets from 0
    check_dev(ctx, vocab, t.data_ptr() + 4 * first, body, offsets(lens))


# ---- 3. many tiny documents

def test_many_tiny_documents(ctx, vocab):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 6, 100_000).tolist()
    ids = zipf_ids(rng, sum(lens), 50)
    ids[rng.random(len(ids)) < 0.1] = UNK
    check(ctx, vocab, ids, offsets(lens))
    info = ctx.terms_info()
    assert info["wave_docs"] == sum(1 for n in lens if n) and info["wg_docs"] == 0 and info["large_docs"] == 0


# ---- 4. the large path in slices

def test_large_path_slices(ctx, vocab, monkeypatch):
    WAVE, WG = consts()
    n_words = WG + 2
    lens = [WG + 1, WG + 900, WG + 1900, 0, WG + 2900, 2 * WG]
    rng = np.random.default_rng(4)
    ids = zipf_ids(rng, sum(lens), n_words)
    ids[rng.random(len(ids)) < 0.05] = UNK
    tok = offsets(lens)
    whole = check(ctx, vocab, ids, tok)
    assert ctx.terms_info()["slices"] == 1 and ctx.terms_info()["large_docs"] == 5
    monkeypatch.setenv("MRG_TEST_TERMS_SLICE_IDS", str(lens[0] + lens[1] + 10))   # the first two together, then one each
    sliced = check(ctx, vocab, ids, tok)
    assert ctx.terms_info()["slices"] == 4
    monkeypatch.setenv("MRG_TEST_TERMS_SLICE_IDS", "1")      # below every document: each one alone
    single = check(ctx, vocab, ids, tok)
    assert ctx.terms_info()["slices"] == 5
    for other in (sliced, single):
        assert other[0] == whole[0] and other[3] == whole[3]
        assert (other[1] == whole[1]).all() and (other[2] == whole[2]).all()
    monkeypatch.delenv("MRG_TEST_TERMS_SLICE_IDS")
    check(ctx, vocab, ids, tok)
    assert ctx.terms_info()["slices"] == 1


# ---- 5. skew: a count above 65535

def test_skew(ctx, vocab):
    n = 200_000
    rng = np.random.default_rng(5)
    ids = zipf_ids(rng, n, consts()[1] + 2)
    r = rng.random(n)
    ids[r < 0.90] = 1234
    ids[r >= 0.95] = UNK
    off, terms, counts, unk = check(ctx, vocab, ids, [0, n])
    assert counts.max() > 65535 and unk[0] > 5000


# ---- 6. the corpus: whole files, and the same ids re-cut into documents of several sizes

@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


def test_corpus(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import to_device
    from vocab_util import count_lines, expected, rank_of, ranked
    WAVE, WG = consts()
    doc_tokens = [O.tokens(d) for d in corpus]
    lines = ranked(count_lines(doc_tokens))[:5000]
    exp_ids, exp_tok = expected(doc_tokens, rank_of(lines))   # from the oracle: not encode's output
    assert (exp_ids == UNK).any() and min(len(t) for t in doc_tokens) > WG
    t, off = to_device(corpus)
    ctx.job_begin(M.APP_WC, 1, M.FLAG_NO_COMPAT_DROP_LAST)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    with ctx.vocab(max_words=5000) as v:
        import torch
        tok = ctx.encode(v, t.data_ptr(), off)
        assert tok == exp_tok
        d_ids = torch.empty((tok[-1],), dtype=torch.int32, device="cuda:0")
        ctx.encode(v, t.data_ptr(), off, d_ids.data_ptr(), tok[-1])
        check_dev(ctx, v, d_ids.data_ptr(), exp_ids, tok)                # whole files: the large path
        assert ctx.terms_info()["large_docs"] == 6
        n = tok[-1]
        for size in (50, 700, WG // 2):                       # only tok_off changes
            rng = random.Random(size)
            cut = [0]
            while cut[-1] < n:
                cut.append(min(n, cut[-1] + rng.randrange(size // 2, size * 3 // 2)))
            check_dev(ctx, v, d_ids.data_ptr(), exp_ids, cut)
            info = ctx.terms_info()
            assert info["large_docs"] == 0 and info["wave_docs"] + info["wg_docs"] == len(cut) - 1
    del t


# ---- 7. errors

def test_errors(ctx, vocab):
    import mapreduce_rust_amd as M
    import torch
    WAVE, WG = consts()
    n_words = WG + 2
    rng = np.random.default_rng(7)
    for lens in ([100, 0, 1000, WG + 500], [WG + 500, 100, 1000]):
        tok = offsets(lens)
        base = zipf_ids(rng, tok[-1], n_words)
        base[::11] = UNK
        good = check(ctx, vocab, base, tok)
        for d, T in enumerate(lens):
            for at in ({tok[d], tok[d] + T // 2, tok[d + 1] - 1} if T else ()):
                for bad in (n_words, 0xFFFFFFFE):
                    ids = base.copy()
                    ids[at] = bad
                    t = ids_to_device(ids)
                    with pytest.raises(M.MrgError) as ei:
                        ctx.term_counts(vocab, t.data_ptr(), tok)
                    assert ei.value.code == M.native.EINVAL and "index %d " % at in str(ei.value), (at, str(ei.value))
        # two bad ids in documents of different paths: the smaller index is named
        docs = [d for d, T in enumerate(lens) if T]
        for a in docs:
            for b in docs:
                if a < b:
                    ids = base.copy()
                    ids[tok[a + 1] - 1] = n_words
                    ids[tok[b] + 1] = 0xFFFFFFFE
                    t = ids_to_device(ids)
                    with pytest.raises(M.MrgError) as ei:
                        ctx.term_counts(vocab, t.data_ptr(), tok)
                    assert "index %d " % (tok[a + 1] - 1) in str(ei.value), (a, b, str(ei.value))
        # cap one short: both destinations stay as they were
        t = ids_to_device(base)
        total = good[0][-1]
        terms = torch.full((total + 8,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
        counts = terms.clone()
        with pytest.raises(M.MrgError) as ei:
            ctx.term_counts(vocab, t.data_ptr(), tok, terms.data_ptr(), counts.data_ptr(), total - 1)
        assert ei.value.code == M.native.EINVAL and "too small" in str(ei.value)
        torch.cuda.synchronize()
        assert (terms.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to d_terms"
        assert (counts.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote to d_counts"
        # one destination of the two
        for tp, cp in ((terms.data_ptr(), None), (None, counts.data_ptr())):
            with pytest.raises(M.MrgError) as ei:
                ctx.term_counts(vocab, t.data_ptr(), tok, tp, cp, total)
            assert ei.value.code == M.native.EINVAL
        torch.cuda.synchronize()
        assert (terms.cpu().numpy().view(np.uint32) == SENTINEL).all()
        # decreasing offsets
        with pytest.raises(M.MrgError) as ei:
            ctx.term_counts(vocab, t.data_ptr(), [0, 100, 99, tok[-1]])
        assert ei.value.code == M.native.EINVAL and "non-decreasing" in str(ei.value)
        # the context and the vocabulary still give the right answer
        again = check(ctx, vocab, base, tok)
        assert again[0] == good[0] and (again[1] == good[1]).all() and (again[2] == good[2]).all()


def test_empty_vocabulary_and_empty_input(ctx, vocab):
    import mapreduce_rust_amd as M
    WAVE, WG = consts()
    with ctx.vocab_from_text(b"") as v0:
        lens = [1, 0, 600, WG + 3]
        ids = np.full(sum(lens), UNK, dtype=np.uint32)
        off, terms, counts, unk = check(ctx, v0, ids, offsets(lens))
        assert off == [0] * 5 and unk == lens
        for at in (0, 300, 700):                              # id 0 is not in an empty vocabulary
            bad = ids.copy()
            bad[at] = 0
            with pytest.raises(M.MrgError) as ei:
                ctx.term_counts(v0, ids_to_device(bad).data_ptr(), offsets(lens))
            assert ei.value.code == M.native.EINVAL and "index %d " % at in str(ei.value)
    empty = np.zeros(0, dtype=np.uint32)
    assert term_counts_dev(ctx, vocab, ids_to_device(empty).data_ptr(), [0])[0] == [0]            # n_docs = 0
    for tok in ([0, 0], [0, 0, 0, 0], [5, 5, 5]):
        off, terms, counts, unk = term_counts_dev(ctx, vocab, ids_to_device(empty).data_ptr(), tok)
        assert off == [0] * len(tok) and unk == [0] * (len(tok) - 1) and len(terms) == 0
    assert ctx.term_counts(vocab, None, [0]) == ([0], []) and ctx.term_counts(vocab, None, [5, 5, 5]) == ([0, 0, 0], [0, 0])


# ---- 8. no side effects: the pool, and a streamed job around the call

def test_pool_is_unchanged(ctx, vocab):
    import mapreduce_rust_amd as M
    WAVE, WG = consts()
    lens = [10, 500, WG + 100, 0, 7]
    rng = np.random.default_rng(8)
    ids = zipf_ids(rng, sum(lens), WG + 2)
    tok = offsets(lens)
    check(ctx, vocab, ids, tok)                              # (the pool has seen these sizes)
    before = ctx.pool_stats()
    check(ctx, vocab, ids, tok)
    assert ctx.pool_stats() == before
    for at in (3, 200, tok[2] + 50):
        bad = ids.copy()
        bad[at] = WG + 2
        t = ids_to_device(bad)
        with pytest.raises(M.MrgError):
            ctx.term_counts(vocab, t.data_ptr(), tok)
        assert ctx.pool_stats() == before, "scratch not returned after an error"
        with pytest.raises(M.MrgError):                      # the full call fails in its count pass too
            ctx.term_counts(vocab, t.data_ptr(), tok, t.data_ptr(), t.data_ptr(), 0)
        assert ctx.pool_stats() == before


def test_streamed_job_does_not_notice(ctx, vocab, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import to_device
    WAVE, WG = consts()
    docs = [d[:d.rindex(b" ", 0, 100_000)] for d in corpus[:6]]
    lens = [10, 500, WG + 100]
    ids = zipf_ids(np.random.default_rng(9), sum(lens), WG + 2)
    tok = offsets(lens)
    ctx.job_begin(M.APP_WC, 10, 0)
    keep = []
    for first in (0, 2):
        tb, off = to_device(docs[first:first + 2])
        keep.append(tb)
        ctx.set_input(tb.data_ptr(), off, list(range(first, first + 2)))
        ctx.map_add()
    top = ctx.topk(10)
    check(ctx, vocab, ids, tok)
    assert ctx.topk(10) == top
    tb, off = to_device(docs[4:6])
    keep.append(tb)
    ctx.set_input(tb.data_ptr(), off, [4, 5])
    ctx.map_add()                                            # a third batch still folds in
    check(ctx, vocab, ids, tok)
    ctx.reduce()
    assert ctx.outputs() == O.wc(docs, 10, O.FAST)
    del keep


# ---- 9. a vocabulary of another device

def test_vocabulary_of_another_device(ctx):
    import mapreduce_rust_amd as M
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    with M.Context(1) as other:
        with make_vocab(other, 10) as v1:
            t = ids_to_device(np.arange(5, dtype=np.uint32))
            with pytest.raises(M.MrgError) as ei:
                ctx.term_counts(v1, t.data_ptr(), [0, 5])
            assert ei.value.code == M.native.EINVAL and "device" in str(ei.value)
