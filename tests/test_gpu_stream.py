"""GPU tests of the batched map: mrg_job_map_add (the accumulator, k_acc.hip) and mrg_run_job with
MRG_FLAG_STREAM.

Every expectation comes from the C oracle (oracle_lib.wc / indexer / tokens / key_hash), the golden
digests, or a Python Counter over the oracle's tokens -- never from the library's one-shot result
alone.  After every map_add the batch's device buffer is overwritten with 0xFF bytes (invalid UTF-8
that no key can contain), so a late read of a released buffer shows."""
import collections
import gzip
import hashlib
import json
import os
import random
import struct
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
NO_COMPAT = 0x1


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


@pytest.fixture
def env():
    """Set environment knobs for one test; restored afterwards."""
    saved = {}

    def set_(**kv):
        for k, v in kv.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def counter_of(files):
    import oracle_lib as O
    cnt = collections.Counter()
    for f in files:
        cnt.update(O.tokens(f))
    return cnt


def expect_wc(files, R, flags):
    """mr-{r}.txt of the word count: the oracle's (flags 0, last group of every partition dropped), or
    every word of a Counter over the oracle's tokens, partitioned by the oracle's key hash."""
    import oracle_lib as O
    if not flags & NO_COMPAT:
        return O.wc(files, R, O.FAST)
    cnt = counter_of(files)
    parts = [[] for _ in range(R)]
    for k in cnt:
        parts[O.key_hash(k) % R].append(k)
    return [b"".join(k + b" " + str(cnt[k]).encode() + b"\n" for k in sorted(p)) for p in parts]


def lines_of(outs):
    return [l for o in outs for l in o.split(b"\n") if l]


def cat(lines):
    return b"".join(l + b"\n" for l in lines)


def ranked(lines):
    def order(ln):
        key, c = ln.rsplit(b" ", 1)
        return (-int(c), key)
    return sorted(lines, key=order)


def add_batch(ctx, blobs, doc_ids=None):
    """set_input + map_add of one batch, then the buffer is filled with 0xFF and released."""
    import torch
    from gpu_util import to_device
    t, off = to_device(blobs)
    ctx.set_input(t.data_ptr(), off, doc_ids)
    try:
        ctx.map_add()
    finally:
        t.fill_(0xFF)
        torch.cuda.synchronize()
        del t


def check_consumers(ctx, exp_outs, ks=(1, 1000, 10**9), topk=True):
    """reduce, final and topk against the expected mr-{r}.txt contents."""
    ctx.reduce()
    assert ctx.outputs() == exp_outs
    lines = lines_of(exp_outs)
    assert ctx.final() == cat(sorted(lines))
    if topk:
        top = ranked(lines)
        for k in ks:
            assert ctx.topk(k) == cat(top[:k]), k


# ---- 1. the bundled corpus, wc

BATCHINGS = {"6": [6], "2-2-2": [2, 2, 2], "1x6": [1] * 6, "1-5": [1, 5]}


@pytest.fixture(scope="module")
def corpus_expect(corpus):
    exp = {}
    for R in (1, 10, 64):
        for flags in (0, NO_COMPAT):
            exp[R, flags] = expect_wc(corpus, R, flags)
        for r in range(R):                              # the oracle agrees with the golden digests
            assert sha(exp[R, 0][r]) == GOLDEN["wc"][str(R)][f"mr-{r}.txt"]
        assert sha(cat(sorted(lines_of(exp[R, 0])))) == GOLDEN["wc"][str(R)]["final.txt"]
    return exp


@pytest.mark.parametrize("flags", [0, NO_COMPAT])
@pytest.mark.parametrize("R", [1, 10, 64])
@pytest.mark.parametrize("batching", list(BATCHINGS))
def test_corpus_batched(ctx, corpus, corpus_expect, batching, R, flags):
    import mapreduce_rust_amd as M
    ctx.job_begin(M.APP_WC, R, flags)
    m = 0
    for n in BATCHINGS[batching]:
        add_batch(ctx, corpus[m:m + n])
        m += n
    assert ctx.stats()["map_batches"] == len(BATCHINGS[batching])
    check_consumers(ctx, corpus_expect[R, flags])


# ---- 2. the indexer: three batches with global document ids

def test_indexer_batched(ctx, corpus):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    names = [f"data/gut-{m}.txt" for m in range(6)]
    exp = O.indexer(corpus, names, 10)
    assert [sha(o) for o in exp] == [GOLDEN["indexer"]["10"][f"mr-{r}.txt"] for r in range(10)]
    ctx.job_begin(M.APP_INDEXER, 10)
    ctx.set_doc_names(names)
    for ids in ([0, 1], [2, 3, 4], [5]):
        add_batch(ctx, [corpus[i] for i in ids], doc_ids=ids)
    check_consumers(ctx, exp, topk=False)


# ---- 3. long keys and ties across batches, with forced hash collisions

def long_tie_batches():
    from test_gpu_topk import tie_words
    rng = random.Random(18)
    stem = "sixteen_byte_stem"[:16]
    longs = [stem + "x" * n + s for n in (1, 2, 5, 14, 22) for s in ("", "a", "é")]   # 17 .. 40 bytes, equal first 16
    longs += ["another_stem_0123" + "y" * n for n in (0, 3, 23)]
    assert all(17 <= len(w.encode()) <= 40 for w in longs)
    short = tie_words()
    batches = []
    for b in range(3):
        toks = []
        for i, w in enumerate(longs):
            if i % 3 == b or i % 4 == 0:               # some in one batch only, some in all
                toks += [w] * rng.choice((1, 2, 3, 7))
        for i, w in enumerate(short):
            if i % 3 == b or i % 5 == 0:
                toks += [w] * rng.choice((1, 2, 3, 7))
        rng.shuffle(toks)
        batches.append(" ".join(toks).encode())
    return batches


@pytest.mark.parametrize("flags", [0, NO_COMPAT])
def test_long_keys_and_ties_across_batches(ctx, flags):
    import mapreduce_rust_amd as M
    batches = long_tie_batches()
    R = 5
    exp = expect_wc(batches, R, flags)
    n = len(lines_of(exp))
    outs = []
    for bits in (0, 1, 4):
        ctx.job_begin(M.APP_WC, R, flags | M.debug_hash_bits(bits))
        for b in batches:
            add_batch(ctx, [b])
        check_consumers(ctx, exp, ks=(1, 7, n - 1, n, n + 3))
        assert ctx.stats()["long_tokens"] > 0
        outs.append(ctx.outputs())
    assert outs[0] == outs[1] == outs[2]


# ---- 4. growth of the table

def test_growth(ctx, env):
    import mapreduce_rust_amd as M
    env(MRG_TEST_ACC_CAP=1024)
    rng = random.Random(4)
    batches, seen = [], []
    for b in range(5):
        new = ["g%d_%05d" % (b, i) for i in range(3000)]   # 3000 new distinct words per batch
        toks = new + [rng.choice(seen) for _ in range(2000)] if seen else list(new)
        rng.shuffle(toks)
        seen += new
        batches.append(" ".join(toks).encode())
    for flags in (0, NO_COMPAT):
        ctx.job_begin(M.APP_WC, 7, flags)
        for i, b in enumerate(batches):
            add_batch(ctx, [b])
            assert ctx.stats()["distinct_keys"] == 3000 * (i + 1)   # 1024 -> 8192 -> 16384 -> 32768 slots
        info = ctx.acc_info()
        assert info["rehashes"] >= 2 and info["short_keys"] == 15000 and info["slots"] >= 2 * 15000
        check_consumers(ctx, expect_wc(batches, 7, flags))


# ---- 5. wide (sort-based) batches: every key of batch 0 repeats in batch 2

def test_wide_batches(ctx, env):
    import torch
    import mapreduce_rust_amd as M
    import oracle_lib as O
    env(MRG_WIDE=1)
    n = 8 << 20
    ctx.job_begin(M.APP_WC, 16)
    host = []
    for fi in (0, 1, 0):
        t = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
        ctx.gen_unique(t.data_ptr(), n, 0xC5, fi)
        torch.cuda.synchronize()
        host.append(t[:n].cpu().numpy())
        ctx.set_input(t.data_ptr(), [0, n])
        ctx.map_add()
        assert ctx.stats()["agg_path"] == 2
        t.fill_(0xFF)
        torch.cuda.synchronize()
        del t
    exp = O.wc_mt(host, 16)
    ctx.reduce()
    got = ctx.outputs()
    assert [sha(g) for g in got] == [sha(e) for e in exp]
    assert sha(ctx.final()) == sha(cat(sorted(lines_of(exp))))


# ---- 6. 64-bit counts: an imported count just below 2^32, then a batch

def test_counts_cross_32_bits(ctx):
    import torch
    import mapreduce_rust_amd as M
    rec = struct.pack("<QQII", int.from_bytes(b"a".ljust(8, b"\0"), "big"), 0, 0xFFFFFFF0, 1)
    R = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda:0")
    H = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    ctx.job_begin(M.APP_WC, 3, NO_COMPAT)
    ctx.import_(R.data_ptr(), 1, H.data_ptr(), 0)
    add_batch(ctx, [b"a " * 32 + b"b"])
    assert ctx.stats()["map_batches"] == 1
    ctx.reduce()
    lines = lines_of(ctx.outputs())
    assert b"a 4294967312" in lines and b"b 1" in lines and len(lines) == 2
    assert ctx.topk(1) == b"a 4294967312\n"


# ---- 7. a failing batch adds nothing

def test_failing_batch_is_all_or_nothing(ctx, corpus):
    import mapreduce_rust_amd as M
    A, Cc = corpus[2], corpus[3]
    X = bytearray(b"word " * 40000)
    X[123457] = 0xFF                                   # invalid UTF-8 at a known offset
    exp = expect_wc([A, Cc], 10, 0)
    ctx.job_begin(M.APP_WC, 10)
    add_batch(ctx, [A])
    with pytest.raises(M.MrgError) as ei:
        add_batch(ctx, [bytes(X)])
    assert ei.value.code == M.native.EUTF8 and "byte offset 123457" in str(ei.value)
    st = ctx.stats()
    assert st["map_batches"] == 1 and st["input_bytes"] == len(A)
    add_batch(ctx, [Cc])
    st = ctx.stats()
    assert st["map_batches"] == 2 and st["input_bytes"] == len(A) + len(Cc)
    check_consumers(ctx, exp)
    # a failure right after a consumer call: the keys are still those of A + C
    with pytest.raises(M.MrgError):
        add_batch(ctx, [bytes(X)])
    check_consumers(ctx, exp)


# ---- 8. consumers between batches; mrg_job_map discards the accumulator

def test_interleaving(ctx, corpus):
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    A, B, Cc = [corpus[0]], [corpus[1], corpus[2]], [corpus[3]]
    ctx.job_begin(M.APP_WC, 10)
    add_batch(ctx, A)
    check_consumers(ctx, expect_wc(A, 10, 0))
    add_batch(ctx, B)
    check_consumers(ctx, expect_wc(A + B, 10, 0))
    t, off = to_device(Cc)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()                                           # replaces the keys
    assert ctx.stats()["map_batches"] == 0
    check_consumers(ctx, expect_wc(Cc, 10, 0))
    add_batch(ctx, A)                                   # and map_add then adds to mrg_job_map's keys
    check_consumers(ctx, expect_wc(Cc + A, 10, 0))
    del t


# ---- 9. export after batches, imported into a second job

def test_export_after_batches(ctx, corpus):
    import torch
    import mapreduce_rust_amd as M
    X = M.native.XREC_BYTES
    long_doc = (" ".join(["a_key_of_twenty_bytes", "another_key_longer_than_16"] * 3)).encode()
    docs = corpus[:3] + [long_doc]
    ctx.job_begin(M.APP_WC, 10)
    add_batch(ctx, docs[:1])
    add_batch(ctx, docs[1:3])
    add_batch(ctx, docs[3:])
    rec, heap = ctx.export_sizes(3)
    drec = torch.empty(max(sum(rec), 1) * X, dtype=torch.uint8, device="cuda:0")
    dheap = torch.empty(max(sum(heap), 1) + 16, dtype=torch.uint8, device="cuda:0")
    ctx.export(drec.data_ptr(), dheap.data_ptr())
    assert sum(heap) > 0 and all(rec)
    ctx.job_begin(M.APP_WC, 10)
    ctx.import_(drec.data_ptr(), sum(rec), dheap.data_ptr(), sum(heap), rec, heap)
    check_consumers(ctx, expect_wc(docs, 10, 0))


# ---- 10. stats and pool

def test_stats_and_pool(ctx, corpus):
    import oracle_lib as O
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    docs = corpus[:3]
    run_wc(ctx, docs, 10)
    ctx.final()
    ctx.topk(5)
    ctx.job_begin(M.APP_WC, 10)
    plain = ctx.pool_stats()[0]
    toks, nbytes = [], 0
    for d in docs:
        add_batch(ctx, [d])
        toks += O.tokens(d)
        nbytes += len(d)
        st = ctx.stats()
        assert (st["tokens"], st["input_bytes"], st["distinct_keys"]) == (len(toks), nbytes, len(set(toks)))
    add_batch(ctx, [b" \t\n  \n" * 100])                 # a whitespace-only batch adds nothing
    st = ctx.stats()
    assert (st["tokens"], st["distinct_keys"], st["map_batches"]) == (len(toks), len(set(toks)), 4)
    assert st["input_bytes"] == nbytes + 600
    check_consumers(ctx, expect_wc(docs, 10, 0))
    ctx.job_begin(M.APP_WC, 10)
    assert ctx.pool_stats()[0] == plain
    add_batch(ctx, [b"  \n"])                            # an empty job: no keys, empty outputs
    ctx.reduce()
    assert ctx.outputs() == [b""] * 10 and ctx.final() == b""
    ctx.job_begin(M.APP_WC, 10)
    assert ctx.pool_stats()[0] == plain


def test_map_add_errors(ctx):
    import mapreduce_rust_amd as M
    ctx.job_begin(M.APP_WC, 4)
    with pytest.raises(M.MrgError) as ei:               # no input set
        ctx.map_add()
    assert ei.value.code == M.native.EINVAL
    add_batch(ctx, [b"one two two"])
    with pytest.raises(M.MrgError) as ei:               # every batch needs its own set_input
        ctx.map_add()
    assert ei.value.code == M.native.EINVAL
    ctx.reduce()
    assert lines_of(ctx.outputs()) == lines_of(expect_wc([b"one two two"], 4, 0))


# ---- 11. the whole job: mrg_run_job with MRG_FLAG_STREAM, and mrgpu --stream

def _data_dir(tmp_path, corpus):
    d = tmp_path / "data"
    d.mkdir(exist_ok=True)
    files = []
    for m in range(6):
        (d / f"gut-{m}.txt").write_bytes(corpus[m])
        files.append(f"data/gut-{m}.txt")
    return files


def _outputs(tmp_path, R, extra=("final.txt", "top.txt")):
    names = [f"mr-{r}.txt" for r in range(R)] + list(extra)
    got = {n: (tmp_path / n).read_bytes() for n in names}
    for n in names:
        (tmp_path / n).unlink()
    return got


def _cli(tmp_path, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([os.path.join(ROOT, "mapreduce_rust_amd", "lib", "mrgpu")] + [str(a) for a in args],
                          cwd=tmp_path, env=e, capture_output=True, text=True, timeout=120)


def test_run_job_streamed(tmp_path, corpus, env):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    N = M.native
    files = _data_dir(tmp_path, corpus)
    sizes = [len(c) for c in corpus]
    flags = N.FLAG_FINAL_TXT | N.flag_top(25)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        N.run_job(files, 10, M.APP_WC, ".", flags)
        assert N.run_stream_stats() == (0, sum(sizes))
        plain = _outputs(tmp_path, 10)
        for r in range(10):
            assert sha(plain[f"mr-{r}.txt"]) == GOLDEN["wc"]["10"][f"mr-{r}.txt"]
        assert sha(plain["final.txt"]) == GOLDEN["wc"]["10"]["final.txt"]
        assert plain["top.txt"] == cat(ranked(lines_of([plain["final.txt"]]))[:25])
        for bb, comm in ((1, 0), (1 << 20, 0), (1 << 20, 1)):
            env(MRG_STREAM_BATCH_BYTES=bb, MRG_TEST_FORCE_COMM=comm)
            st = N.run_job(files, 10, M.APP_WC, ".", flags | N.FLAG_STREAM)
            assert _outputs(tmp_path, 10) == plain, (bb, comm)
            first = N.stream_plan(sizes, bb)
            assert first == ([0, 1, 2, 3, 4, 5] if bb == 1 else [0, 1, 4, 5])
            largest = max(sum(sizes[a:b]) for a, b in zip(first, first[1:] + [6]))
            batches, peak = N.run_stream_stats()
            assert batches == len(first) and 0 < peak <= 2 * largest + 128
            assert st["input_bytes"] == sum(sizes)
        env(MRG_TEST_FORCE_COMM=0)
        # the indexer
        exp = O.indexer(corpus, files, 10)
        N.run_job(files, 10, M.APP_INDEXER, ".", N.FLAG_STREAM)
        got = _outputs(tmp_path, 10, extra=())
        assert [got[f"mr-{r}.txt"] for r in range(10)] == exp
    finally:
        os.chdir(cwd)


def test_cli_stream_and_failures(tmp_path, corpus):
    """mrgpu --stream in a fresh child process, under the test's own timeout: golden output; a file
    removed from the last batch is MRG_EIO, invalid bytes in the fourth file are MRG_EUTF8 naming the
    file -- status codes, never a hang."""
    _data_dir(tmp_path, corpus)
    e = {"MRG_STREAM_BATCH_BYTES": str(1 << 20)}
    p = _cli(tmp_path, 6, 10, "--stream", "--final", "--times", env=e)
    assert p.returncode == 0, p.stderr
    for r in range(10):
        assert sha((tmp_path / f"mr-{r}.txt").read_bytes()) == GOLDEN["wc"]["10"][f"mr-{r}.txt"], r
    assert sha((tmp_path / "final.txt").read_bytes()) == GOLDEN["wc"]["10"]["final.txt"]
    times = json.loads(p.stderr.strip().splitlines()[-1])
    assert times["stream"] == 1 and times["batches"] == 4 and times["input_bytes"] == sum(len(c) for c in corpus)
    bad = bytearray(corpus[3])
    bad[1000] = 0xFF
    (tmp_path / "data" / "gut-3.txt").write_bytes(bytes(bad))
    p = _cli(tmp_path, 6, 10, "--stream", env=e)
    assert p.returncode == 1 and "error -2" in p.stderr and "data/gut-3.txt" in p.stderr, p.stderr
    (tmp_path / "data" / "gut-3.txt").write_bytes(corpus[3])
    (tmp_path / "data" / "gut-5.txt").unlink()
    p = _cli(tmp_path, 6, 10, "--stream", env=e)
    assert p.returncode == 1 and "error -5" in p.stderr and "data/gut-5.txt" in p.stderr, p.stderr
