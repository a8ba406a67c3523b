"""GPU tests of the map's error exits: a map that fails returns every scratch block to the context's pool
(mrg_pool_stats), drops the staged writes that pointed at them, and leaves the context usable.

Every forced failure is a host-side range check of a test knob (MRG_TEST_TAIL_CAP, MRG_TEST_OVF_CAP,
MRG_TEST_LONG_PER, MRG_TEST_WMAP_CAP = 2^32 - 1: no region of that size is asked for and no map kernel
of that attempt is launched) or invalid UTF-8 in the input, which the map reports.  The inputs are three
documents of the bundled corpus cut to 64 KiB; every expected output comes from the C oracle.

The last test injects the failure instead (mrg_test_pool_fail: the k-th allocation of the context's pool throws)
and sweeps k over every allocation of map, reduce, final and top-k, the .hip-side callers of the pool included
(mrg_format, the wide aggregation's fallback)."""
import collections
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = 10
CUT = 64 << 10
BAD_AT = 12345          # the invalid byte's offset in the second document
TOO_LARGE = 0xFFFFFFFF  # beyond every 32-bit capacity check (> 0xFFFFFFF0)
UNK = 0xFFFFFFFF
NAMES = ["a.txt", "b.txt", "c.txt"]


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def docs():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read()[:CUT] for m in range(3)]


@pytest.fixture(scope="module")
def bad_docs(docs):
    d = bytearray(docs[1])
    assert max(d[BAD_AT - 4:BAD_AT + 5]) < 0x80  # (inside ASCII text: the 0xFF is the first invalid byte)
    d[BAD_AT] = 0xFF
    return [docs[0], bytes(d), docs[2]]


@pytest.fixture(scope="module")
def expect(docs):
    """The oracle's outputs of the clean job, computed once."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    return {M.APP_WC: O.wc(docs, R, O.FAST), M.APP_INDEXER: O.indexer(docs, NAMES, R)}


@pytest.fixture
def env():
    """Set (or, with None, unset) environment knobs for one test; restored afterwards."""
    saved = {}

    def set_(**kv):
        for k, v in kv.items():
            saved.setdefault(k, os.environ.get(k))
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def failing_map(ctx, blobs, app, code):
    """job_begin, set_input and a map that must fail with `code`: returns (blocks out before, the error)."""
    import mapreduce_rust_amd as M
    import torch
    from gpu_util import to_device
    t, off = to_device(blobs)
    ctx.job_begin(app, R)
    before = ctx.pool_stats()[0]
    if app == M.APP_INDEXER:
        ctx.set_doc_names(NAMES)
    ctx.set_input(t.data_ptr(), off)
    with pytest.raises(M.MrgError) as ei:
        ctx.map()
    assert ei.value.code == code, str(ei.value)
    torch.cuda.synchronize()
    del t
    return before, ei.value


def clean_job(ctx, docs, expect, app):
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    assert run_wc(ctx, docs, R, app=app, names=NAMES if app == M.APP_INDEXER else None) == expect[app]


@pytest.mark.parametrize("knobs", [
    dict(MRG_TEST_TAIL_CAP=TOO_LARGE),                   # top of the map loop: the input tables held, writes staged
    dict(MRG_TEST_OVF_CAP=TOO_LARGE),                    # the per-bucket tables taken
    dict(MRG_TEST_LONG_PER=TOO_LARGE),                   # nearly all map buffers taken
    dict(MRG_WIDE_MAP=1, MRG_TEST_WMAP_CAP=TOO_LARGE),   # the wide map, its splitters held
], ids=["tail_cap", "ovf_cap", "long_per", "wmap_cap"])
def test_failed_capacity_check_returns_scratch(ctx, env, docs, expect, knobs):
    import mapreduce_rust_amd as M
    env(**knobs)
    before, _ = failing_map(ctx, docs, M.APP_WC, M.native.ENOMEM)
    ctx.job_begin(M.APP_WC, R)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    env(**{k: None for k in knobs})
    clean_job(ctx, docs, expect, M.APP_WC)


@pytest.mark.parametrize("wide_map,app", [(0, "wc"), (1, "wc"), (0, "indexer")])
def test_invalid_utf8_returns_scratch(ctx, env, docs, bad_docs, expect, wide_map, app):
    import mapreduce_rust_amd as M
    app = M.APP_WC if app == "wc" else M.APP_INDEXER
    env(MRG_WIDE_MAP=wide_map)
    before, err = failing_map(ctx, bad_docs, app, M.native.EUTF8)
    msg = str(err)
    assert "document 1 (id 1" in msg and msg.endswith(f"byte offset {BAD_AT}"), msg
    if app == M.APP_INDEXER:
        assert "document 1 (id 1, b.txt)" in msg, msg
    ctx.job_begin(app, R)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    env(MRG_WIDE_MAP=None)
    clean_job(ctx, docs, expect, app)


def test_vocabulary_calls_after_failed_map(ctx, env, docs, expect):
    """Between the failed map and the next job_begin, calls that touch no job state take blocks the failed
    map returned: the staged writes that pointed at them must not be issued any more."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    import torch
    from gpu_util import to_device
    env(MRG_TEST_TAIL_CAP=TOO_LARGE)
    before, _ = failing_map(ctx, docs, M.APP_WC, M.native.ENOMEM)
    env(MRG_TEST_TAIL_CAP=None)
    # a vocabulary from text and an encode, against the host tokenizer (as tests/test_gpu_encode.py)
    blobs = [docs[0][:4096], b"", docs[2][:3000]]
    toks = [O.tokens(b) for b in blobs]
    cnt = collections.Counter(x for t in toks[:1] for x in t)  # (the third document has unknown words)
    lines = sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))
    rank = {k: i for i, (k, _) in enumerate(lines)}
    text = b"".join(k + b" " + str(n).encode() + b"\n" for k, n in lines)
    exp_ids, exp_off = [], [0]
    for t in toks:
        exp_ids += [rank.get(x, UNK) for x in t]
        exp_off.append(len(exp_ids))
    with ctx.vocab_from_text(text) as v:
        t, off = to_device(blobs)
        tok = ctx.encode(v, t.data_ptr(), off)
        assert tok == exp_off
        out = torch.zeros((tok[-1] + 1,), dtype=torch.int32, device="cuda:0")
        assert ctx.encode(v, t.data_ptr(), off, out.data_ptr(), tok[-1]) == tok
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)[:tok[-1]]
        assert (got == np.array(exp_ids, dtype=np.uint32)).all()
        del t
    ctx.job_begin(M.APP_WC, R)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    clean_job(ctx, docs, expect, M.APP_WC)


# ---- every allocation of a job fails once (mrg_test_pool_fail): nothing stays out, the context stays usable

SWEEP_NAMES = NAMES + ["d.txt"]
STAGES = ("map", "reduce", "final", "topk")
MAX_K = 2000
INJECTED = "injected allocation failure"


@pytest.fixture(scope="module")
def sweep_docs(docs):
    """The module's documents and one with keys of more than 16 bytes (the long-key path, k_fix_runs)."""
    return docs + [b"x" * 40 + b" y " + b"z" * 23]


@pytest.fixture(scope="module")
def sweep_expect(sweep_docs):
    """Per app, the oracle's (mr-{r}.txt contents, final.txt, the 5 most frequent lines) of the clean job."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    exp = {}
    for app, outs in ((M.APP_WC, O.wc(sweep_docs, R, O.FAST)), (M.APP_INDEXER, O.indexer(sweep_docs, SWEEP_NAMES, R))):
        lines = sorted(l for o in outs for l in o.split(b"\n") if l)
        top = b""
        if app == M.APP_WC:
            def order(ln):
                key, c = ln.rsplit(b" ", 1)
                return (-int(c), key)
            top = b"".join(l + b"\n" for l in sorted(lines, key=order)[:5])
        exp[app] = (outs, b"".join(l + b"\n" for l in lines), top)
    return exp


@pytest.mark.parametrize("app,knobs", [
    ("wc", {}),
    ("indexer", {}),
    ("wc", dict(MRG_WIDE=1, MRG_TEST_LEAF_CAP=8)),   # the wide aggregation, its leaves overflowing into the fallback
], ids=["wc", "indexer", "wc_wide_fallback"])
def test_every_allocation_failure_returns_scratch(ctx, env, sweep_docs, sweep_expect, app, knobs):
    """For each stage of a job (map, reduce, final, topk) the k-th pool allocation of the stage fails, k = 1, 2, ...
    until the stage succeeds.  After every failure a clean job gives the oracle's outputs, and the blocks out after
    it are those of the first clean job: a block stranded by the failed call would show as baseline + n (d_out,
    d_final and d_top are context members: a failed regrow leaves one null and the clean job takes it again)."""
    import time
    import mapreduce_rust_amd as M
    import torch
    from gpu_util import to_device
    app = M.APP_WC if app == "wc" else M.APP_INDEXER
    stages = STAGES if app == M.APP_WC else STAGES[:3]
    outs, final, top = sweep_expect[app]
    env(**knobs)
    t, off = to_device(sweep_docs)
    call = {"map": ctx.map, "reduce": ctx.reduce, "final": ctx.final, "topk": lambda: ctx.topk(5)}

    def begin():
        ctx.job_begin(app, R)
        if app == M.APP_INDEXER:
            ctx.set_doc_names(SWEEP_NAMES)
        ctx.set_input(t.data_ptr(), off)

    def clean_job():
        begin()
        ctx.map()
        ctx.reduce()
        assert ctx.outputs() == outs
        assert ctx.final() == final
        if app == M.APP_WC:
            assert ctx.topk(5) == top

    clean_job()
    if knobs:
        assert ctx.stats()["overflow_keys"] > 0, "the fallback did not run"
    ctx.job_begin(app, R)
    baseline = ctx.pool_stats()[0]
    failures = {}
    for si, stage in enumerate(stages):
        t0 = time.perf_counter()
        for k in range(1, MAX_K + 2):
            assert k <= MAX_K, f"{stage}: still failing at k = {k}"
            begin()
            for earlier in stages[:si]:
                call[earlier]()
            ctx.pool_fail(k)
            try:
                call[stage]()
            except M.MrgError as e:
                ctx.pool_fail(0)
                assert e.code == M.native.ENOMEM and INJECTED in str(e), (stage, k, str(e))
            else:
                ctx.pool_fail(0)
                break
            clean_job()
            ctx.job_begin(app, R)
            assert ctx.pool_stats()[0] == baseline, f"{stage}: allocation {k} failed and blocks stayed out"
        failures[stage] = k - 1
        print(f"{stage}: {k - 1} injected failures, {time.perf_counter() - t0:.2f} s")
    assert all(failures[s] >= 1 for s in stages), failures
    torch.cuda.synchronize()
    del t
