"""GPU tests of the map's error exits: a map that fails returns every scratch block to the context's pool
(mrg_pool_stats), drops the staged writes that pointed at them, and leaves the context usable.

Every forced failure is a host-side range check of a test knob (MRG_TEST_TAIL_CAP, MRG_TEST_OVF_CAP,
MRG_TEST_LONG_PER, MRG_TEST_WMAP_CAP = 2^32 - 1: no region of that size is asked for and no map kernel
of that attempt is launched) or invalid UTF-8 in the input, which the map reports.  The inputs are three
documents of the bundled corpus cut to 64 KiB; every expected output comes from the C oracle."""
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
