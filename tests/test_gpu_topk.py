"""GPU tests of mrg_job_topk (k_topk.hip): the K most frequent words, selected on the device.

The expectation is always a Python sort, by (count descending, key bytes ascending), of lines that
come from the C oracle (flags 0: its mr-{r}.txt, so with every partition's last key dropped) or from a
Counter over the oracle's tokens (MRG_FLAG_NO_COMPAT_DROP_LAST) -- never from the library."""
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


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus():
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(6)]


def ranked(lines):
    """Lines (b"key count") by (count descending, key bytes ascending)."""
    def order(ln):
        key, c = ln.rsplit(b" ", 1)
        return (-int(c), key)
    return sorted(lines, key=order)


def cat(lines):
    return b"".join(l + b"\n" for l in lines)


def oracle_lines(files, R, flags):
    """The lines of final.txt, unordered: what the reference writes (flags 0) or every word."""
    import oracle_lib as O
    if flags & NO_COMPAT:
        cnt = collections.Counter()
        for f in files:
            cnt.update(O.tokens(f))
        return [k + b" " + str(c).encode() for k, c in cnt.items()]
    return [l for o in O.wc(files, R, O.FAST) for l in o.split(b"\n") if l]


def start_job(ctx, blobs, R, flags=0):
    """map only; returns the device tensor (keep it alive while the job is used)"""
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    t, off = to_device(blobs)
    ctx.job_begin(M.APP_WC, R, flags)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    return t


# ---- 1. the bundled corpus

@pytest.fixture(scope="module")
def corpus_all_words(corpus):
    return oracle_lines(corpus, 1, NO_COMPAT)


@pytest.mark.parametrize("flags", [0, NO_COMPAT])
@pytest.mark.parametrize("R", [1, 10, 64])
def test_corpus_topk(ctx, corpus, corpus_all_words, R, flags):
    from gpu_util import run_wc
    exp = ranked(corpus_all_words if flags else oracle_lines(corpus, R, 0))
    n = len(exp)
    run_wc(ctx, corpus, R, flags=flags)
    fin = [l for l in ctx.final().split(b"\n") if l]
    assert len(fin) == n
    by_final = ranked(fin)
    for k in (0, 1, 10, 1000, n - 1, n, n + 5, 10**9):
        got = ctx.topk(k)
        assert got == cat(exp[:k]), (R, flags, k)
        assert got == cat(by_final[:k]), (R, flags, k)


# ---- 2. ties at every boundary of the select: counts from {1, 2, 3, 7} only

def tie_words():
    words = ["abcdefgh", "abcdefgh1", "abcdefgh2", "abcdefghi", "abcdefghij1", "abcdefghij2"]   # differ after byte 8
    words += [w + s for w in ("x" * 16, "x" * 16 + "a", "x" * 17, "x" * 30) for s in ("", "é")]  # ... after byte 16
    words += ["naïve", "ſong", "Ærø", "a"]
    words += ["w%02d" % i for i in range(42)]
    return words


@pytest.fixture(scope="module")
def tie_text():
    rng = random.Random(2026)
    toks = []
    for w in tie_words():
        toks += [w] * rng.choice((1, 2, 3, 7))
    rng.shuffle(toks)
    return " ".join(toks).encode()


@pytest.mark.parametrize("flags", [0, NO_COMPAT, 3 << 8])  # 3 << 8 = MRG_FLAG_DEBUG_HASH_BITS(3)
@pytest.mark.parametrize("R", [1, 5])
def test_ties_every_k(ctx, tie_text, R, flags):
    exp = ranked(oracle_lines([tie_text], R, flags))
    n = len(exp)
    nw = len(tie_words())
    assert n == nw if flags & NO_COMPAT else nw - R <= n < nw
    t = start_job(ctx, [tie_text], R, flags)
    for k in range(0, n + 2):
        assert ctx.topk(k) == cat(exp[:k]), (R, flags, k)
    del t


# ---- 3. drop-last: the most frequent word is the byte-largest key of its partition

def test_drop_last_of_the_top_word(ctx):
    rng = random.Random(5)
    filler = ["f%03d" % i for i in range(200)]
    toks = ["zz"] * 100 + [rng.choice(filler) for _ in range(3000)] + filler
    rng.shuffle(toks)
    text = " ".join(toks).encode()
    t = start_job(ctx, [text], 1, 0)
    got = ctx.topk(5)
    assert not got.startswith(b"zz ") and b"\nzz " not in got
    assert got == cat(ranked(oracle_lines([text], 1, 0))[:5])
    t = start_job(ctx, [text], 1, NO_COMPAT)
    got = ctx.topk(5)
    assert got.startswith(b"zz 100\n")
    assert got == cat(ranked(oracle_lines([text], 1, NO_COMPAT))[:5])
    exp = ranked(oracle_lines([text], 3, 0))
    t = start_job(ctx, [text], 3, 0)
    for k in (1, 2, 5, 50, len(exp), len(exp) + 1):
        assert ctx.topk(k) == cat(exp[:k]), k
    del t


# ---- 4. massive ties: near-unique keys, counts 1 or 2

@pytest.fixture(scope="module")
def unique_job(ctx):
    import torch
    n = 8 << 20
    t = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    ctx.gen_unique(t.data_ptr(), n, 0xC5, 3)
    host = t[:n].cpu().numpy().tobytes()
    exp = ranked(oracle_lines([host], 16, 0))
    return t, n, exp


@pytest.fixture
def wide():
    os.environ["MRG_WIDE"] = "1"
    yield
    del os.environ["MRG_WIDE"]


def check_unique(ctx, unique_job):
    import mapreduce_rust_amd as M
    t, n, exp = unique_job
    c2 = sum(1 for l in exp if l.endswith(b" 2"))
    assert 0 < c2 < len(exp) and len(exp) > 500000
    ctx.job_begin(M.APP_WC, 16)
    ctx.set_input(t.data_ptr(), [0, n])
    ctx.map()
    for k in (1, 100, c2, c2 + 1, 50000, len(exp)):
        got = ctx.topk(k)
        assert hashlib.sha256(got).digest() == hashlib.sha256(cat(exp[:k])).digest(), k


def test_massive_ties(ctx, unique_job):
    check_unique(ctx, unique_job)


def test_massive_ties_wide_result(ctx, unique_job, wide):
    check_unique(ctx, unique_job)
    assert ctx.stats()["agg_path"] == 2


# ---- 5. Zipf

def test_zipf(ctx):
    import torch
    import mapreduce_rust_amd as M
    n = 8 << 20
    t = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    ctx.gen_zipf(t.data_ptr(), n, 0x5EED2026, 0, 1 << 14, 1.1)
    host = t[:n].cpu().numpy().tobytes()
    exp = ranked(oracle_lines([host], 7, 0))
    ctx.job_begin(M.APP_WC, 7)
    ctx.set_input(t.data_ptr(), [0, n])
    ctx.map()
    for k in (1, 100, 5000):
        assert ctx.topk(k) == cat(exp[:k]), k


# ---- 6. 64-bit counts, through mrg_job_import

def test_counts_beyond_32_bits(ctx):
    """Exchange records (include/mrgpu.h): short key {u64 k0, u64 k1 big-endian packed, u32 v, u32 len},
    long key {u64 heap offset, u64 count, u32 0xFFFFFFFF, u32 len}."""
    import torch
    import mapreduce_rust_amd as M
    F = 0xFFFFFFFF

    def short(key, v):
        p = key.ljust(16, b"\0")
        return struct.pack("<QQII", int.from_bytes(p[:8], "big"), int.from_bytes(p[8:], "big"), v, len(key))
    sends = {b"high2": [F, F, 7],      # 2^33 + 5
             b"high1": [F, 6],         # 2^32 + 5: differs from high2 in the high word only
             b"low6": [F, F, 8],       # 2^33 + 6: differs from high2 in the low word only
             b"thrice": [F, F, F],
             b"small": [12],
             b"sixteen_bytes_kk": [F, 1]}
    longkey = b"a_key_of_twenty_bytes"
    recs, want = [], {}
    for key, vs in sends.items():
        recs += [short(key, v) for v in vs]
        want[key] = sum(vs)
    recs.append(struct.pack("<QQII", 0, (1 << 40) + 3, F, len(longkey)))
    want[longkey] = (1 << 40) + 3
    random.Random(3).shuffle(recs)
    assert want[b"high2"] >> 32 != want[b"high1"] >> 32 and want[b"high2"] & F == want[b"high1"] & F
    assert want[b"high2"] >> 32 == want[b"low6"] >> 32 and want[b"high2"] & F != want[b"low6"] & F
    exp = ranked([k + b" " + str(c).encode() for k, c in want.items()])
    assert exp[0] == b"a_key_of_twenty_bytes 1099511627779"
    R = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to("cuda:0")
    H = torch.frombuffer(bytearray(longkey + bytes(16)), dtype=torch.uint8).to("cuda:0")
    ctx.job_begin(M.APP_WC, 3, NO_COMPAT)
    ctx.import_(R.data_ptr(), len(recs), H.data_ptr(), len(longkey))
    for k in (1, 2, 3, 4, 5, len(exp), len(exp) + 3):
        assert ctx.topk(k) == cat(exp[:k]), k


# ---- 7. job state

def test_topk_leaves_the_job_alone(ctx, corpus):
    import oracle_lib as O
    docs = corpus[:3]
    exp = ranked(oracle_lines(docs, 10, 0))
    t = start_job(ctx, docs, 10)
    assert ctx.topk(10) == cat(exp[:10])          # before reduce
    ctx.reduce()
    outs = ctx.outputs()
    assert outs == O.wc(docs, 10, O.FAST)
    assert ctx.final() == cat(sorted(l for o in outs for l in o.split(b"\n") if l))
    assert ctx.topk(10) == cat(exp[:10])          # after reduce
    assert ctx.topk(333) == cat(exp[:333])        # another k
    held2 = ctx.pool_stats()[0]
    assert ctx.topk(10) == cat(exp[:10])
    assert ctx.pool_stats()[0] == held2           # every scratch block went back to the pool
    rec, heap = ctx.export_sizes(2)               # export after it still sees every key
    assert sum(rec) >= len(exp)
    del t


# ---- 8. errors

def test_topk_errors(ctx, corpus):
    import ctypes as C
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    L = M.load()
    EINVAL = M.native.EINVAL
    names = ["data/gut-0.txt"]
    run_wc(ctx, corpus[:1], 4, app=M.APP_INDEXER, names=names)
    with pytest.raises(M.MrgError) as ei:
        ctx.topk(5)
    assert ei.value.code == EINVAL
    ctx.job_begin(M.APP_WC, 4)
    with pytest.raises(M.MrgError) as ei:       # nothing mapped
        ctx.topk(5)
    assert ei.value.code == EINVAL
    buf = C.create_string_buffer(64)
    assert L.mrg_job_copy_topk(ctx.h, buf, 64) == EINVAL    # copy before topk
    assert b"mrg_job_topk" in L.mrg_last_error()
    t = start_job(ctx, corpus[:1], 4)
    n, lines = C.c_uint64(), C.c_uint64()
    assert L.mrg_job_topk(ctx.h, 3, None, C.byref(n), C.byref(lines)) == 0
    assert lines.value == 3 and n.value > 6
    assert L.mrg_job_copy_topk(ctx.h, buf, n.value - 1) == EINVAL   # cap too small
    assert L.mrg_job_topk(ctx.h, 3, None, None, None) == 0          # every out pointer may be NULL
    assert L.mrg_job_topk(None, 3, None, None, None) == EINVAL
    assert L.mrg_job_copy_topk(None, buf, 64) == EINVAL
    del t


# ---- 9. the whole job: top.txt from mrg_run_job and from the CLI

def test_run_job_and_cli_write_top_txt(tmp_path, corpus):
    import mapreduce_rust_amd as M
    d = tmp_path / "data"
    d.mkdir()
    files = []
    for m in range(6):
        (d / f"gut-{m}.txt").write_bytes(corpus[m])
        files.append(f"data/gut-{m}.txt")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        M.native.run_job(files, 10, M.APP_WC, ".", M.FLAG_FINAL_TXT | M.native.flag_top(25))
        with pytest.raises(M.MrgError) as ei:
            M.native.run_job(files, 10, M.APP_INDEXER, ".", M.native.flag_top(25))
        assert ei.value.code == M.native.EINVAL
    finally:
        os.chdir(cwd)
    fin = (tmp_path / "final.txt").read_bytes()
    assert hashlib.sha256(fin).hexdigest() == GOLDEN["wc"]["10"]["final.txt"]
    exp = cat(ranked([l for l in fin.split(b"\n") if l])[:25])
    top = (tmp_path / "top.txt").read_bytes()
    assert top == exp and top.count(b"\n") == 25
    (tmp_path / "top.txt").unlink()
    exe = os.path.join(ROOT, "mapreduce_rust_amd", "lib", "mrgpu")
    p = subprocess.run([exe, "6", "10", "--top", "25"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "top.txt").read_bytes() == exp
    p = subprocess.run([exe, "6", "10", "--top", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
