"""GPU tests: the indexer (MRG_APP_INDEXER) at many documents, through the C ABI, against the C oracle.

The inputs are those of tests/indexer_util.py; tests/test_indexer_cpu.py pins the oracle on the same inputs
against the Python twin.  Every expectation is byte equality with oracle_lib.indexer; where final() is checked it
must equal the bytewise sort of the lines of the job's own outputs(), which the same test checks against the oracle.

What is reached here and nowhere else: two and three document-rank bytes in the LSD radix sort (mrg_reduce.cpp
sort_plan, k_sort.hip RecTraits::digit), MSD buckets above MSD_LCAP records without a test knob, group sizes of
up to four digits and names of many lengths in k_idx_glen / k_idx_write, a rank table far from the identity in
k_make_sortrec, runs of equal 16-byte prefixes that hold several long keys over many documents (k_fix_runs,
k_final_part), the indexer's overflow and rerun paths, and MRG_EINVAL for a document id that has no name.

Full regions, full overflow lists and ids without a name are documented conditions with a defined return; nothing
here is meant to fault the device."""
import os
import random
import struct

import pytest

import indexer_util as U
from test_gpu_map_block_queue import knob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


def corpus2():
    import gzip
    return [gzip.open(os.path.join(HERE, "golden", "corpus", f"gut-{m}.txt.gz")).read() for m in range(2)]


_INPUTS, _EXPECT = {}, {}


def inputs(name, arg=None):
    """(docs, names) of a builder, built once"""
    if (name, arg) not in _INPUTS:
        build = getattr(U, name)
        _INPUTS[name, arg] = build() if arg is None else build(arg)
    return _INPUTS[name, arg]


def expect(name, arg, R, drop=True):
    """the oracle's mr-{r}.txt for a builder's input, computed once per (input, R).

    drop = False (MRG_FLAG_NO_COMPAT_DROP_LAST): the oracle always drops the last group of a partition.  So it is
    given one more document that holds one more word per partition, each sorting behind every key of the input:
    those sentinel groups are the ones it drops, and every group of the input itself is kept."""
    key = (name, arg, R, drop)
    if key in _EXPECT:
        return _EXPECT[key]
    import oracle_lib as O
    docs, names = inputs(name, arg)
    if drop:
        out = O.indexer(docs, names, R)
    else:
        # U+FF5A (a letter, bytes EF BD 9A) + digits sorts behind every key of these inputs, whose first bytes are
        # at most 0xC5; candidates are hashed until every partition has one
        need, words, i = set(range(R)), [], 0
        while need:
            w = ("\uff5a%d" % i).encode()
            assert O.tokens(w) == [w]
            r = O.key_hash(w) % R
            if r in need:
                need.discard(r)
                words.append(w)
            i += 1
        assert max(t[0] for d in docs for t in O.tokens(d)) <= 0xC5
        out = O.indexer(docs + [b" ".join(words)], names + ["sentinel"], R)
        assert not any("\uff5a".encode() in o for o in out)      # every sentinel group was the dropped one
    _EXPECT[key] = out
    return out


def final_of(outs):
    """run.sh:16-20 restated: every line of every mr-{r}.txt, sorted bytewise"""
    lines = [ln for o in outs for ln in o.split(b"\n") if ln]
    return b"".join(ln + b"\n" for ln in sorted(lines))


def run_ix(ctx, docs, names, R, flags=0, final=False):
    """one indexer job: outputs(), and final() checked against them"""
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    outs = run_wc(ctx, docs, R, app=M.APP_INDEXER, flags=flags, names=names)
    if final:
        assert ctx.final() == final_of(outs)
    return outs


# ---------------------------------------------------------------- 1. group sizes

@pytest.mark.parametrize("keep_last", [False, True])
@pytest.mark.parametrize("R", [1, 7])
def test_group_sizes(ctx, R, keep_last):
    """groups of 1 .. 1001 documents: sizes of one to four digits (mrg_ndigits in k_idx_glen, put_u64 in
    k_idx_write), names of 4 .. 7 bytes placed at P[i] - P[s] behind them; the last group of a partition dropped
    and kept"""
    import mapreduce_rust_amd as M
    docs, names = inputs("digits")
    exp = expect("digits", None, R, drop=not keep_last)
    got = run_ix(ctx, docs, names, R, flags=M.FLAG_NO_COMPAT_DROP_LAST if keep_last else 0, final=True)
    assert got == exp
    lines = {ln.split(b" ", 1)[0]: ln for o in exp for ln in o.split(b"\n") if ln}
    for n in U.DIGITS_N:
        if b"g%d" % n in lines:       # (a gN that is its partition's last group is dropped)
            assert lines[b"g%d" % n].startswith(b"g%d %d " % (n, n))
            assert lines[b"g%d" % n].count(b",") == n - 1
    if keep_last and R == 1:
        # the last group of the partition is a many-document group: x4, 200 documents (asserted on the oracle)
        last = exp[0].rstrip(b"\n").rsplit(b"\n", 1)[-1]
        assert last.startswith(b"x4 200 ") and last.count(b",") == 199
        assert len(lines) == len(U.DIGITS_N) + 37 + 5


# ---------------------------------------------------------------- 2. document-rank bytes

def sort_modes(n):
    """the default sort; everything through the LSD radix sort; at 256 / 257 also some buckets through it"""
    return [{}, {"MRG_TEST_SORT_LCAP": 1}] + ([{"MRG_TEST_SORT_LCAP": 48}] if n in (256, 257) else [])


@pytest.mark.parametrize("R", [1, 10])
@pytest.mark.parametrize("n", U.RANKS_N)
def test_document_rank_bytes(ctx, n, R):
    """1, 2, 255 .. 257, 65536 and 65537 documents with permuted names: one, two and three rank bytes in the LSD
    sort (doc_bytes = bytes_for(n - 1)), which orders the documents of `the` (all n) by rank alone"""
    docs, names = inputs("ranks", n)
    exp = expect("ranks", n, R)
    if n > 2:   # the group over all n documents is written, not the one its partition drops
        assert any(ln.startswith(b"the %d " % n) for o in exp for ln in o.split(b"\n"))
    for env in sort_modes(n):
        with knob(**env):
            got = run_ix(ctx, docs, names, R, final=n in (257, 65537) and not env)
        assert got == exp, env


# ---------------------------------------------------------------- 3. name order

@pytest.mark.parametrize("R", [1, 3])
def test_name_order(ctx, R):
    """names that are prefixes of one another, differ after 16 and 32 bytes, hold bytes >= 0x80, repeat, or are
    empty: the documents of a word come in the bytewise order of their names"""
    import oracle_lib as O
    docs, names = inputs("name_order")
    got = run_ix(ctx, docs, names, R, final=True)
    assert got == expect("name_order", None, R)
    # the same documents with the names in id order (rank == id): another output, so the permutation is what is tested
    in_order = sorted(names, key=lambda s: s.encode())
    got2 = run_ix(ctx, docs, in_order, R)
    assert got2 == O.indexer(docs, in_order, R)
    assert got2 != got


# ---------------------------------------------------------------- 4. natural oversized buckets

@pytest.mark.parametrize("k,R", [(1, 1), (16, 1), (17, 1), (17, 10)])
def test_natural_oversized_buckets(ctx, k, R):
    """k words in each of 2049 documents: k MSD buckets of 2049 > MSD_LCAP records (the bucket id holds no
    document bits).  k = 1 and 16: each bucket by the LSD sort on its segment; k = 17 > MSD_MAX_BIG: the whole
    array through the LSD sort.  Two rank bytes, no sort knob (test_indexer_cpu.py checks the bucket sizes and
    both constants)."""
    assert "MRG_TEST_SORT_LCAP" not in os.environ
    docs, names = inputs("oversized", k)
    exp = expect("oversized", k, R)
    # every 2049-document group is written (the own words sort behind the shared ones: none is a last group)
    assert sum(1 for o in exp for ln in o.split(b"\n") if b" %d " % U.OVERSIZED_DOCS in ln[:16]) == k
    assert run_ix(ctx, docs, names, R) == exp


# ---------------------------------------------------------------- 5. long keys across documents

@pytest.mark.parametrize("bits", [0, 4, 1])
@pytest.mark.parametrize("R", [1, 5])
def test_long_keys_across_documents(ctx, R, bits):
    """a 16-byte key and long keys that extend it, each in its own subset of 40 documents: a run of equal
    prefixes arrives ordered by document rank and k_fix_runs regroups it by key; k_final_part finds the last group
    across its documents.  Also with internal hashes truncated to 4 bits and 1 bit."""
    import mapreduce_rust_amd as M
    docs, names = inputs("long_runs")
    got = run_ix(ctx, docs, names, R, flags=M.debug_hash_bits(bits) if bits else 0, final=True)
    assert got == expect("long_runs", None, R)


def test_long_keys_last_group_kept(ctx):
    """the same with the last group kept: at R = 1 it is a group over all 40 documents"""
    import mapreduce_rust_amd as M
    docs, names = inputs("long_runs")
    exp = expect("long_runs", None, 1, drop=False)
    assert exp[0].rstrip(b"\n").rsplit(b"\n", 1)[-1].startswith("ſlast 40 ".encode())
    assert run_ix(ctx, docs, names, 1, flags=M.FLAG_NO_COMPAT_DROP_LAST, final=True) == exp


# ---------------------------------------------------------------- 6. overflow and rerun paths

# The knobs of these jobs size device blocks (overflow lists of 2^22 records per bucket), which a closed context
# leaves in the library's process-wide device cache; tests/test_gpu_scale.py counts the allocations of a fresh
# context of the same process.  So, as in tests/test_gpu_map_runs.py, they run in ONE child process started by a
# module fixture; it prints what it saw and the tests here judge it.

LDS_SLOTS = 4096          # k_keys.hip ba_cap<IDX>: the indexer's LDS table of one aggregation workgroup
MAX_NSUB = 16             # mrg_agg.cpp: at most 16 workgroups (sub-ranges) per bucket
MAP_SLOTS = 4096          # k_map.hip: at most 4096 slots in a map workgroup's LDS table
NBUCKET = 256             # mrg_internal.h MRG_NBUCKET

# The three map cases run with MRG_TEST_MAP_GRID=1.  On the job's own grid (one workgroup per few blocks of this
# 1.8 MB input) every workgroup's LDS table holds all it sees, and whether a record reaches the tail stream at all
# depends on the device's size; with ONE workgroup the counts of the input alone decide it (see the assertions).
OVERFLOW_CASES = {
    "agg_regrow": dict(bits=4, env=dict(MRG_TEST_AGG_OCAP=1000)),
    "nsub3": dict(bits=0, env=dict(MRG_TEST_AGG_NSUB=3)),
    "nsub16": dict(bits=0, env=dict(MRG_TEST_AGG_NSUB=16)),
    "spill": dict(bits=0, env=dict(MRG_TEST_TAIL_CAP=1, MRG_TEST_OVF_CAP=1 << 22, MRG_TEST_MAP_GRID=1)),
    "rerun": dict(bits=0, env=dict(MRG_TEST_TAIL_CAP=1, MRG_TEST_OVF_CAP=16, MRG_TEST_MAP_GRID=1)),
    "long_rerun": dict(bits=0, env=dict(MRG_TEST_LONG_PER=1, MRG_TEST_LONG_LIST=3, MRG_TEST_MAP_GRID=1)),
}


def overflow_input():
    docs, names = U.pairs(300)
    c = corpus2()
    return docs + c, names + ["data/gut-0.txt", "data/gut-1.txt"]


def overflow_jobs():
    """(the child process) every case of OVERFLOW_CASES at R = 10; one JSON line on stdout"""
    import json
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    docs, names = overflow_input()
    exp = O.indexer(docs, names, 10)
    toks = [set(O.tokens(d)) for d in docs]
    out = {"pairs": sum(len(t) for t in toks), "long_pairs": sum(1 for t in toks for w in t if len(w) > 16), "jobs": {}}
    with M.Context(0) as ctx:
        for tag, case in OVERFLOW_CASES.items():
            with knob(**case["env"]):
                got = run_wc(ctx, docs, 10, app=M.APP_INDEXER, names=names,
                             flags=M.debug_hash_bits(case["bits"]) if case["bits"] else 0)
                st = ctx.stats()
                fin = ctx.final() if tag in ("agg_regrow", "rerun") else None
            out["jobs"][tag] = {"equal": got == exp, "final": fin is None or fin == final_of(got),
                                **{k: st[k] for k in ("agg_launches", "overflow_keys", "map_spill", "map_launches",
                                                      "agg_path", "map_kind", "distinct_keys", "long_tokens")}}
    print("RESULT " + json.dumps(out), flush=True)


@pytest.fixture(scope="module")
def overflow_results():
    import json
    import subprocess
    import sys
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, p.stdout[-2000:]
    return json.loads(line[0][len("RESULT "):])


@pytest.mark.parametrize("tag", list(OVERFLOW_CASES))
def test_overflow_and_rerun_paths(overflow_results, tag):
    """300 documents of 200 distinct words plus two corpus files, R = 10: B.odoc of the bucket aggregation and
    T.tdoc of table_aggregate (agg_regrow), the sub-range split (nsub3, nsub16), 24-byte tail records through the
    overflow lists (spill) and through a map rerun (rerun), long-token regions regrown (long_rerun).  Each
    condition below follows from counts of the input alone (the oracle's tokenizer), so a case that no longer
    reaches its path fails."""
    P, PL = overflow_results["pairs"], overflow_results["long_pairs"]
    j = overflow_results["jobs"][tag]
    assert j["equal"] and j["final"], j
    assert j["distinct_keys"] == P and j["agg_path"] == 1 and j["map_kind"] == 0, j
    if tag == "agg_regrow":
        # 4-bit hashes: every (word, document) pair lies in ONE bucket, whose at most MAX_NSUB workgroups hold
        # at most LDS_SLOTS pairs each: the others are overflow records, more than the list of 1000 holds
        assert P - MAX_NSUB * LDS_SLOTS > 1000, P
        assert j["agg_launches"] >= 2 and j["overflow_keys"] > 1000, j
    if tag in ("spill", "rerun"):
        # one map workgroup (MRG_TEST_MAP_GRID=1): its LDS table keeps at most MAP_SLOTS of the P - PL short
        # pairs and its NBUCKET tail regions one record each; the rest goes to the overflow lists ...
        over = P - PL - MAP_SLOTS - NBUCKET
        assert over > NBUCKET * 16, (P, PL)
        if tag == "spill":
            assert j["map_spill"] > 0 and j["map_launches"] == 1, j
        else:       # ... which hold NBUCKET * 16 records: the launch overflows and the map runs again
            assert j["map_launches"] >= 2, j
    if tag == "long_rerun":
        # one workgroup's long-token region of 1 record and a shared list of 3: more long (word, document) pairs
        # than 4, so the launch is repeated with regions grown to the demand
        assert PL > 4 and j["long_tokens"] >= PL, (PL, j)
        assert j["map_launches"] >= 2, j


# ---------------------------------------------------------------- 7. batches

def add_batch(ctx, blobs, doc_ids):
    """set_input + map_add of one batch; the buffer is overwritten and released afterwards"""
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


@pytest.mark.parametrize("name,arg,R", [("ranks", 257, 10), ("pairs", 300, 10), ("ranks", 257, 1)])
def test_batches_with_scattered_ids(ctx, name, arg, R):
    """7 batches of whole documents in a shuffled order, the ids of a batch non-contiguous and descending
    (id % 7 == b, from the largest down): reduce, outputs and final equal the one-shot job's"""
    import mapreduce_rust_amd as M
    docs, names = inputs(name, arg)
    exp = expect(name, arg, R)
    order = list(range(7))
    random.Random(7).shuffle(order)
    assert order != sorted(order)
    ctx.job_begin(M.APP_INDEXER, R)
    ctx.set_doc_names(names)
    for b in order:
        ids = [d for d in range(len(docs) - 1, -1, -1) if d % 7 == b]
        assert ids == sorted(ids, reverse=True) and ids[0] - ids[1] == 7
        add_batch(ctx, [docs[d] for d in ids], ids)
    assert ctx.stats()["map_batches"] == 7
    ctx.reduce()
    got = ctx.outputs()
    assert got == exp
    assert ctx.final() == final_of(exp)
    assert run_ix(ctx, docs, names, R) == got          # the one-shot job


# ---------------------------------------------------------------- 8. exchange and plugin surface

@pytest.mark.parametrize("G", [1, 3])
def test_export_import_with_global_ids(ctx, G):
    """ranks(257) mapped in two shards with global document ids, exported to G owners (part % G) and imported:
    the union of the owners' partitions equals the oracle (the structure of test_export_import_many_owners)"""
    import torch
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    X = M.native.XREC_BYTES
    R = 10
    docs, names = inputs("ranks", 257)
    exp = expect("ranks", 257, R)
    shards = [[d for d in range(257) if d % 3 == 0][::-1], [d for d in range(257) if d % 3 != 0]]
    sends = []
    for ids in shards:
        t, off = to_device([docs[d] for d in ids])
        ctx.job_begin(M.APP_INDEXER, R)
        ctx.set_doc_names(names)
        ctx.set_input(t.data_ptr(), off, ids)
        ctx.map()
        rec, heap = ctx.export_sizes(G)
        drec = torch.empty(max(sum(rec), 1) * X, dtype=torch.uint8, device="cuda:0")
        dheap = torch.empty(max(sum(heap), 1), dtype=torch.uint8, device="cuda:0")
        ctx.export(drec.data_ptr(), dheap.data_ptr())
        sends.append((drec.cpu(), dheap.cpu(), rec, heap))
        del t
    got = [None] * R
    for owner in range(G):
        recs, heaps, sr, shp = [], [], [], []
        for drec, dheap, rec, heap in sends:
            ro = sum(rec[:owner]) * X
            ho = sum(heap[:owner])
            recs.append(drec[ro:ro + rec[owner] * X])
            heaps.append(dheap[ho:ho + heap[owner]])
            sr.append(rec[owner])
            shp.append(heap[owner])
        Rt = torch.cat(recs + [torch.zeros(X, dtype=torch.uint8)]).to("cuda:0")
        Ht = torch.cat(heaps + [torch.zeros(1, dtype=torch.uint8)]).to("cuda:0")
        ctx.job_begin(M.APP_INDEXER, R)
        ctx.set_doc_names(names)
        ctx.import_(Rt.data_ptr(), sum(sr), Ht.data_ptr(), sum(shp), sr, shp)
        ctx.reduce()
        o = ctx.outputs()
        for r in range(R):
            if r % G == owner:
                got[r] = o[r]
            else:
                assert o[r] == b"", (owner, r)
    assert got == exp


@pytest.mark.parametrize("R", [1, 3])
def test_plugin_surface_per_document(ctx, R):
    """mrg_map per document with its global id, for the 40 documents of name_order(), then mrg_reduce with the
    names for every partition"""
    import mapreduce_rust_amd as M
    docs, names = inputs("name_order")
    exp = expect("name_order", None, R)
    parts = [ctx.map_task(M.APP_INDEXER, docs[d], names[d], d, R) for d in range(len(docs))]
    try:
        for r in range(R):
            assert ctx.reduce_task(M.APP_INDEXER, r, parts, R, doc_names=names) == exp[r], r
    finally:
        for p in parts:
            p.free()


# ---------------------------------------------------------------- 9. ids without a name

CLEAN_DOCS = [b"alpha beta gamma", b"beta gamma delta", b"gamma delta epsilon zeta"]
CLEAN_NAMES = ["c.txt", "a.txt", "b.txt"]


def clean_job(ctx):
    import oracle_lib as O
    assert run_ix(ctx, CLEAN_DOCS, CLEAN_NAMES, 2, final=True) == O.indexer(CLEAN_DOCS, CLEAN_NAMES, 2)


def einval(call, *words):
    import mapreduce_rust_amd as M
    with pytest.raises(M.MrgError) as e:
        call()
    assert e.value.code == M.native.EINVAL, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_set_input_id_without_a_name(ctx):
    """set_input(doc_ids=[0, 5]) with three names: MRG_EINVAL at reduce() and at final(), naming the id and the
    number of names; the context then runs a clean job and holds no more blocks than before"""
    import torch
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    clean_job(ctx)
    t, off = to_device([b"one two", b"two three"])
    ctx.job_begin(M.APP_INDEXER, 2)
    before = ctx.pool_stats()[0]
    ctx.set_doc_names(["x", "y", "z"])
    ctx.set_input(t.data_ptr(), off, [0, 5])
    ctx.map()
    einval(ctx.reduce, "document id 5", "3 names")
    einval(ctx.final, "document id 5", "3 names")
    torch.cuda.synchronize()
    del t
    ctx.job_begin(M.APP_INDEXER, 2)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    clean_job(ctx)


def test_map_task_id_without_a_name(ctx):
    """mrg_map(doc_id=9) reduced with two names: MRG_EINVAL from mrg_reduce"""
    import mapreduce_rust_amd as M
    clean_job(ctx)
    ctx.job_begin(M.APP_INDEXER, 1)
    before = ctx.pool_stats()[0]
    parts = ctx.map_task(M.APP_INDEXER, b"one two three", "nine", 9, 1)
    try:
        einval(lambda: ctx.reduce_task(M.APP_INDEXER, 0, [parts], 1, doc_names=["x", "y"]), "document id 9", "2 names")
    finally:
        parts.free()
    ctx.job_begin(M.APP_INDEXER, 1)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    clean_job(ctx)


def test_imported_id_without_a_name(ctx):
    """one imported exchange record with v = 1000 and four names: MRG_EINVAL at reduce()"""
    import torch
    import mapreduce_rust_amd as M
    clean_job(ctx)
    key = b"word"
    rec = struct.pack("<QQII", int.from_bytes(key.ljust(8, b"\0"), "big"), 0, 1000, len(key))
    assert len(rec) == M.native.XREC_BYTES
    d_rec = torch.frombuffer(bytearray(rec + bytes(M.native.XREC_BYTES)), dtype=torch.uint8).to("cuda:0")
    d_heap = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    ctx.job_begin(M.APP_INDEXER, 1)
    before = ctx.pool_stats()[0]
    ctx.set_doc_names(["p", "q", "r", "s"])
    ctx.import_(d_rec.data_ptr(), 1, d_heap.data_ptr(), 0)
    einval(ctx.reduce, "document id 1000", "4 names")
    torch.cuda.synchronize()
    del d_rec, d_heap
    ctx.job_begin(M.APP_INDEXER, 1)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    clean_job(ctx)


if __name__ == "__main__":
    import sys
    root = os.path.dirname(HERE)
    for d in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        sys.path.insert(0, d)
    overflow_jobs()
