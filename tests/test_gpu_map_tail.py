"""GPU tests: k_map's tail append with packed cursors (one 64-bit LDS word per bucket and record class: the next
record index below, the region's end above) and the 13..16-byte keys appended off the token round, against the
64-bit cursors the host falls back to (MRG_TEST_TAIL64=1 forces them).

Every expectation is the C oracle's (oracle_lib) over inputs built here from fixed seeds.  Every case runs with
both cursor forms and with MRG_TEST_MAP_GRID 1 and 3 (one workgroup's 16 waves share every region; three
workgroups' shares end inside the text), wc with the 4096- and the 2048-slot table and, where it says so, the
indexer.  MRG_TEST_TAIL_CAP makes regions of 1, 2 and 33 records, so a cursor runs on past its region's end --
the count the host sizes a rerun from -- and the records go to the overflow lists.

The jobs run in ONE child process, started by a module fixture; it prints what it saw and the tests here judge
it.  Their contexts end with device blocks of many sizes (regions of 1 record, overflow lists of 2^20), which a
closed context leaves in the library's process-wide device cache; that cache has no release call, and
tests/test_gpu_scale.py counts the allocations of a fresh context of the same process (as in
tests/test_gpu_map_runs.py).

A full region and a full overflow list are documented conditions with a defined rerun; nothing here is meant to
fault the device."""
import random

import pytest

from test_gpu_map_block_queue import knob

pytestmark = pytest.mark.gpu

GRIDS = (1, 3)
TAIL64 = (None, 1)
LDS_CAPS = (4096, 2048)
TAIL_CAPS = (1, 2, 33)
R = 3
CLASS_CASES = ("12/13", "13/12", "12/16", "16/12", "one13")


# ---------------------------------------------------------------- inputs

def word(i, L):
    """L lowercase letters, i in base 26 in the first four: distinct for distinct (i, L), i < 26 ** min(L, 4)"""
    out = bytearray()
    for k in range(L):
        out.append(97 + (i % 26 if k < 4 else (i * 7 + k * 11 + L) % 26))
        if k < 4:
            i //= 26
    return bytes(out)


def words_of(lengths, n, first=0):
    """n words, word j of length lengths[j % len(lengths)]"""
    return [word(first + j, lengths[j % len(lengths)]) for j in range(n)]


def text(words):
    return b" ".join(words) + b" "


def miss_docs():
    """12 000 distinct words of every length 3..16 and some of 17, 19 and 22 bytes (long-token records ride
    along), the 26 one-letter and 26 two-letter words behind them, twice over in two orders and two documents:
    more keys than both ways of every set of either table, so the tail carries nearly every token"""
    rng = random.Random(2701)
    a = words_of(tuple(range(3, 17)) + (17, 19, 22), 12000)
    a += [bytes([97 + k]) for k in range(26)] + [bytes([97 + k, 97 + (k + 1) % 26]) for k in range(26)]
    b = list(a)
    rng.shuffle(b)
    return [text(a), text(b)]


def class_docs(name):
    if name == "one13":   # exactly one 13-byte word in a text of keys of <= 12 bytes: the cold block, one lane
        ws = words_of((3, 5, 8, 12, 7), 6000)
        ws[3333] = b"thirteenbytes"
        assert len(ws[3333]) == 13
        return [text(ws)]
    # distinct words, token j of la bytes when (j // 64) % 2 == 0 and of lb bytes otherwise: queue entries q and
    # q + 64 of a round differ in class
    la, lb = map(int, name.split("/"))
    return [text([word(j, la if (j // 64) % 2 == 0 else lb) for j in range(6000)])]


def no16_docs():
    """no key of 13..16 bytes (17 and 20 are long tokens): the cold block never runs"""
    return [text(words_of((3, 5, 8, 12, 7, 17, 20), 6000))]


def full_docs():
    """12 000 distinct words of 13..16 bytes, 20 000 tokens of them, and 12 000 distinct words of 3..5 bytes,
    32 000 tokens of them, shuffled: with regions of 33 records both classes still overflow (some 21 and 35
    records per bucket and workgroup at a grid of 3, three times that at a grid of 1)"""
    rng = random.Random(2702)
    w16 = words_of((13, 14, 15, 16), 12000)
    w12 = words_of((3, 4, 5), 12000, first=40000)
    toks = w16 + w16[:8000] + w12 + w12 + w12[:8000]
    rng.shuffle(toks)
    half = len(toks) // 2
    return [text(toks[:half]), text(toks[half:])]


# ---------------------------------------------------------------- the child process

def variants():
    for t64 in TAIL64:
        for grid in GRIDS:
            env = {"MRG_TEST_MAP_GRID": grid}
            if t64 is not None:
                env["MRG_TEST_TAIL64"] = t64
            yield f"tail64 {t64}, grid {grid}", env


class Case:
    def __init__(self, docs):
        import oracle_lib as O
        assert sum(map(len, docs)) <= 600 << 10
        self.docs = docs
        self.names = [f"d/{i}.txt" for i in range(len(docs))]
        toks = [t for d in docs for t in O.tokens(d) if t]
        self.facts = {"tokens": len(toks), "distinct": len(set(toks)),
                      "has16": any(13 <= len(t) <= 16 for t in toks)}
        self.exp_wc = O.wc(docs, R, O.FAST)
        self._exp_ix = None

    def exp_ix(self):
        import oracle_lib as O
        if self._exp_ix is None:
            self._exp_ix = O.indexer(self.docs, self.names, R)
        return self._exp_ix


KEEP = ("map_kind", "tokens", "distinct_keys", "tail_records_16", "map_launches", "map_spill")


def run(ctxs, case, tag, lds, app="wc", **env):
    """one job: {what ran, whether it gave the oracle's bytes, the counters}"""
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    ctx = ctxs[lds]
    with knob(**env):
        if app == "wc":
            equal = run_wc(ctx, case.docs, R) == case.exp_wc
        else:
            equal = run_wc(ctx, case.docs, R, app=M.APP_INDEXER, names=case.names) == case.exp_ix()
        st = ctx.stats()
    return {"tag": f"{tag}, table {lds}, {app}", "app": app, "equal": equal, **{k: st[k] for k in KEEP}}


def run_all(ctxs, case, indexer=False, **env):
    out = []
    for tag, venv in variants():
        for lds in LDS_CAPS:
            out.append(run(ctxs, case, tag, lds, **venv, **env))
        if indexer:
            out.append(run(ctxs, case, tag, 4096, app="indexer", **venv, **env))
    return out


def child_jobs():
    """(the child process) every job of this module; one JSON line on stdout"""
    import json
    import mapreduce_rust_amd as M
    ctxs = {}
    for lds in LDS_CAPS:      # MRG_LDS_CAP is read when a context is made
        with knob(MRG_LDS_CAP=lds):
            ctxs[lds] = M.Context(0)
    out = {}
    case = Case(miss_docs())
    out["miss"] = {"facts": case.facts, "jobs": run_all(ctxs, case, indexer=True)}
    for name in CLASS_CASES:
        case = Case(class_docs(name))
        out[name] = {"facts": case.facts, "jobs": run_all(ctxs, case)}
    case = Case(no16_docs())
    out["no16"] = {"facts": case.facts, "jobs": run_all(ctxs, case)}
    case = Case(full_docs())
    out["full"] = {"facts": case.facts}
    for cap in TAIL_CAPS:
        out["full"][f"lists/{cap}"] = run_all(ctxs, case, MRG_TEST_TAIL_CAP=cap, MRG_TEST_OVF_CAP=1 << 20)
        out["full"][f"rerun/{cap}"] = run_all(ctxs, case, MRG_TEST_TAIL_CAP=cap, MRG_TEST_OVF_CAP=16)
    ix = {"lists": [], "rerun": []}
    for tag, venv in variants():    # the indexer's one class (24-byte records) through full regions
        ix["lists"].append(run(ctxs, case, tag, 4096, app="indexer", MRG_TEST_TAIL_CAP=2, MRG_TEST_OVF_CAP=1 << 20,
                               **venv))
        ix["rerun"].append(run(ctxs, case, tag, 4096, app="indexer", MRG_TEST_TAIL_CAP=2, MRG_TEST_OVF_CAP=16, **venv))
    out["full"]["indexer"] = ix
    for c in ctxs.values():
        c.close()
    print("RESULT " + json.dumps(out), flush=True)


@pytest.fixture(scope="module")
def results():
    import json
    import os
    import subprocess
    import sys
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, p.stdout[-2000:]
    return json.loads(line[0][len("RESULT "):])


# ---------------------------------------------------------------- the tests

def expected_jobs(indexer=False):
    return len(TAIL64) * len(GRIDS) * (len(LDS_CAPS) + (1 if indexer else 0))


def judge(jobs, facts, n):
    """every job gave the oracle's bytes; every wc job ran the LDS-combine map and counted what the text holds"""
    assert len(jobs) == n, (len(jobs), n)
    for j in jobs:
        assert j["equal"], j
        if j["app"] == "wc":
            assert j["map_kind"] == 0, j
            assert j["tokens"] == facts["tokens"] and j["distinct_keys"] == facts["distinct"], (j, facts)
            assert (j["tail_records_16"] > 0) == facts["has16"], (j, facts)


def test_most_tokens_miss(results):
    """more distinct keys than either table holds, of every length 1..16 and some longer: wc and the indexer"""
    r = results["miss"]
    assert r["facts"]["distinct"] > 12000 and r["facts"]["has16"]
    judge(r["jobs"], r["facts"], expected_jobs(indexer=True))


@pytest.mark.parametrize("name", CLASS_CASES)
def test_both_classes_in_one_round(results, name):
    """a lane's two tokens of a round in different classes (12 / 13, 12 / 16, either first), and the cold block
    taken by a single lane"""
    r = results[name]
    assert r["facts"]["has16"]
    judge(r["jobs"], r["facts"], expected_jobs())


def test_no_long_class_no_16_byte_records(results):
    """a text without a key of 13..16 bytes leaves the 16-byte regions empty"""
    r = results["no16"]
    assert not r["facts"]["has16"]
    judge(r["jobs"], r["facts"], expected_jobs())


@pytest.mark.parametrize("cap", TAIL_CAPS)
def test_full_regions_overflow_lists(results, cap):
    """regions of `cap` records, long overflow lists: one launch, the records in the lists, the oracle's bytes"""
    r = results["full"]
    assert r["facts"]["has16"]
    jobs = r[f"lists/{cap}"]
    judge(jobs, r["facts"], expected_jobs())
    for j in jobs:
        assert j["map_launches"] == 1 and j["map_spill"] > 0, j


@pytest.mark.parametrize("cap", TAIL_CAPS)
def test_full_regions_rerun(results, cap):
    """the overflow lists hold 16 records as well: the launch is rerun with regions sized from the counts that
    ran on past the regions' ends, and then gives the oracle's bytes"""
    r = results["full"]
    jobs = r[f"rerun/{cap}"]
    judge(jobs, r["facts"], expected_jobs())
    for j in jobs:
        assert j["map_launches"] > 1, j


def test_full_regions_indexer(results):
    """the indexer's one class (24-byte records) through full regions, both outcomes"""
    ix = results["full"]["indexer"]
    n = len(TAIL64) * len(GRIDS)
    judge(ix["lists"], results["full"]["facts"], n)
    judge(ix["rerun"], results["full"]["facts"], n)
    for j in ix["lists"]:
        assert j["map_launches"] == 1 and j["map_spill"] > 0, j
    for j in ix["rerun"]:
        assert j["map_launches"] > 1, j


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        sys.path.insert(0, d)
    child_jobs()
