"""GPU tests: k_map's runs of blocks (a wave claims MRG_MAP_RUN consecutive blocks of its workgroup's share per
LDS atomic, derives a block's bounds from its predecessor's inside a document, and masks bytes outside the
document only in a block that holds some), the exact pool budget and the bounded tile list.

Every expectation is the C oracle's (oracle_lib) over inputs built here from fixed seeds; every case runs with
MRG_MAP_RUN = 1, 2, 4 and 8 (the one-entry tile list: 1 and 8) and must give the oracle's bytes each time.  MRG_TEST_MAP_GRID makes a workgroup's
share many blocks long (a job's grid is otherwise one workgroup per block on inputs this small), so that
its 16 waves walk runs: with a grid of 1 the runs start at multiples of the run length, with a grid of 3 the
shares' ends cut them short.

Invalid UTF-8 is a documented input with a defined error return; nothing here is meant to fault the device."""
import pytest

from test_gpu_map_block_queue import BLK, filler, knob, layout

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 4, 8)
GRIDS = (1, 3)


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


def tokens_of(docs):
    import oracle_lib as O
    return sum(1 for d in docs for t in O.tokens(d) if t)


def check_all_runs(ctx, docs, R=3, apps=("wc", "indexer", "wide"), grids=GRIDS, **env):
    """wc (the block queue), the indexer (per tile) and the forced wide map over docs, per run length and grid"""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    names = [f"d/{i}.txt" for i in range(len(docs))]
    exp_wc = O.wc(docs, R, O.FAST)
    exp_ix = O.indexer(docs, names, R) if "indexer" in apps else None
    ntok = tokens_of(docs)
    for grid in grids:
        for run in RUNS:
            with knob(MRG_MAP_RUN=run, MRG_TEST_MAP_GRID=grid, **env):
                tag = f"run {run}, grid {grid}"
                if "wc" in apps:
                    got = run_wc(ctx, docs, R)
                    st = ctx.stats()
                    assert st["map_kind"] == 0, (tag, st)
                    assert got == exp_wc, tag
                    assert st["tokens"] == ntok, (tag, st)
                if "indexer" in apps:
                    assert run_wc(ctx, docs, R, app=M.APP_INDEXER, names=names) == exp_ix, tag
                if "wide" in apps:
                    with knob(MRG_WIDE_MAP=1):
                        got = run_wc(ctx, docs, R)
                        st = ctx.stats()
                    assert st["map_kind"] == 1, (tag, st)
                    assert got == exp_wc, tag


# ---------------------------------------------------------------- document lengths and placement

LENGTHS = (0, 1, 15, 16, 17, 2047, 2048, 2049, 2048 + 63, 2048 + 64, 2048 + 65, 4 * 2048 - 1, 4 * 2048 + 1,
           5 * 2048 + 7)


def off_grid(lengths):
    """documents of these lengths back to back, a 3-byte document in front of each one that would otherwise
    start on the 16-byte grid: every listed document starts off the grid"""
    docs, at = [], 0
    for n in lengths:
        if at % 16 == 0:
            docs.append(b"p q")
            at += 3
        assert at % 16 != 0
        docs.append(filler(n, 4000 + n))
        at += n
    return docs


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_document_lengths(ctx, order):
    """documents of 0 .. 5 blocks + 7 bytes, off the 16-byte grid, in two orders: their first and last blocks
    fall in the first, a middle and the last block of a run and on run edges, per run length"""
    docs = off_grid(LENGTHS if order == "ascending" else LENGTHS[::-1])
    check_all_runs(ctx, docs)


# ---------------------------------------------------------------- tokens across the blocks of a run

NBLK = 40
LONG = bytes(97 + k % 26 for k in range(70))      # a token of more than 64 bytes: the slow path, a long key


def crossing(kind, edge):
    """(position, bytes) of what crosses (or meets) the block boundary at byte `edge`"""
    cps = {"cp2": "é", "cp3": "中", "cp4": "\U00010400"}
    if kind == "plain":
        return edge - 5, b"crossingit"
    if kind == "apostrophe":
        return edge - 3, b"don't"
    if kind == "long":
        return edge - 33, LONG
    if kind == "ends":           # a block ending in a word byte, the next one starting with a space
        return edge - 5, b"ended"
    if kind == "starts":         # a block ending in a space, the next one starting with a word byte
        return edge, b"started"
    name, k = kind.split("/")    # a codepoint with k of its bytes before the boundary, inside a token
    return edge - int(k) - 2, b"ab" + cps[name].encode() + b"cd"


KINDS = ["plain", "apostrophe", "long", "ends", "starts", "cp2/1", "cp3/1", "cp3/2", "cp4/1", "cp4/2", "cp4/3"]


def boundaries_doc(shift):
    """NBLK blocks with something at each of their boundaries: boundary b holds kind (b + shift) % 11"""
    placed = [crossing(KINDS[(b + shift) % len(KINDS)], b * BLK) for b in range(1, NBLK)]
    return layout(NBLK * BLK, placed, 500 + shift)


@pytest.fixture(scope="module")
def boundary_docs():
    # 11 documents of whole blocks (each starts on the grid): every kind at every boundary number once, so at
    # the boundaries inside a run and at those between two runs for every run length (11 and 8 are coprime)
    return [boundaries_doc(s) for s in range(len(KINDS))]


def test_tokens_across_run_blocks(ctx, boundary_docs):
    """a token crossing every block boundary inside a run and between two runs: short, with a deleted byte,
    longer than 64 bytes, with a 2-, 3- and 4-byte codepoint split every way; and the previous byte's class
    at a block's start (a word byte: one token; a space: a new one), also where the block before it was
    another wave's"""
    check_all_runs(ctx, boundary_docs)
    assert ctx.stats()["long_tokens"] > 0


def test_tokens_across_run_blocks_off_grid(ctx, boundary_docs):
    """the same documents 7 bytes off the grid: the crossings lie inside blocks, the blocks' edges elsewhere"""
    check_all_runs(ctx, [b"seven b"] + boundary_docs[:3], grids=(1,))


@pytest.mark.parametrize("run", RUNS)
def test_invalid_byte_in_interior_block(ctx, run):
    """one invalid byte in a block inside its document and inside a run: the oracle's offset"""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc, to_device
    at = 9 * BLK + 777
    first = b"fine text " * 8                      # 80 bytes: the second document starts on the grid
    bad = bytearray(filler(24 * BLK, 31))
    bad[at] = 0xFF
    with pytest.raises(UnicodeDecodeError) as u:    # the reference's read_to_string: the first invalid byte
        bytes(bad).decode("utf-8")
    assert u.value.start == at
    for grid in GRIDS:
        with knob(MRG_MAP_RUN=run, MRG_TEST_MAP_GRID=grid):
            t, off = to_device([first, bytes(bad)])
            ctx.job_begin(M.APP_WC, 3)
            ctx.set_input(t.data_ptr(), off)
            with pytest.raises(M.MrgError) as e:
                ctx.map()
            assert e.value.code == M.native.EUTF8 and "document 1 (id 1" in str(e.value), str(e.value)
            assert str(e.value).endswith(f"byte offset {at}"), str(e.value)
            good = [first, filler(3 * BLK, 5)]
            assert run_wc(ctx, good, 3) == O.wc(good, 3, O.FAST)        # the same context afterwards


# ---------------------------------------------------------------- runs and the pool

def sparse_nonascii(nbytes, seed):
    """words with a non-ASCII codepoint about every 190 bytes (English text with typographic quotes)"""
    import random
    rng = random.Random(seed)
    words = [b"the", b"of", b"and", b"kernel", b"wave", b"block", b"run", b"pool", b"a", b"mapping", b"don't",
             "’tis".encode(), "café".encode(), "naïve—so".encode(), "中文".encode()]
    weights = [12] * 11 + [1] * 4
    out = bytearray()
    while len(out) < nbytes:
        out += rng.choices(words, weights)[0] + b" "
    return bytes(out[:nbytes]).decode("utf-8", "ignore").encode()


# The jobs below run on a grid four times the resident one: 1024 workgroups own 256 tail regions each, some
# 200 MB of device blocks however small the input.  A closed context leaves its blocks in the library's
# process-wide device cache, which has no release call, and blocks that large change what later tests of the
# same process see of the allocator (tests/test_gpu_scale.py counts the allocations of a fresh context).  So these
# jobs run in ONE child process, started by a module fixture; it prints what it saw, and the tests here judge it.

def big_grid_jobs():
    """(the child process) the pool jobs and the tile-list jobs; one JSON line on stdout"""
    import json
    import torch
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc, to_device
    big_grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    # about 6 blocks per workgroup of the oversized grid, in documents of uneven sizes
    total = 6 * big_grid * BLK
    cuts = [0, total // 7 + 5, total // 2 + 11, total - 4099, total]
    docs = [sparse_nonascii(b - a, 70 + i) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    out = {"grid": big_grid, "pool": [], "tile_list": []}
    with M.Context(0) as ctx:
        exp = O.wc(docs, 3, O.FAST)
        for steal in (2, 1):  # half of the blocks in the pool; all of them (the static shares are empty)
            for run in RUNS:
                with knob(MRG_MAP_RUN=run, MRG_MAP_STEAL=steal, MRG_TEST_STEAL_MIN=0, MRG_TEST_MAP_GRID=big_grid):
                    got = run_wc(ctx, docs, 3)
                    st = ctx.stats()
                out["pool"].append({"steal": steal, "run": run, "equal": got == exp, "map_kind": st["map_kind"],
                                    "nonascii_tiles": st["nonascii_tiles"]})
        # invalid bytes in many pooled blocks of the second document
        doc = bytearray(docs[1])
        first_bad = None
        for at in range(5 * BLK + 300, len(doc) - 8, 3 * BLK + 17):
            if doc[at] < 0x80 and doc[at + 1] < 0x80 and doc[at - 1] < 0x80:
                doc[at] = 0xFF
                first_bad = at if first_bad is None else first_bad
        try:
            bytes(doc).decode("utf-8")
            ref_bad = None
        except UnicodeDecodeError as u:   # the reference's read_to_string: the first invalid byte
            ref_bad = u.start
        bad_docs = [docs[0], bytes(doc)]
        for run in (1, 8):
            for kwords in (1, 0):
                env = dict(MRG_MAP_RUN=run, MRG_MAP_STEAL=2, MRG_TEST_STEAL_MIN=0, MRG_TEST_MAP_GRID=big_grid // 8)
                if kwords:
                    env["MRG_TEST_KWORDS"] = kwords
                with knob(**env):
                    t, off = to_device(bad_docs)
                    ctx.job_begin(M.APP_WC, 3)
                    ctx.set_input(t.data_ptr(), off)
                    code, msg = 0, ""
                    try:
                        ctx.map()
                    except M.MrgError as e:
                        code, msg = e.code, str(e)
                    out["tile_list"].append({"run": run, "kwords": kwords, "code": code, "msg": msg,
                                             "eutf8": M.native.EUTF8, "launches": ctx.stats()["map_launches"],
                                             "first_bad": first_bad, "ref_bad": ref_bad})
    print("RESULT " + json.dumps(out), flush=True)


@pytest.fixture(scope="module")
def big_grid_results():
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


def test_runs_and_pool(big_grid_results):
    """most blocks from the pool (half of them, and all of them), on a grid four times the resident one, over
    text with sparse non-ASCII codepoints: the job gives the oracle's output with every run length"""
    jobs = big_grid_results["pool"]
    assert [(j["steal"], j["run"]) for j in jobs] == [(s, r) for s in (2, 1) for r in RUNS]
    for j in jobs:
        assert j["equal"] and j["map_kind"] == 0 and j["nonascii_tiles"] > 0, j


def test_tile_list_is_bounded(big_grid_results):
    """invalid UTF-8 in many pooled blocks with a tile list of ONE entry per workgroup (MRG_TEST_KWORDS): the
    appends past the list are counted, not written; the launch is rerun with full lists and reports the first
    invalid byte, as the job with full lists does at once"""
    jobs = big_grid_results["tile_list"]
    assert [(j["run"], j["kwords"]) for j in jobs] == [(r, k) for r in (1, 8) for k in (1, 0)]
    for j in jobs:
        assert j["first_bad"] is not None and j["first_bad"] == j["ref_bad"], j
        assert j["code"] == j["eutf8"] and "document 1 (id 1" in j["msg"], j
        assert j["msg"].endswith(f"byte offset {j['first_bad']}"), j
        if j["kwords"]:
            assert j["launches"] >= 2, j


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        sys.path.insert(0, d)
    big_grid_jobs()
