"""GPU tests: what a block of k_map takes from its neighbours in a run -- the record of the block the wave is at
(advanced in place to the next 2 KiB of the same document, looked up in full when the run leaves the document),
the bytes before a block and the halo after it -- at the smallest shapes where that can go wrong.

Every expectation is the C oracle's (oracle_lib) over inputs built here from fixed seeds.  Every text runs with
MRG_MAP_RUN = 1, 2, 4 and 8, on grids of 1 and 3 workgroups and on one grid larger than the resident one (the
static shares are then a block or two and the pool hands out blocks), with the packed and the 64-bit tail
cursors (MRG_TEST_TAIL64) and both table sizes (MRG_LDS_CAP), as wc (the block queue) and the indexer (per
tile); the wide map, which has one code object and no table, with every run length and grid.  For every job
the output bytes, `tokens` and `distinct_keys` are compared.

The jobs run in ONE child process, started by a module fixture; it prints what it saw and the tests here judge
it (as in tests/test_gpu_map_runs.py: the oversized grid leaves large blocks in the library's process-wide
device cache, and tests/test_gpu_scale.py counts the allocations of a fresh context of the same process).

Invalid UTF-8 is a documented input with a defined error return; nothing here is meant to fault the device."""
import pytest

from test_gpu_map_block_queue import BLK, filler, knob, layout

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 4, 8)
TAIL64 = (None, 1)
LDS_CAPS = (4096, 2048)
R = 3

# ---------------------------------------------------------------- inputs (host only, fixed seeds)

DOC_LENGTHS = (2047, 2048, 2049, 2048 + 63, 2048 + 64, 2048 + 65, 4 * 2048 - 1, 4 * 2048, 4 * 2048 + 1,
               4 * 2048 + 63, 4 * 2048 + 64, 4 * 2048 + 65, 8 * 2048 + 1)


def length_docs():
    """one document per length around a block's, the halo's and a run's edges, each on the 16-byte grid (a
    filler document pads the one before it to the grid), so its blocks are the job's"""
    docs = []
    for i, n in enumerate(DOC_LENGTHS):
        docs.append(filler(n, 9100 + i))
        pad = -n % 16
        if pad:
            docs.append(filler(pad, 9200 + i))
    return docs


def leaving_docs():
    """documents of 1, 3 and 5 blocks back to back, three times over in rotated orders: a run of 2, 4 or 8 leaves
    its document after 1, 2 and 3 blocks; then a document of fewer than 16 bytes directly before a block
    boundary (it shares its 16-byte vector with the end of the document before it)"""
    docs = []
    for rot in range(3):
        for k in range(3):
            docs.append(filler((1, 3, 5)[(k + rot) % 3] * BLK, 9300 + 3 * rot + k))
    docs.append(filler(BLK - 9, 9400))
    docs.append(b"nine byt ")           # bytes [BLK - 9, BLK) of its block
    assert sum(map(len, docs)) % BLK == 0
    docs.append(filler(2 * BLK + 5, 9401))
    return docs


LONG40 = bytes(97 + (k * 5) % 26 for k in range(40))    # 17..40 bytes: the slow path through the masks
LONG70 = bytes(97 + (k * 3) % 26 for k in range(70))    # longer than the halo: the exact walker


def seam_tokens():
    """(bytes before the boundary, token): every way a token meets or crosses a block boundary"""
    out = [(5, b"ended"), (0, b"started")]                       # ends on the last byte; starts on the first
    out += [(k, b"crossingboundary") for k in range(1, 16)]      # a 16-byte key, 1..15 bytes on either side
    out += [(1, b"xy"), (2, b"xyz"), (7, b"shortkey")]            # short keys, 1 byte on either side too
    out += [(k, b"twelvebytes!"[:11] + b"s") for k in (1, 6, 11)]  # a 12-byte key
    out += [(9, LONG40[:17]), (20, LONG40[:29]), (1, LONG40), (39, LONG40)]
    out += [(3, LONG70), (66, LONG70)]
    out += [(3, b"don't"), (4, b"don't"), (1, b"'tis"), (0, b"'tis"), (5, b"rock'"), (4, b"rock'n")]
    return out


def seams_doc(shift):
    """a document of whole blocks with seam_tokens()[(b + shift) % n] at boundary b; a space on both sides of each,
    so a boundary is preceded by a word byte (a token crossing or ending there) or by a non-word byte"""
    toks = seam_tokens()
    nblk = len(toks) + 1
    placed = []
    for b in range(1, nblk):
        before, tok = toks[(b + shift) % len(toks)]
        placed.append((b * BLK - before, tok))
    return layout(nblk * BLK, placed, 9500 + shift)


def seam_docs():
    # 35 boundaries per document, three shifts: a kind meets boundaries inside a run and between runs
    return [seams_doc(s) for s in (0, 1, 5)]


CPS = ("é", "中", "\U00010400")


def nonascii_docs():
    """2-, 3- and 4-byte codepoints straddling a block boundary at every split, inside a token and alone between
    spaces; a block whose only non-ASCII byte lies in the 16 bytes before it, and one whose only non-ASCII bytes
    lie in the first halo segment after it -- every other block of these documents is ASCII"""
    placed = []
    b = 1
    for cp in CPS:
        e = cp.encode()
        for k in range(1, len(e)):
            placed.append((b * BLK - k - 2, b"ab" + e + b"cd"))
            b += 1
            placed.append((b * BLK - k, e))
            b += 1
    first = layout(b * BLK, placed, 9600)
    # groups of three blocks: block 3g + 1 is ASCII with a codepoint in the 16 bytes before it (ending two bytes
    # before the boundary, or on byte -1), block 3g + 2 is ASCII with one in its first halo segment
    placed = []
    for g in range(2 * len(CPS)):
        e = CPS[g % len(CPS)].encode()
        edge = (3 * g + 1) * BLK
        placed.append((edge - len(e) - 6, b"w" + e + b"tail") if g < len(CPS) else (edge - len(e), e))
        placed.append(((3 * g + 3) * BLK + 2, b"h" + e + b"x"))
    second = layout((3 * 2 * len(CPS) + 1) * BLK, placed, 9601)
    for g in range(2 * len(CPS)):
        for blk in (3 * g + 1, 3 * g + 2):
            assert max(second[blk * BLK:(blk + 1) * BLK]) < 0x80
        assert max(second[(3 * g + 1) * BLK - 16:(3 * g + 1) * BLK]) >= 0x80
        assert max(second[(3 * g + 3) * BLK:(3 * g + 3) * BLK + 16]) >= 0x80
    return [first, second]


def invalid_cases():
    """(name, documents, document of the bad byte): a truncated lead and a stray continuation byte at a seam"""
    cases = []
    spots = {"last byte": 4 * BLK - 1, "first byte": 4 * BLK, "before, 16": 4 * BLK - 7, "halo": 4 * BLK + 9}
    for what, byte in (("truncated lead", 0xE4), ("stray continuation", 0x9F)):
        for where, at in spots.items():
            doc = bytearray(layout(9 * BLK, [(at - 3, b"abc def")], 9700))
            doc[at] = byte
            cases.append((f"{what}, {where}", [b"fine text " * 8, bytes(doc)], 1))
    return cases


# ---------------------------------------------------------------- the child process

KEEP = ("map_kind", "tokens", "distinct_keys")


class Case:
    def __init__(self, docs):
        import oracle_lib as O
        assert sum(map(len, docs)) <= 600 << 10
        self.docs = docs
        self.names = [f"d/{i}.txt" for i in range(len(docs))]
        toks = [t for d in docs for t in O.tokens(d) if t]
        self.facts = {"tokens": len(toks), "distinct": len(set(toks)), "bytes": sum(map(len, docs))}
        self.exp_wc = O.wc(docs, R, O.FAST)
        self.exp_ix = O.indexer(docs, self.names, R)


def grids_of(big_grid):
    # (the pool: as tests/test_gpu_map_runs.py sets it)
    return [("grid 1", {"MRG_TEST_MAP_GRID": 1}), ("grid 3", {"MRG_TEST_MAP_GRID": 3}),
            ("pool", {"MRG_TEST_MAP_GRID": big_grid, "MRG_MAP_STEAL": 2, "MRG_TEST_STEAL_MIN": 0})]


def run_case(ctxs, case, big_grid):
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    jobs = []
    for gname, genv in grids_of(big_grid):
        for run in RUNS:
            for t64 in TAIL64:
                env = dict(genv, MRG_MAP_RUN=run)
                if t64 is not None:
                    env["MRG_TEST_TAIL64"] = t64
                for lds in LDS_CAPS:
                    ctx = ctxs[lds]
                    for app in ("wc", "indexer"):
                        with knob(**env):
                            if app == "wc":
                                equal = run_wc(ctx, case.docs, R) == case.exp_wc
                            else:
                                equal = run_wc(ctx, case.docs, R, app=M.APP_INDEXER, names=case.names) == case.exp_ix
                            st = ctx.stats()
                        jobs.append({"tag": f"{app}, {gname}, run {run}, tail64 {t64}, table {lds}", "app": app,
                                     "equal": equal, **{k: st[k] for k in KEEP}})
            with knob(MRG_WIDE_MAP=1, MRG_MAP_RUN=run, **genv):
                equal = run_wc(ctxs[4096], case.docs, R) == case.exp_wc
                st = ctxs[4096].stats()
            jobs.append({"tag": f"wide, {gname}, run {run}", "app": "wide", "equal": equal, **{k: st[k] for k in KEEP}})
    return {"facts": case.facts, "jobs": jobs}


def run_invalid(ctx, name, docs, bad_doc, big_grid):
    """the error of every run length and grid, and the oracle's first invalid byte of that document"""
    import ctypes
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc, to_device
    pos = ctypes.c_size_t()
    rc = O.lib().oracle_validate_utf8(docs[bad_doc], len(docs[bad_doc]), ctypes.byref(pos))
    out = {"name": name, "oracle_rc": rc, "oracle_at": pos.value, "eutf8": M.native.EUTF8, "jobs": []}
    for gname, genv in grids_of(big_grid):
        for run in RUNS:
            for app in (M.APP_WC, M.APP_INDEXER):
                with knob(MRG_MAP_RUN=run, **genv):
                    t, off = to_device(docs)
                    ctx.job_begin(app, R)
                    if app == M.APP_INDEXER:
                        ctx.set_doc_names([f"d/{i}.txt" for i in range(len(docs))])
                    ctx.set_input(t.data_ptr(), off)
                    code, msg = 0, ""
                    try:
                        ctx.map()
                    except M.MrgError as e:
                        code, msg = e.code, str(e)
                out["jobs"].append({"tag": f"app {app}, {gname}, run {run}", "code": code, "msg": msg})
    good = [docs[0], filler(3 * BLK, 5)]
    out["after"] = run_wc(ctx, good, R) == O.wc(good, R, O.FAST)   # the same context afterwards
    return out


def child_jobs():
    """(the child process) every job of this module; one JSON line on stdout"""
    import json
    import torch
    import mapreduce_rust_amd as M
    big_grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    ctxs = {}
    for lds in LDS_CAPS:      # MRG_LDS_CAP is read when a context is made
        with knob(MRG_LDS_CAP=lds):
            ctxs[lds] = M.Context(0)
    out = {"grid": big_grid}
    for name, docs in (("lengths", length_docs()), ("leaving", leaving_docs()), ("seams", seam_docs()),
                       ("nonascii", nonascii_docs())):
        out[name] = run_case(ctxs, Case(docs), big_grid)
    out["invalid"] = [run_invalid(ctxs[4096], name, docs, d, big_grid) for name, docs, d in invalid_cases()]
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

N_JOBS = 3 * len(RUNS) * (len(TAIL64) * len(LDS_CAPS) * 2 + 1)


def judge(r):
    """every job gave the oracle's bytes and counted the tokens and keys the text holds; wc and the indexer ran
    the LDS-combine map, the forced wide map the wide one"""
    facts = r["facts"]
    assert len(r["jobs"]) == N_JOBS, (len(r["jobs"]), N_JOBS)
    for j in r["jobs"]:
        assert j["equal"], j
        assert j["map_kind"] == (1 if j["app"] == "wide" else 0), j
        assert j["tokens"] == facts["tokens"], (j, facts)
        if j["app"] == "wc":     # (the indexer's keys are (word, document) pairs; the wide map has no table)
            assert j["distinct_keys"] == facts["distinct"], (j, facts)


def test_document_lengths_at_block_halo_and_run_edges(results):
    """documents of 2047 .. 8 * 2048 + 1 bytes: the last block of each is clipped at, just before and just past a
    block's end, the halo's end and the end of a run of 4"""
    judge(results["lengths"])


def test_runs_leaving_their_document(results):
    """documents of 1, 3 and 5 blocks back to back (a run leaves its document after 1, 2 and 3 blocks), and a
    document of 9 bytes directly before a block boundary"""
    judge(results["leaving"])


def test_tokens_at_every_boundary_kind(results):
    """a token ending on a block's last byte, starting on its first, a 16-byte key crossing with 1..15 bytes on
    either side, short keys, tokens of 17, 29 and 40 bytes (the masks' slow path), of 70 bytes (the walker),
    and an apostrophe as the last byte before and the first byte after the boundary"""
    r = results["seams"]
    assert r["facts"]["bytes"] == 3 * (len(seam_tokens()) + 1) * BLK
    judge(r)


def test_nonascii_at_the_seams(results):
    """2-, 3- and 4-byte codepoints split every way by a block boundary; a non-ASCII byte only in the 16 bytes
    before a block and only in the first halo segment after one, the block itself ASCII"""
    judge(results["nonascii"])


def test_invalid_utf8_at_the_seams(results):
    """a truncated lead and a stray continuation byte on a block's last and first byte, in the 16 bytes before
    it and in its first halo segment: the oracle's first invalid byte, for every run length and grid"""
    cases = results["invalid"]
    assert len(cases) == 8
    for c in cases:
        assert c["oracle_rc"] != 0, c["name"]
        assert len(c["jobs"]) == 3 * len(RUNS) * 2
        for j in c["jobs"]:
            assert j["code"] == c["eutf8"] and "document 1 (id 1" in j["msg"], (c["name"], j)
            assert j["msg"].endswith(f"byte offset {c['oracle_at']}"), (c["name"], c["oracle_at"], j)
        assert c["after"], c["name"]


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        sys.path.insert(0, d)
    child_jobs()
