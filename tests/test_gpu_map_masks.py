"""GPU tests: the token round of k_map with its lane conditions kept as lane masks, and
what a block inside a run takes from its neighbours -- the halo behind it, the 16 bytes before it -- at the
smallest shapes where either can go wrong.

Every expectation is the C oracle's (oracle_lib) over inputs built here from fixed seeds: output bytes,
`tokens` and (wc) `distinct_keys`, exactly.  Every text runs with MRG_MAP_RUN = 1, 2, 4 and 8, on grids of 1 and
3 workgroups and on four times the resident grid (the pool), with the packed and the 64-bit tail cursors
(MRG_TEST_TAIL64) and both table sizes, as wc and as the indexer, and through the wide map per run length and
grid: tests/test_gpu_map_neighbours.py's job list (run_case), 108 jobs per text.  No document is longer than
8 * 2048 + 1 bytes (nine blocks).

The jobs run in ONE child process, started by a module fixture (as in tests/test_gpu_map_runs.py: the oversized
grid and the one-record regions leave large blocks in the library's process-wide device cache).

Invalid UTF-8 is a documented input with a defined error return; nothing here is meant to fault the device."""
import pytest

from test_gpu_map_block_queue import BLK, filler, knob, layout
from test_gpu_map_neighbours import KEEP, LDS_CAPS, N_JOBS, RUNS, R, Case, judge, run_case, run_invalid
from test_gpu_map_tail import word

pytestmark = pytest.mark.gpu

DOC9 = 8 * BLK + 1          # the longest document here: nine blocks
CPS = ("é", "中", "\U00010400")


def on_grid(docs):
    """each document on the 16-byte grid (a short filler document pads the one before it), so that a document's
    blocks start at multiples of BLK of its own bytes"""
    out = []
    for i, d in enumerate(docs):
        out.append(d)
        if len(d) % 16:
            out.append(filler(-len(d) % 16, 9900 + i))
    return out


# ---------------------------------------------------------------- the halo from the next set

LONG40 = bytes(97 + (k * 5) % 26 for k in range(40))
LONG70 = bytes(97 + (k * 3) % 26 for k in range(70))
LONG90 = bytes(97 + (k * 7) % 26 for k in range(90))   # past the first halo segment and the halo: the walker


def ascii_seams():
    """(bytes before the boundary, token)"""
    return [(5, b"ended"), (0, b"started"), (1, b"xy"), (5, b"twelvebytess"), (7, b"crossingboundary"),
            (9, LONG40[:17]), (20, LONG40[:29]), (1, LONG40), (3, LONG70), (2, LONG90), (5, b"rock'"), (4, b"rock'n"),
            (0, b"'tis"), (1, b"'tis")]


def nonascii_seams():
    out = []
    for cp in CPS:
        e = cp.encode()
        out += [(k + 2, b"ab" + e + b"cd") for k in range(1, len(e))]      # split every way, inside a token
    out += [(1, "é".encode()), (2, "\U00010400".encode())]                   # split, alone between spaces
    out += [(-2, b"h" + "中".encode() + b"x")]                               # only in the halo's first segment
    out += [(-20, "é".encode() + b"far"), (-57, b"w" + "\U00010400".encode())]   # only in halo bytes 16 .. 63
    return out


def seam_docs(seams, seed):
    """documents of nine blocks (8 * BLK + 1 bytes): document k has seams[(b + k) % n] at boundary b, so every
    kind meets every boundary 1 .. 8, and with every run length some block is a run's first, inner and last"""
    n = len(seams)
    docs = []
    for k in range(n):
        placed = []
        for b in range(1, 9):
            before, tok = seams[(b + k) % n]
            if b == 8:        # (the ninth block is one byte, a space: a token ends on the eighth's last byte)
                before, tok = 5, b"ended"
            placed.append((b * BLK - before, tok))
        docs.append(layout(DOC9, placed, seed + k))
    return on_grid(docs)


# ---------------------------------------------------------------- the 16 bytes before from the window

def dense_block():
    """more than 320 token starts: the block is drained a range of segments at a time"""
    return bytes(b for k in range(BLK // 2) for b in (97 + k % 26, 32))


def nonascii_block(seed):
    blk = bytearray(filler(BLK, seed))
    for at in range(300, 1700, 100):      # codepoints well inside the block, each between two spaces
        e = CPS[(at // 100) % 3].encode()
        blk[at - 1:at + len(e) + 1] = b" " + e + b" "
    return bytes(blk)


def before_docs():
    """eight-block documents in which an ASCII block follows, and is followed by, a dense block and a non-ASCII
    block, with a token ending on, starting on and crossing each boundary"""
    kinds = "ADANADNA", "DANADNAA", "NADANAAD"
    seams = [(5, b"ended"), (0, b"started"), (7, b"crossingboundary"), (5, b"twelvebytess"), (1, LONG40[:17])]
    docs = []
    for k, pat in enumerate(kinds):
        doc = bytearray()
        for b, c in enumerate(pat):
            doc += {"A": filler(BLK, 9800 + 8 * k + b), "D": dense_block(), "N": nonascii_block(9850 + 8 * k + b)}[c]
        for b in range(1, 8):
            before, tok = seams[(b + k) % len(seams)]
            at = b * BLK - before
            doc[at - 1:at + len(tok) + 1] = b" " + tok + b" "
        docs.append(bytes(doc))
    for d in docs:
        d.decode()      # still valid UTF-8
    return docs


# ---------------------------------------------------------------- edges keep their load

def edge_docs():
    docs = []
    for rot in range(3):          # documents of 1, 2 and 3 blocks back to back
        for k in range(3):
            docs.append(filler((1, 2, 3)[(k + rot) % 3] * BLK, 9700 + 3 * rot + k))
    docs.append(filler(BLK - 9, 9720))
    docs.append(b"nine byt ")     # nine bytes directly before a block boundary
    assert sum(map(len, docs)) % BLK == 0
    for i, e in enumerate((1, 15, 16, 17, 63, 64, 65)):      # a document ending e bytes into a block
        docs += on_grid([filler((1 + i % 3) * BLK + e, 9730 + i)])
    docs.append(filler(2 * BLK, 9740))     # the last document ends on the buffer's last byte, and on a block's
    return docs


def invalid_cases():
    """(name, documents, document of the bad byte): a truncated lead and a stray continuation byte at a boundary
    inside a run (last byte, first byte, the halo's first segment, halo bytes 16 .. 63), and in the middle of a
    block with ASCII blocks on either side (the block is deferred; its neighbours are not)"""
    cases = []
    spots = {"last byte": 2 * BLK - 1, "first byte": 2 * BLK, "halo": 2 * BLK + 9, "halo 16..63": 6 * BLK + 40,
             "inner block": 3 * BLK + 1000, "inner block of 8": 5 * BLK + 77}
    for what, byte in (("truncated lead", 0xE4), ("stray continuation", 0x9F)):
        for where, at in spots.items():
            doc = bytearray(layout(DOC9, [(at - 3, b"abc def")], 9600))
            doc[at] = byte
            cases.append((f"{what}, {where}", [b"fine text " * 8, bytes(doc)], 1))
    return cases


# ---------------------------------------------------------------- masks in the round

HOT = [b"the", b"count", b"kernel", b"mapping", b"of", b"word", b"doorkeep", b"a"]


def kind_tokens(kind, salt):
    """64 tokens of one kind; `salt` makes the unique ones unique across the text"""
    if kind == "hit":       # few words, repeated: in the table after their first sightings
        return [HOT[(j + salt) % len(HOT)] for j in range(64)]
    if kind == "miss":      # seen once: the doorkeeper sends them to the tail, 12-byte records
        return [word(64 * salt + j, 5 + j % 8) for j in range(64)]
    if kind == "w16":       # 13 .. 16 bytes, seen once: the cold block's 16-byte records
        return [word(64 * salt + j, 13 + j % 4) for j in range(64)]
    if kind == "slow":      # 17 .. 20 key bytes: deferred by the round, a long-token record
        return [word(64 * salt + j, 17 + j % 4) for j in range(64)]
    if kind == "fast":
        return [word(j % 16, 3) for j in range(64)]
    # two deleted runs inside the token: squeezed after the selectors; 12 and 13 key bytes
    n = {"gap12": 12, "gap13": 13}[kind]
    out = []
    for j in range(64):
        w = word(64 * (salt % 2) + j, n)    # (salt % 2: half of them come back, so some hit)
        out.append(w[:1] + b"'" + w[1:2] + b"'" + w[2:])
    return out


PAIRS = [("hit", "miss"), ("miss", "hit"), ("miss", "w16"), ("w16", "miss"), ("slow", "fast"), ("fast", "slow"),
         ("gap12", "gap13"), ("gap13", "gap12"), ("hit", "w16"), ("gap13", "miss")]


def pair_block(a, b, salt):
    """one block of exactly 128 tokens: its one round gives every lane a token of kind a (queue entry q) and one
    of kind b (entry q + 64)"""
    body = b" ".join(kind_tokens(a, 2 * salt) + kind_tokens(b, 2 * salt + 1)) + b" "
    assert len(body) <= BLK and len(body.split()) == 128, (a, b, len(body))
    return body + b" " * (BLK - len(body))


def round_docs():
    """every pair of PAIRS as one block, the list three times over (the hot words and half of the multi-gap keys
    are in the table from the second time on), five blocks per document"""
    blocks = [pair_block(a, b, len(PAIRS) * rep + i) for rep in range(3) for i, (a, b) in enumerate(PAIRS)]
    return [b"".join(blocks[i:i + 5]) for i in range(0, len(blocks), 5)]


def fill_docs():
    """6000 distinct words, each four times: groups of 64 words written four times in a row, so that a key's
    sightings are 64 queue entries apart -- the two tokens of one lane in a round.  More keys than either table
    holds: the table fills and the claim side of the round turns off in the middle of the job, and before that
    the doorkeeper's sighting, the claim and the first hit of a key fall into the same rounds"""
    words = [word(j, 3 + j % 7) for j in range(6000)]
    toks = []
    for g in range(0, len(words), 64):
        toks += words[g:g + 64] * 4
    docs, cur = [], bytearray()
    for t in toks:
        if len(cur) + len(t) + 1 > DOC9 - 16:
            docs.append(bytes(cur))
            cur = bytearray()
        cur += t + b" "
    docs.append(bytes(cur))
    return on_grid(docs)


# ---------------------------------------------------------------- the child process

def run_small_regions(ctxs, case):
    """regions of 1 and 2 records: nearly every append finds its region full, so the rare block of the round
    (overflow lists, the cold append) runs beside the mask tests"""
    import mapreduce_rust_amd as M
    from gpu_util import run_wc
    jobs = []
    for cap in (1, 2):
        for grid in (1, 3):
            for t64 in (None, 1):
                env = {"MRG_TEST_TAIL_CAP": cap, "MRG_TEST_OVF_CAP": 1 << 20, "MRG_TEST_MAP_GRID": grid}
                if t64 is not None:
                    env["MRG_TEST_TAIL64"] = t64
                for lds in LDS_CAPS:
                    for app in ("wc", "indexer"):
                        with knob(**env):
                            if app == "wc":
                                equal = run_wc(ctxs[lds], case.docs, R) == case.exp_wc
                            else:
                                equal = run_wc(ctxs[lds], case.docs, R, app=M.APP_INDEXER, names=case.names) == case.exp_ix
                            st = ctxs[lds].stats()
                        jobs.append({"tag": f"{app}, regions of {cap}, grid {grid}, tail64 {t64}, table {lds}", "app": app,
                                     "equal": equal, **{k: st[k] for k in KEEP}})
    return {"facts": case.facts, "jobs": jobs}


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
    out = {}
    texts = (("halo_ascii", seam_docs(ascii_seams(), 9000)), ("halo_nonascii", seam_docs(nonascii_seams(), 9100)),
             ("before", before_docs()), ("edges", edge_docs()), ("round", round_docs()), ("fill", fill_docs()))
    for name, docs in texts:
        assert max(map(len, docs)) <= DOC9, name
        case = Case(docs)
        out[name] = run_case(ctxs, case, big_grid)
        if name in ("round", "fill"):
            out[name + "_small"] = run_small_regions(ctxs, case)
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

def judge_small(r):
    facts = r["facts"]
    assert len(r["jobs"]) == 2 * 2 * 2 * len(LDS_CAPS) * 2
    for j in r["jobs"]:
        assert j["equal"], j
        assert j["map_kind"] == 0, j
        assert j["tokens"] == facts["tokens"], (j, facts)
        if j["app"] == "wc":
            assert j["distinct_keys"] == facts["distinct"], (j, facts)


def test_halo_ascii_tokens_at_every_boundary_of_nine_blocks(results):
    """nine-block documents; at every boundary a token ending on the last byte, starting on the first, tokens of
    2, 12, 16, 17, 29, 40 and 70 bytes across it, one of 90 bytes (past the halo: the codepoint walker), and an
    apostrophe on either side"""
    assert len(ascii_seams()) == 14
    judge(results["halo_ascii"])


def test_halo_codepoints_at_every_boundary_of_nine_blocks(results):
    """2-, 3- and 4-byte codepoints split every way by every boundary, a codepoint only in the halo's first
    segment and only in halo bytes 16 .. 63"""
    judge(results["halo_nonascii"])


def test_bytes_before_a_block_after_dense_and_nonascii_blocks(results):
    """an ASCII block after, and before, a block of 1024 token starts (drained by ranges) and a non-ASCII block,
    tokens ending on, starting on and crossing each boundary"""
    assert len(dense_block().split()) == BLK // 2 > 320
    judge(results["before"])


def test_document_edges(results):
    """documents of 1, 2 and 3 blocks back to back, a 9-byte document directly before a block boundary, documents
    ending 1, 15, 16, 17, 63, 64 and 65 bytes into a block, the last one ending on the buffer's last byte"""
    judge(results["edges"])


def test_invalid_utf8_inside_a_run(results):
    """a truncated lead and a stray continuation byte on the last and first byte of a boundary inside a run, in
    the halo's first segment and in halo bytes 16 .. 63, and in a block between two ASCII blocks: the oracle's
    first invalid byte, for every run length and grid"""
    cases = results["invalid"]
    assert len(cases) == 12
    for c in cases:
        assert c["oracle_rc"] != 0, c["name"]
        assert len(c["jobs"]) == 3 * len(RUNS) * 2
        for j in c["jobs"]:
            assert j["code"] == c["eutf8"] and "document 1 (id 1" in j["msg"], (c["name"], j)
            assert j["msg"].endswith(f"byte offset {c['oracle_at']}"), (c["name"], c["oracle_at"], j)
        assert c["after"], c["name"]


def test_two_kinds_of_token_per_lane_in_one_round(results):
    """blocks of exactly 128 tokens, 64 of one kind and 64 of another, either order: a hit and a miss, a miss and
    a 13..16-byte key, a slow and a fast token, multi-gap keys of 12 and of 13 bytes after squeezing"""
    for a, b in PAIRS:
        assert (b, a) in PAIRS or (a, b) in (("hit", "w16"), ("gap13", "miss"))
    sq = [t.replace(b"'", b"") for t in kind_tokens("gap12", 0) + kind_tokens("gap13", 0)]
    assert {len(t) for t in sq} == {12, 13}
    assert len(results["round"]["jobs"]) == N_JOBS
    judge(results["round"])


def test_table_fills_in_the_middle_of_the_job(results):
    """6000 distinct keys, each four times, 64 queue entries apart: sighting, claim and hit of a key in the same
    rounds, and the claim side turning off when the table (4096 or 2048 slots) is full"""
    r = results["fill"]
    assert r["facts"]["distinct"] >= 6000 and r["facts"]["tokens"] >= 4 * 6000     # (and the grid fillers' words)
    judge(r)


@pytest.mark.parametrize("name", ["round_small", "fill_small"])
def test_regions_of_one_and_two_records(results, name):
    """the same two texts with tail regions of 1 and 2 records: the round's rare block on nearly every append"""
    judge_small(results[name])


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for d in (os.path.join(root, "tests", "golden"), os.path.join(root, "tests"), root):
        sys.path.insert(0, d)
    child_jobs()
