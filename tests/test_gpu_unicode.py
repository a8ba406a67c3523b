"""GPU tests: every Unicode scalar and every UTF-8 acceptance edge through the device tokenizers.

Two decisions per codepoint make every output of the library: its class (\\w, White_Space or deleted) and
whether its bytes are valid UTF-8.  They are made in k_map's register class fix (per-lane loop, compacted
decode, the byte before the block, the halo segment), uni_class (LDS copy / constant table), the exact
walker (walk_token / generic_tile), the indexer and wide instantiations of k_map, k_text (mrg_map_text) and
k_encode with mrg_vocab_from_text.  Each is fed here

  * the sweep of uclass_util.sweep(): one unit HEX + c + "z " per scalar c, whose expected tokens follow from
    the class fixture tests/golden/uclass_runs.json by construction (jobs with one partition) or from the C
    oracle (partitioned jobs; tests/test_uclass_cpu.py ties the oracle to the fixture);
  * a deterministic position sweep of nine codepoints over every lane, tile seam and halo slot of a block;
  * the matrix uclass_util.utf8_matrix() of valid and invalid 4-byte strings: the invalid ones must fail
    with MRG_EUTF8 naming the document and the byte offset that Python's strict decoder reports
    (UnicodeDecodeError.start, the valid_up_to of the reference's from_utf8).

Invalid UTF-8 is a documented input with a defined error return; nothing here is meant to fault the device.
No expectation comes from the library, `regex` is not imported and nothing outside the repository is read."""
import contextlib
import os
import random

import numpy as np
import pytest

import uclass_util as U
from vocab_util import (cat, check, count_lines, decode, encode, expected, expected_text, rank_of, ranked)

pytestmark = pytest.mark.gpu

NTOKENS = 1_112_089
FINE = b"fine text"
GOOD_DOCS = [b"fine text " * 40, "café naïve ’tis 中文　\U00010400x \U0001F600y\u0085z ".encode() * 90]


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def full():
    """The full sweep, built once: 17 documents, their tokens, the sorted (key, count) items."""
    docs, toks = U.full_sweep()
    return docs, toks, U.count_items(toks)


@pytest.fixture(scope="module")
def boundary():
    return list(U.boundary_set())


@contextlib.contextmanager
def knob(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_lines(got, exp_lines, what):
    """got == the lines; on a difference name the first differing line (its hex names the sweep unit)"""
    exp = exp_lines if isinstance(exp_lines, bytes) else b"".join(exp_lines)
    if got == exp:
        return
    g = got.split(b"\n")
    e = exp.split(b"\n")
    i = next((i for i in range(min(len(g), len(e))) if g[i] != e[i]), min(len(g), len(e)))
    raise AssertionError(f"{what}: line {i}: got {g[i:i + 2]!r}, expected {e[i:i + 2]!r} ({len(g)} / {len(e)} lines)")


def items_lines(items):
    return [k + b" %d\n" % n for k, n in items]


def job(ctx, ptr, off, R, flags=0, app=None, names=None):
    import mapreduce_rust_amd as M
    ctx.job_begin(M.APP_WC if app is None else app, R, flags)
    if names is not None:
        ctx.set_doc_names(names)
    ctx.set_input(ptr, off)
    ctx.map()
    ctx.reduce()
    return ctx.outputs()


# ================================================================ a. the full sweep, short keys

def test_full_sweep_one_partition(ctx, full):
    import mapreduce_rust_amd as M
    import torch
    from gpu_util import to_device
    docs, toks, items = full
    lines = items_lines(items)
    t, off = to_device(docs)
    outs = job(ctx, t.data_ptr(), off, 1, M.FLAG_NO_COMPAT_DROP_LAST)
    fin = ctx.final()
    st = ctx.stats()
    torch.cuda.synchronize()
    del t
    same_lines(outs[0], lines, "mr-0.txt")
    same_lines(fin, lines, "final.txt")
    assert st["tokens"] == NTOKENS == sum(map(len, toks)) and st["nonascii_tiles"] > 0, st
    assert st["long_tokens"] == 0, st


def test_full_sweep_seven_partitions(ctx, full):
    """SipHash-1-3 partitioning over keys that hold every byte pattern of valid UTF-8."""
    import oracle_lib as O
    from gpu_util import run_wc
    docs = full[0]
    got = run_wc(ctx, docs, 7)
    exp = O.wc(docs, 7, O.FAST)
    for r in range(7):
        same_lines(got[r], exp[r], f"mr-{r}.txt")


# ================================================================ b. the boundary set, other instantiations

def test_boundary_long_keys(ctx, boundary):
    """prefix "L" * 14: the keys are longer than 16 bytes and go through walk_token -- all but the "z" after
    each S scalar and the keys of the few scalars below U+0100 whose hex is one or two digits, so the
    expected long_tokens is counted from the constructed tokens, not taken as the token count."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    doc, toks = U.sweep(boundary, b"L" * 14)
    n_long = sum(len(t) > 16 for t in toks)
    assert len(toks) - 40 < n_long < len(toks)
    outs = run_wc(ctx, [doc], 1, flags=M.FLAG_NO_COMPAT_DROP_LAST)
    st = ctx.stats()
    same_lines(outs[0], U.lines([toks]), "mr-0.txt")
    assert st["tokens"] == len(toks) and st["long_tokens"] == n_long, st
    assert run_wc(ctx, [doc], 5) == O.wc([doc], 5, O.FAST)
    assert ctx.stats()["long_tokens"] == n_long


def test_boundary_indexer(ctx, boundary):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    docs = [U.sweep(part)[0] for part in U.chunks(boundary, 3)]
    names = ["plane/a.txt", "plane/b.txt", "plane/c.txt"]
    assert len(docs) == 3
    assert run_wc(ctx, docs, 4, app=M.APP_INDEXER, names=names) == O.indexer(docs, names, 4)


def test_boundary_wide_map(ctx, boundary):
    import oracle_lib as O
    from gpu_util import run_wc
    doc = U.sweep(boundary)[0]
    with knob(MRG_WIDE_MAP=1):
        got = run_wc(ctx, [doc], 3)
        st = ctx.stats()
    assert st["map_kind"] == 1, st
    assert got == O.wc([doc], 3, O.FAST)


# ================================================================ c. mrg_map_text over the full sweep

def test_map_text_full_sweep(ctx, full):
    import oracle_lib as O
    docs, toks, _ = full
    buf = b"".join(docs)
    got = ctx.map_text(buf, 1)
    assert len(got) == 1
    same_lines(got[0], [t + b" 1\n" for ts in toks for t in ts], "mr-0-0.txt")   # input order
    del got
    parts = ctx.map_text(buf, 7)
    exp = O.wc([buf], 7, O.FAST)
    for r in range(7):
        same_lines(ctx.reduce_text([parts[r]]), exp[r], f"mr-{r}.txt")


# ================================================================ d. the vocabulary

def test_vocabulary_full_sweep(ctx, full):
    """vocab_from_text accepts every W scalar (each stands in one word of the sweep); encode and decode over
    the 17 documents equal the constructed ids, offsets and normalized text."""
    docs, toks, items = full
    rk = sorted(items, key=lambda kv: (-kv[1], kv[0]))
    lines = [k + b" %d" % n for k, n in rk]
    assert lines[0] == b"z 25" and len(lines) == U.NSCALARS + 1
    text = cat(lines)
    rank = {k: i for i, (k, _) in enumerate(rk)}
    with ctx.vocab_from_text(text) as v:
        assert v.size() == (len(lines), len(text))
        assert v.text() == text
        exp, off = expected(toks, rank)
        assert exp.size == NTOKENS and not (exp == 0xFFFFFFFF).any()
        got, tok = encode(ctx, v, docs)
        assert tok == off
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), int(bad.size))
        exp_text, exp_off = expected_text([k for k, _ in rk], exp, off)
        got_text, got_off = decode(ctx, v, exp, off)
        assert got_off == exp_off
        same_lines(got_text, exp_text, "decoded text")


def test_vocabulary_rejects_every_other_scalar(ctx, boundary):
    import mapreduce_rust_amd as M
    cls = U.classes()
    rejected = sorted({c for c in boundary if cls[c] != U.W} | {0x0A, 0x20})   # '\n': a missing count; ' ': a second space
    assert len(rejected) > 1000
    bad = []
    for c in rejected:
        text = b"ok 1\n" + b"a" + chr(c).encode() + b"b 1\n"
        try:
            ctx.vocab_from_text(text).close()
            bad.append((hex(c), "accepted"))
        except M.MrgError as e:
            if e.code != M.native.EINVAL or "line 1:" not in str(e):
                bad.append((hex(c), str(e)))
    assert not bad, (len(bad), bad[:8])
    for c in [c for c in boundary if cls[c] == U.W][::97]:        # the same line with a W scalar is accepted
        text = b"ok 1\n" + b"a" + chr(c).encode() + b"b 1\n"
        with ctx.vocab_from_text(text) as v:
            assert v.text() == text


# ================================================================ e. positions in k_map's block

KINDS = [("e_acute", "é", U.W), ("section", "§", U.X), ("nel", "\u0085", U.S),
         ("cjk", "中", U.W), ("em_dash", "—", U.X), ("ideographic_space", "　", U.S),
         ("em_space", " ", U.S), ("deseret", "\U00010400", U.W), ("grin", "\U0001F600", U.X)]
NSHIFT = 2048 + 256 + 32


def make_filler(n, seed=20261019):
    """ASCII text with mixed word lengths (1 to 24 bytes: short keys, 16-byte keys, long keys)"""
    rng = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = "".join(rng.choice("abcdefghijklmnopqrstuvwxyzABCDEFGH0123_") for _ in range(rng.choice((1, 2, 3, 4, 5, 7, 8, 11, 15, 16, 17, 24))))
        w += rng.choice((" ", " ", " ", "\n", "  ", "-", "' "))
        out.append(w)
        size += len(w)
    return "".join(out).encode()[:n]


@pytest.fixture(scope="module")
def filler():
    return make_filler(NSHIFT + 64)


@pytest.mark.parametrize("name,ch,cls", KINDS, ids=[k[0] for k in KINDS])
def test_position_sweep(ctx, filler, name, ch, cls):
    """Documents c + filler[:s] + "q" + c + "r " + filler[:40] + c for s = 0 .. 2335, back to back: their
    starts cycle through every alignment, the codepoint's lead meets every lane of both tiles, the tile
    seam, the halo segment, the byte-before-the-block slot and a document's first and last bytes."""
    import oracle_lib as O
    from gpu_util import run_wc
    assert U.classes()[ord(ch)] == cls
    c = ch.encode()
    docs = [c + filler[:s] + b"q" + c + b"r " + filler[:40] + c for s in range(NSHIFT)]
    assert 2_500_000 < sum(map(len, docs)) < 3_500_000
    assert run_wc(ctx, docs, 3) == O.wc(docs, 3, O.FAST)
    assert ctx.stats()["nonascii_tiles"] > 0
    doc_tokens = [O.tokens(d) for d in docs]
    lines = ranked(count_lines(doc_tokens))
    with ctx.vocab_from_text(cat(lines)) as v:
        check(ctx, v, docs, rank_of(lines), doc_tokens)


@pytest.mark.parametrize("leads", [63, 64, 65])
def test_compacted_decode_edge(ctx, leads):
    """k_map compacts a block's leads one per lane when a lane holds two or more and the block has at most
    64.  A unit of a 2-byte codepoint and 30 ASCII bytes puts one lead into each tile's even segments: 64
    per 2 KiB block, two per even lane (T = 64).  One lead fewer (T = 63); one more, in an odd segment (T =
    65: the per-lane loop takes over).  The document is first in its buffer, so block 0 is its first 2 KiB.
    Both paths must give the same output, so the test cannot tell which one ran: it pins the results on both
    sides of the switch, not that the switch is at 64."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    ascii30 = b"bc d efgh ij klmnop qrs tu vw "
    assert len(ascii30) == 30
    units = [["é", "§", "\u0085", "ß"][i % 4].encode() + ascii30 for i in range(64)]
    if leads == 63:
        units[37] = b"ee" + ascii30
    if leads == 65:
        u = bytearray(units[20])
        assert u[17:19] == b"mn"
        u[17:19] = "é".encode()                  # bytes 17, 18 of the unit: the odd segment
        units[20] = bytes(u)
    block = b"".join(units)
    assert len(block) == 2048 and sum(b >= 0xC0 for b in block) == leads
    for tail in (b"", b"plain ascii tail\n", block[:1000]):
        doc = block + tail
        toks = O.tokens(doc)
        outs = run_wc(ctx, [doc], 1, flags=M.FLAG_NO_COMPAT_DROP_LAST)
        same_lines(outs[0], U.lines([toks]), f"{leads} leads, tail of {len(tail)}")
        assert ctx.stats()["nonascii_tiles"] >= 2
        lines = ranked(count_lines([toks]))
        with ctx.vocab_from_text(cat(lines)) as v:
            check(ctx, v, [doc], rank_of(lines), [toks])


# ================================================================ f. invalid UTF-8: the exact report

class Packed:
    """Many small jobs' documents in one device buffer, each job in a slot of its own (64-byte aligned)."""

    def __init__(self, jobs):
        import torch
        size = max(sum(len(d) for d in j) for j in jobs)
        self.slot = (size + 64 + 63) // 64 * 64
        buf = bytearray(self.slot * len(jobs) + 64)
        self.off = []
        for i, j in enumerate(jobs):
            o = [0]
            for d in j:
                buf[i * self.slot + o[-1]:i * self.slot + o[-1] + len(d)] = d
                o.append(o[-1] + len(d))
            self.off.append(o)
        self.t = torch.frombuffer(buf, dtype=torch.uint8).to("cuda:0")
        assert self.t.data_ptr() % 64 == 0

    def ptr(self, i):
        return self.t.data_ptr() + i * self.slot


@pytest.fixture
def reuse(ctx):
    """Around a test of failing calls: afterwards the pool holds what it held before and the same context
    runs a valid Unicode job exactly."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    exp = O.wc(GOOD_DOCS, 3, O.FAST)
    assert run_wc(ctx, GOOD_DOCS, 3) == exp
    ctx.job_begin(M.APP_WC, 1)
    before = ctx.pool_stats()[0]
    yield
    ctx.job_begin(M.APP_WC, 1)
    assert ctx.pool_stats()[0] == before, "scratch not returned"
    assert run_wc(ctx, GOOD_DOCS, 3) == exp


def map_error(ctx, ptr, off, app=None, names=None):
    """The MrgError of a map over the documents, or None if it succeeds."""
    import mapreduce_rust_amd as M
    ctx.job_begin(M.APP_WC if app is None else app, 3)
    if names is not None:
        ctx.set_doc_names(names)
    ctx.set_input(ptr, off)
    try:
        ctx.map()
    except M.MrgError as e:
        return e
    return None


def wrong_report(e, code, *parts, end=None):
    """None if e is the error `code` whose message holds every part (and ends in `end`), else a description"""
    if e is None:
        return "no error"
    msg = str(e)
    if e.code != code or not all(p in msg for p in parts) or (end is not None and not msg.endswith(end)):
        return msg
    return None


def invalid_docs(matrix):
    """(document, offset of its first invalid byte) of every invalid string of the matrix, embedded, and of
    the sequences truncated by the document's end"""
    out = [(U.embed(q), U.py_error(U.embed(q))) for q in matrix if U.py_error(q) is not None]
    out += [(b"ab cd " + t, 6) for t in U.TRUNCATED]
    assert all(at == U.py_error(d) and at is not None for d, at in out)
    return out


SMALL_VOCAB = b"ab 1\ncd 1\nef 1\nfine 1\ntext 1\n"


def test_matrix_valid_half(ctx):
    import oracle_lib as O
    from gpu_util import run_wc
    docs = [U.embed(q) for q in U.utf8_matrix() if U.py_error(q) is None]
    assert len(docs) == 1611 - 1497
    assert run_wc(ctx, docs, 3) == O.wc(docs, 3, O.FAST)
    doc_tokens = [O.tokens(d) for d in docs]
    lines = ranked(count_lines(doc_tokens))
    with ctx.vocab_from_text(cat(lines)) as v:
        check(ctx, v, docs, rank_of(lines), doc_tokens)
    joined = b" ".join(docs)
    same_lines(ctx.map_text(joined, 1)[0], [t + b" 1\n" for t in O.tokens(joined)], "mr-0-0.txt")


def test_matrix_invalid_map(ctx, reuse):
    import mapreduce_rust_amd as M
    cases = invalid_docs(U.utf8_matrix())
    assert len(cases) == 1497 + len(U.TRUNCATED)
    p = Packed([[FINE, d] for d, _ in cases])
    bad = []
    for i, (d, at) in enumerate(cases):
        w = wrong_report(map_error(ctx, p.ptr(i), p.off[i]), M.native.EUTF8, "document 1 (id 1", end=f"byte offset {at}")
        if w:
            bad.append((d.hex(), at, w))
    assert not bad, (len(bad), bad[:6])


def test_matrix_invalid_encode(ctx, reuse):
    import mapreduce_rust_amd as M
    cases = invalid_docs(U.utf8_matrix())
    p = Packed([[FINE, d] for d, _ in cases])
    bad = []
    with ctx.vocab_from_text(SMALL_VOCAB) as v:
        for i, (d, at) in enumerate(cases):
            try:
                ctx.encode(v, p.ptr(i), p.off[i])
                e = None
            except M.MrgError as err:
                e = err
            w = wrong_report(e, M.native.EUTF8, "document 1,", end=f"byte offset {at}")
            if w:
                bad.append((d.hex(), at, w))
        check(ctx, v, [FINE, b"ab cd ef"], rank_of(SMALL_VOCAB.split(b"\n")[:-1]))
    assert not bad, (len(bad), bad[:6])


def test_matrix_invalid_map_text(ctx, reuse):
    import mapreduce_rust_amd as M
    bad = []
    for d, at in invalid_docs(U.utf8_matrix()):
        try:
            ctx.map_text(d, 3)
            e = None
        except M.MrgError as err:
            e = err
        w = wrong_report(e, M.native.EUTF8, end=f"byte offset {at}")
        if w:
            bad.append((d.hex(), at, w))
    assert not bad, (len(bad), bad[:6])


def test_thin_matrix_indexer_and_wide_map(ctx, reuse):
    import mapreduce_rust_amd as M
    cases = invalid_docs(U.utf8_matrix_thin())
    assert {d[6] for d, _ in cases[:-len(U.TRUNCATED)]} == set(U.M_B0) and len(cases) > 600
    p = Packed([[FINE, d] for d, _ in cases])
    names = ["fine.txt", "bad.txt"]
    bad = []
    for i, (d, at) in enumerate(cases):
        e = map_error(ctx, p.ptr(i), p.off[i], M.APP_INDEXER, names)
        w = wrong_report(e, M.native.EUTF8, "document 1 (id 1, bad.txt)", end=f"byte offset {at}")
        if w:
            bad.append(("indexer", d.hex(), at, w))
    with knob(MRG_WIDE_MAP=1):
        for i, (d, at) in enumerate(cases):
            w = wrong_report(map_error(ctx, p.ptr(i), p.off[i]), M.native.EUTF8, "document 1 (id 1", end=f"byte offset {at}")
            if w:
                bad.append(("wide", d.hex(), at, w))
    assert not bad, (len(bad), bad[:6])


def test_thin_matrix_vocab_from_text(ctx, reuse):
    """A line that strict UTF-8 decoding rejects is MRG_EUTF8 with the line named, whatever else the line
    holds (some strings of the matrix also hold a space, DEL or a codepoint that is not \\w)."""
    import mapreduce_rust_amd as M
    bad = []
    for q in U.utf8_matrix_thin():
        if U.py_error(q) is None:
            continue
        try:
            ctx.vocab_from_text(b"ok 1\n" + b"a" + q + b"b 1\n").close()
            e = None
        except M.MrgError as err:
            e = err
        w = wrong_report(e, M.native.EUTF8, "line 1:")
        if w:
            bad.append((q.hex(), w))
    assert not bad, (len(bad), bad[:6])


REPRESENTATIVE = [b"\x80", b"\xc0\x80", b"\xc3\x41", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f\xbf\xbf",
                  b"\xf4\x90\x80\x80", b"\xff", b"\xe2\x82\x41", b"\xf0\x9f\x98\x41", b"\xe2\x82\xac\x80",
                  b"\xf0\x9f\x98\x80"]      # the last one is valid: it fails only where the document's end cuts it
# a 13th: a valid codepoint and five orphan continuation bytes, so that a segment, tile or block can begin
# behind four continuation bytes in a row (the first invalid byte, q + 3, then belongs to an earlier lane)
ORPHANS = b"\xe2\x82\xac\x80\x80\x80\x80\x80"
DOC_LEN = 2100
SEAMS_AT = list(range(1016, 1033)) + list(range(2040, 2057))
TAIL_AT = [DOC_LEN - k for k in (4, 3, 2, 1)]


@pytest.mark.parametrize("layout", ["first", "second"])
def test_error_positions(ctx, reuse, filler, layout):
    """13 strings with their lead around the tile seam (1016..1032), the block seam (2040..2056) and at the
    last 1 to 4 bytes of a 2100-byte document (which then cuts the sequence).  k_map lays its grid per
    document, from the document's start rounded down to 16 bytes.  Layout "first": the document is alone and
    first in its buffer, so its offsets 1024 and 2048 ARE the tile and the block seam, and leads at seam - 3
    .. seam - 1 have their continuation bytes (or orphans) in the next tile or block: lane 0 there looks back
    across the seam.  Layout "second": document 1 behind a 9-byte document, as in the other tests here; the
    seams are then its offsets 1015 and 2039, so the same leads are also placed 9 bytes earlier.  Where the
    document is valid after all (the valid string in full, a cut that leaves whole codepoints) the job must
    equal the oracle."""
    import mapreduce_rust_amd as M
    import oracle_lib as O
    strings = REPRESENTATIVE + [ORPHANS]
    assert len(REPRESENTATIVE) == 12
    head = [] if layout == "first" else [FINE]
    doc_lo = sum(map(len, head))
    n = len(head)
    lead_at = sorted(set(SEAMS_AT) | {a - doc_lo for a in SEAMS_AT}) + TAIL_AT
    cases = [(q, at) for q in strings for at in lead_at]
    # a multi-byte lead in the last three bytes of a tile and of a block, its other bytes behind the seam
    for seam in (1024, 2048):
        assert {(doc_lo + at) - seam for q, at in cases if q[0] >= 0xC2 and len(q) >= 4} >= {-3, -2, -1}
    assert any((doc_lo + at) % 1024 in (1021, 1022, 1023) for q, at in cases if q is ORPHANS)
    docs = [(filler[:at] + q + filler[at + len(q):])[:DOC_LEN] for q, at in cases]
    assert all(len(d) == DOC_LEN for d in docs)
    p = Packed([head + [d] for d in docs])
    bad, n_valid = [], 0
    with ctx.vocab_from_text(SMALL_VOCAB) as v:
        for i, d in enumerate(docs):
            at = U.py_error(d)
            if at is None:
                n_valid += 1
                if job(ctx, p.ptr(i), p.off[i], 3) != O.wc(head + [d], 3, O.FAST):
                    bad.append(("valid", i, "differs from the oracle"))
                exp_off = [0] + ([2] if head else [])
                if ctx.encode(v, p.ptr(i), p.off[i]) != exp_off + [exp_off[-1] + len(O.tokens(d))]:
                    bad.append(("valid", i, "token offsets"))
                continue
            w = wrong_report(map_error(ctx, p.ptr(i), p.off[i]), M.native.EUTF8, f"document {n} (id {n}", end=f"byte offset {at}")
            if w:
                bad.append(("map", cases[i][0].hex(), cases[i][1], at, w))
            try:
                ctx.encode(v, p.ptr(i), p.off[i])
                e = None
            except M.MrgError as err:
                e = err
            w = wrong_report(e, M.native.EUTF8, f"document {n},", end=f"byte offset {at}")
            if w:
                bad.append(("encode", cases[i][0].hex(), cases[i][1], at, w))
    assert 30 < n_valid < 120         # the valid string at every inner position, and a few whole cuts
    assert not bad, (len(bad), bad[:6])


def test_codepoint_split_across_documents(ctx, reuse, filler):
    """Document 1 ends E2 82 and document 2 starts AC, at every alignment of the boundary mod 16, in the
    first block and beyond it: the report is document 1 (the lowest failing one) at its length - 2."""
    import mapreduce_rust_amd as M
    jobs = []
    for base in (0, 2032):
        for a in range(16):
            jobs.append([FINE, filler[:base] + b" ab " + b"y" * a + b" w\xe2\x82", b"\xac tail text"])
    assert {sum(map(len, j[:2])) % 16 for j in jobs} == set(range(16))
    p = Packed(jobs)
    bad = []
    with ctx.vocab_from_text(SMALL_VOCAB) as v:
        for i, j in enumerate(jobs):
            at = len(j[1]) - 2
            assert U.py_error(j[1]) == at and U.py_error(j[2]) == 0
            w = wrong_report(map_error(ctx, p.ptr(i), p.off[i]), M.native.EUTF8, "document 1 (id 1", end=f"byte offset {at}")
            if w:
                bad.append(("map", i, at, w))
            try:
                ctx.encode(v, p.ptr(i), p.off[i])
                e = None
            except M.MrgError as err:
                e = err
            w = wrong_report(e, M.native.EUTF8, "document 1,", end=f"byte offset {at}")
            if w:
                bad.append(("encode", i, at, w))
    assert not bad, (len(bad), bad[:6])
