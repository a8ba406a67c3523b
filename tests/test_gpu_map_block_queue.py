"""GPU tests: the wc map's block queue (k_map<CAP, false, false>: one staging, one scan and one token queue
per 2 KiB block, drained 40 segments at a time when a block holds more than 320 token starts).

Every expectation is the C oracle's (oracle_lib) over inputs built here from fixed seeds; nothing comes from
the library.  A document's blocks lie on the 16-byte grid below its first byte, so "offset o of a block" is
arranged by giving a document a first byte on that grid (documents of whole 16-byte multiples in front of it)
and placing bytes at o, o + 2048, ...  The same inputs also run as indexer jobs (the per-tile path) and one
near-unique job runs through the wide map: the other instantiations of the kernel.

Invalid UTF-8 is a documented input with a defined error return; nothing here is meant to fault the device."""
import contextlib
import os
import random

import pytest

pytestmark = pytest.mark.gpu

BLK = 2048
WORDS = [b"a", b"of", b"the", b"word", b"count", b"kernel", b"mapping", b"doorkeep", b"tokenizer", b"don't", b"x-ray,"]
GOOD_DOCS = [b"fine text " * 40, "café naïve ’tis 中文　\U00010400x \U0001F600y\u0085z ".encode() * 90]


@pytest.fixture(scope="module")
def ctx():
    import mapreduce_rust_amd as M
    c = M.Context(0)
    yield c
    c.close()


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


# ---------------------------------------------------------------- builders (host only, fixed seeds)

def filler(n, seed):
    """n bytes of space-separated words (the last one cut where the length says)"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + b" "
    return bytes(out[:n])


def layout(size, placed, seed):
    """size bytes: every (position, bytes) of `placed` where it says, a space on both sides of it, and words in
    the gaps between them"""
    rng = random.Random(seed)
    buf = bytearray(b" " * size)
    used = bytearray(size)
    for pos, b in placed:
        assert pos >= 1 and pos + len(b) < size and not any(used[pos - 1:pos + len(b) + 1]), (pos, len(b))
        buf[pos:pos + len(b)] = b
        used[pos - 1:pos + len(b) + 1] = b"\1" * (len(b) + 2)
    i = 0
    while i < size:
        if used[i]:
            i += 1
            continue
        j = i
        while j < size and not used[j]:
            j += 1
        p = i                       # words into the free bytes [i, j), each followed by a space
        while p < j:
            w = rng.choice(WORDS)
            if p + len(w) + 1 > j:
                break
            buf[p:p + len(w)] = w
            p += len(w) + 1
        i = j
    return bytes(buf)


def starts_block(n):
    """One 2 KiB block with exactly n token starts: n tokens of (near) equal period, each followed by one space"""
    base, extra = divmod(BLK, n)
    assert base >= 2
    out = bytearray()
    for i in range(n):
        ln = base + (1 if i < extra else 0)
        out += bytes([97 + (i * 7 + n) % 26]) * (ln - 1) + b" "
    assert len(out) == BLK and len(out.split()) == n
    return bytes(out)


def key(L, salt):
    return bytes(97 + (salt * 5 + k * 3 + L) % 26 for k in range(L))


PLAIN, APOS, PUNCT = "plain", "apostrophe", "punctuation"
OFFSETS = list(range(1000, 1041)) + list(range(2030, 2071))


def boundary_token(L, o, kind):
    """The raw token of L key bytes that starts at block offset o"""
    k = key(L, o)
    if kind == PLAIN:
        return k
    if kind == APOS:           # one deleted byte inside the token (none fits inside a 1-byte key: behind it)
        return k[:max(1, L // 2)] + b"'" + k[max(1, L // 2):]
    edge = 1024 if o < 1500 else 2048   # a run of deleted bytes where the token meets the tile / block end
    cut = min(max(edge - o, 1), L)
    return k[:cut] + b"-.,;" + k[cut:]


def boundary_doc(L, kind):
    """Cells of one block each behind a block of words; a cell holds the token at offsets 1000 + i and 2030 + i
    (i = 0..40) of a block: the cells of 2048..2070 first, so a token that crosses a block's end runs into a cell
    with words there"""
    order = list(range(18, 41)) + list(range(0, 18))
    placed = []
    for c, i in enumerate(order, 1):
        placed.append((c * BLK + 1000 + i, boundary_token(L, 1000 + i, kind)))
        o2 = 2030 + i
        placed.append((c * BLK + (o2 if o2 < BLK else o2 - BLK), boundary_token(L, o2, kind)))
    placed.sort()
    return layout((len(order) + 2) * BLK, placed, 1000 * L + len(kind))


@pytest.fixture(scope="module")
def edge_docs():
    docs = [starts_block(n) + filler(300, n) for n in (255, 256, 257, 319, 320, 321, 1024)]
    dense, sparse = b"a " * 512, b"abcdefghijklmno " * 64
    docs += [dense + sparse + filler(100, 1), sparse + dense + filler(100, 2)]
    return docs


@pytest.fixture(scope="module")
def unaligned_docs():
    """three of the dense documents back to back, their first bytes 5, 8 and 9 past the 16-byte grid"""
    a, b, c = starts_block(321) + b"end", b"a " * 1024 + b"b", starts_block(257)
    docs = [b"five ", a, b, c]
    off = [sum(map(len, docs[:i])) % 16 for i in range(1, 4)]
    assert off == [5, 8, 9], off
    return docs


END_LENGTHS = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 2112)


@pytest.fixture(scope="module")
def end_docs():
    return [filler(n, 7000 + n) for n in END_LENGTHS]


@pytest.fixture(scope="module")
def boundary_docs():
    return {kind: [boundary_doc(L, kind) for L in range(1, 41)] for kind in (PLAIN, APOS, PUNCT)}


# W, S and deleted codepoints of 2, 3 and 4 bytes (no White_Space codepoint has 4)
SCALARS = ["é", "中", "\U00010400", "\u0085", "　", "§", "’", "\U0001F600"]


@pytest.fixture(scope="module")
def nonascii_doc():
    """cells of two blocks: each codepoint inside a token, split every way by byte 1024 and by byte 2048"""
    placed, c = [], 0
    for ch in SCALARS:
        e = ch.encode()
        for k in range(1, len(e)):
            for edge in (1024, 2048):
                placed.append((c * 2 * BLK + edge - k - 2, b"ab" + e + b"cd"))
                c += 1
    return layout((c + 1) * 2 * BLK, placed, 99)


def check_wc(ctx, docs, R=3):
    import oracle_lib as O
    from gpu_util import run_wc
    got = run_wc(ctx, docs, R)
    st = ctx.stats()
    assert st["map_kind"] == 0, st      # the LDS-table map, not the wide one
    exp = O.wc(docs, R, O.FAST)
    for r in range(R):
        assert got[r] == exp[r], f"mr-{r}.txt differs ({len(got[r])} / {len(exp[r])} bytes)"
    assert st["tokens"] == sum(1 for d in docs for t in O.tokens(d) if t), st


def check_indexer(ctx, docs, R=3):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc
    names = [f"d/{i}.txt" for i in range(len(docs))]
    assert run_wc(ctx, docs, R, app=M.APP_INDEXER, names=names) == O.indexer(docs, names, R)


# ---------------------------------------------------------------- round and queue edges

def test_starts_per_block(ctx, edge_docs):
    """255 .. 321 and 1024 starts in one block (two rounds, a third, the queue's capacity, drained ranges),
    and blocks with one dense and one sparse tile"""
    for d in edge_docs:
        check_wc(ctx, [d], 2)
    check_wc(ctx, edge_docs)


def test_starts_per_block_unaligned(ctx, unaligned_docs):
    check_wc(ctx, unaligned_docs)


def test_starts_per_block_small_table(edge_docs, unaligned_docs):
    """the 2048-slot instantiation takes the same path"""
    import mapreduce_rust_amd as M
    with knob(MRG_LDS_CAP=2048):
        with M.Context(0) as c:
            check_wc(c, edge_docs + unaligned_docs)


# ---------------------------------------------------------------- document ends inside a block

def test_document_ends(ctx, end_docs):
    check_wc(ctx, end_docs)
    check_wc(ctx, end_docs[::-1], 1)


@pytest.mark.parametrize("n", END_LENGTHS)
def test_document_alone(ctx, end_docs, n):
    check_wc(ctx, [end_docs[END_LENGTHS.index(n)]], 2)


# ---------------------------------------------------------------- tokens across the tile seam and the block end

@pytest.mark.parametrize("kind", [PLAIN, APOS, PUNCT])
def test_tokens_across_boundaries(ctx, boundary_docs, kind):
    """keys of 1..40 bytes (17 and more: long tokens) starting at every offset 1000..1040 and 2030..2070"""
    docs = boundary_docs[kind]
    check_wc(ctx, docs)
    assert ctx.stats()["long_tokens"] == 24 * len(OFFSETS)


# ---------------------------------------------------------------- non-ASCII

def test_codepoints_across_boundaries(ctx, nonascii_doc):
    check_wc(ctx, [nonascii_doc])
    assert ctx.stats()["nonascii_tiles"] > 0
    check_wc(ctx, [b"seven b", nonascii_doc], 1)


@pytest.mark.parametrize("at", [1023, 1024, 2047, 2048])
def test_invalid_byte_offset(ctx, at):
    import mapreduce_rust_amd as M
    import oracle_lib as O
    from gpu_util import run_wc, to_device
    good = O.wc(GOOD_DOCS, 3, O.FAST)
    first = b"fine text " * 8                      # 80 bytes: the second document starts on the 16-byte grid
    bad = bytearray(filler(3 * BLK, at))
    bad[at] = 0xFF
    t, off = to_device([first, bytes(bad)])
    ctx.job_begin(M.APP_WC, 3)
    ctx.set_input(t.data_ptr(), off)
    with pytest.raises(M.MrgError) as e:
        ctx.map()
    assert e.value.code == M.native.EUTF8 and "document 1 (id 1" in str(e.value), str(e.value)
    assert str(e.value).endswith(f"byte offset {at}"), str(e.value)
    assert run_wc(ctx, GOOD_DOCS, 3) == good        # the same context afterwards


# ---------------------------------------------------------------- the other instantiations

def test_same_inputs_indexer(ctx, edge_docs, unaligned_docs, end_docs, boundary_docs, nonascii_doc):
    check_indexer(ctx, edge_docs)
    check_indexer(ctx, unaligned_docs)
    check_indexer(ctx, end_docs)
    for d in end_docs:
        check_indexer(ctx, [d], 1)
    for kind in (PLAIN, APOS, PUNCT):
        check_indexer(ctx, boundary_docs[kind])
    check_indexer(ctx, [nonascii_doc])


def test_near_unique_wide_map(ctx):
    import oracle_lib as O
    from gpu_util import run_wc
    rng = random.Random(5)
    doc = b" ".join(b"%x" % rng.getrandbits(48) for _ in range(6000)) + b" " + starts_block(321)
    with knob(MRG_WIDE_MAP=1):
        got = run_wc(ctx, [doc], 3)
        st = ctx.stats()
    assert st["map_kind"] == 1, st
    assert got == O.wc([doc], 3, O.FAST)
