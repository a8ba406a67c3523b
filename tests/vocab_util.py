"""Helpers shared by the vocabulary tests (copies of the small helpers of tests/test_gpu_encode.py, which
stays as it is).  No expectation comes from the library: tokens come from the C oracle
(oracle_lib.tokens), ranks from a Counter over them sorted by (count descending, key bytes ascending)."""
import collections

import numpy as np

NO_COMPAT = 0x1
UNK = 0xFFFFFFFF
SENTINEL = 0xFFFFFFFE  # never an id here (vocabularies are far smaller) and not UNK
BYTE_SENTINEL = 0xA5   # fills a decode destination: bytes the call must not touch keep it


def ranked(lines):
    def order(ln):
        key, c = ln.rsplit(b" ", 1)
        return (-int(c), key)
    return sorted(lines, key=order)


def cat(lines):
    return b"".join(l + b"\n" for l in lines)


def count_lines(doc_tokens):
    cnt = collections.Counter()
    for t in doc_tokens:
        cnt.update(t)
    return [k + b" " + str(c).encode() for k, c in cnt.items()]


def words_of(lines):
    return [ln.rsplit(b" ", 1)[0] for ln in lines]


def rank_of(lines):
    return {ln.rsplit(b" ", 1)[0]: i for i, ln in enumerate(lines)}


def expected(doc_tokens, rank):
    ids, off = [], [0]
    for t in doc_tokens:
        ids += [rank.get(x, UNK) for x in t]
        off.append(len(ids))
    return np.array(ids, dtype=np.uint32), off


def start_job(ctx, blobs, R=1, flags=NO_COMPAT):
    import mapreduce_rust_amd as M
    from gpu_util import to_device
    t, off = to_device(blobs)
    ctx.job_begin(M.APP_WC, R, flags)
    ctx.set_input(t.data_ptr(), off)
    ctx.map()
    return t


def encode_dev(ctx, v, ptr, off):
    """count-only call, then the full call into a sentinel-filled buffer; returns (ids, tok_off)"""
    import torch
    tok = ctx.encode(v, ptr, off)
    assert len(tok) == len(off) and tok[0] == 0
    n = tok[-1]
    out = torch.full((n + 3,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda:0")
    tok2 = ctx.encode(v, ptr, off, out.data_ptr(), n)
    assert tok2 == tok, "the count-only call and the full call disagree on the offsets"
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[n:] == SENTINEL).all(), "wrote past the last token"
    return got[:n], tok


def encode(ctx, v, blobs):
    from gpu_util import to_device
    t, off = to_device(blobs)
    got, tok = encode_dev(ctx, v, t.data_ptr(), off)
    del t
    return got, tok


def check(ctx, v, blobs, rank, doc_tokens=None):
    import oracle_lib as O
    if doc_tokens is None:
        doc_tokens = [O.tokens(b) for b in blobs]
    exp, off = expected(doc_tokens, rank)
    got, tok = encode(ctx, v, blobs)
    assert tok == off
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]), bad.size)


# the Unicode table of tests/test_gpu_encode.py: text, its tokens' keys
UNI = [
    ("don't a\u2014b -- x", [b"dont", b"ab", b"x"]),
    ("p\u0085q\u00a0r\u2003s\u3000t\u2028u", [b"p", b"q", b"r", b"s", b"t", b"u"]),   # each one White_Space
    ("a\u200bb", [b"ab"]),                                     # ZERO WIDTH SPACE is neither \s nor \w
    ("''' \u2014 ...", []),
    ("e\u0301 x", ["e\u0301".encode(), b"x"]),                  # the combining mark is \w
    ("\U00010400bc \U00010400", ["\U00010400bc".encode(), "\U00010400".encode()]),   # a 4-byte letter starts a token
]


def tie_words():
    words = ["abcdefgh", "abcdefgh1", "abcdefgh2", "abcdefghi", "abcdefghij1", "abcdefghij2"]
    words += [w + s for w in ("x" * 16, "x" * 16 + "a", "x" * 17, "x" * 30) for s in ("", "\u00e9")]
    words += ["na\u00efve", "\u017fong", "\u00c6r\u00f8", "a"]
    words += ["w%02d" % i for i in range(42)]
    return words


def expected_text(words, ids, tok_off, unk=b""):
    """The decoded text, built in Python: every id's word and a separator, ' ' inside a document and '\\n'
    after its last id.  Returns (text, out_off)."""
    parts, off = [], [0]
    for d in range(len(tok_off) - 1):
        seg = ids[tok_off[d]:tok_off[d + 1]]
        if len(seg):
            parts.append(b" ".join(unk if i == UNK else words[i] for i in seg.tolist()) + b"\n")
            off.append(off[-1] + len(parts[-1]))
        else:
            off.append(off[-1])
    return b"".join(parts), off


def ids_to_device(ids):
    """uint32 ids on the device (at least one element, so that the pointer is real)"""
    import torch
    a = np.ascontiguousarray(ids, dtype=np.uint32)
    if a.size == 0:
        a = np.zeros(4, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32).copy()).to("cuda:0")


def decode_dev(ctx, v, ids_ptr, tok_off, unk=b""):
    """sizes-only call, then the full call with cap = the exact size into a buffer that is 64 bytes longer
    and sentinel-filled; returns (text, out_off, the device tensor)"""
    import torch
    off = ctx.decode(v, ids_ptr, tok_off, unk=unk)
    assert len(off) == len(tok_off) and off[0] == 0
    n = off[-1]
    out = torch.full((n + 64,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda:0")
    off2 = ctx.decode(v, ids_ptr, tok_off, out.data_ptr(), n, unk=unk)
    assert off2 == off, "the sizes-only call and the full call disagree on the offsets"
    torch.cuda.synchronize()
    got = out.cpu().numpy().tobytes()
    assert got[n:] == bytes([BYTE_SENTINEL]) * 64, "wrote past the last byte"
    return got[:n], off, out


def decode(ctx, v, ids, tok_off, unk=b""):
    t = ids_to_device(ids)
    got, off, out = decode_dev(ctx, v, t.data_ptr(), tok_off, unk)
    del t, out
    return got, off
