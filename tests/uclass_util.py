"""Builders shared by tests/test_uclass_cpu.py and tests/test_gpu_unicode.py.  Nothing here touches the GPU,
the library or the oracle: the class of a scalar comes from the fixture tests/golden/uclass_runs.json
(written by tools/gen_unicode_tables.py), the expected tokens of a sweep follow from the class by
construction, and UTF-8 acceptance is Python's strict decoder."""
import collections
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "uclass_runs.json")
X, W, S = 0, 1, 2
NSCALARS = 0x110000 - 0x800          # 1,112,064: every codepoint but the surrogates
SEAMS = (0x7F, 0x80, 0x7FF, 0x800, 0x1FFF, 0x2000, 0x20FF, 0x2100, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def classes():
    """uint8[0x110000]: the class (0 X, 1 W, 2 S) of every codepoint; surrogates are 0.  Read-only."""
    runs = fixture()["runs"]
    starts = np.array([a for a, _ in runs] + [0x110000], dtype=np.int64)
    cls = np.repeat(np.array([c for _, c in runs], dtype=np.uint8), np.diff(starts))
    assert cls.size == 0x110000 and starts[0] == 0
    cls.setflags(write=False)
    return cls


def is_surrogate(c):
    return 0xD800 <= c <= 0xDFFF


@functools.lru_cache(maxsize=None)
def boundary_set():
    """A few thousand scalars: both sides of every class change, the seams of the encodings and of
    uni_class's table split, and every 251st scalar.  Sorted, no surrogates."""
    out = set(SEAMS)
    for a, _ in fixture()["runs"]:
        out.update((a - 1, a))
    out.update(range(0, 0x110000, 251))
    return tuple(sorted(c for c in out if 0 <= c < 0x110000 and not is_surrogate(c)))


def sweep(scalars, prefix=b""):
    """One unit prefix + HEX + c + b"z " per scalar c.  Returns (document bytes, its expected tokens): the
    hex names the scalar in every key, so no two misclassifications can cancel."""
    cls = classes()
    parts, toks = [], []
    for c in scalars:
        head = prefix + b"%X" % c
        enc = chr(c).encode()
        parts.append(head + enc + b"z ")
        k = cls[c]
        if k == W:
            toks.append(head + enc + b"z")
        elif k == X:
            toks.append(head + b"z")
        else:
            toks.append(head)
            toks.append(b"z")
    return b"".join(parts), toks


def plane_scalars(p):
    return [c for c in range(p << 16, (p + 1) << 16) if not is_surrogate(c)]


@functools.lru_cache(maxsize=None)
def full_sweep():
    """Every scalar, one document per plane: (17 documents, 17 token lists)."""
    docs, toks = zip(*(sweep(plane_scalars(p)) for p in range(17)))
    return list(docs), list(toks)


def chunks(seq, n):
    """seq cut into n nearly equal consecutive pieces"""
    k = (len(seq) + n - 1) // n
    return [seq[i:i + k] for i in range(0, len(seq), k)]


def count_items(doc_tokens):
    """(key, count) of every distinct token of the documents, sorted bytewise by key"""
    cnt = collections.Counter()
    for t in doc_tokens:
        cnt.update(t)
    return sorted(cnt.items())


def lines(doc_tokens):
    """The "key count\\n" lines of a word count over the documents' tokens, sorted bytewise."""
    return [k + b" %d\n" % n for k, n in count_items(doc_tokens)]


# ---- UTF-8 acceptance

M_B0 = (0x80, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xF7,
        0xF8, 0xFB, 0xFC, 0xFE, 0xFF)
M_B1 = (0x20, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC2, 0xE0, 0xFF)
M_TAILS = (b"\x80\x80", b"\x41\x41", b"\x80\x41")
M4_B0 = (0xE0, 0xE1, 0xED, 0xEF, 0xF0, 0xF1, 0xF4)
M4_B1 = (0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF)
M4_B2 = (0x41, 0x7F, 0x80, 0xBF, 0xC0)
M4_B3 = (0x41, 0x80, 0xBF, 0xC0)
THIN_B1 = (0x41, 0x80, 0xBF)
FULL_ROWS = (0xE0, 0xED, 0xF0, 0xF4)


@functools.lru_cache(maxsize=None)
def utf8_matrix():
    """4-byte strings around every acceptance edge of UTF-8 (leads, second-byte ranges, continuation or
    not), valid and invalid, without duplicates, in a fixed order."""
    out = {}
    for b0 in M_B0:
        for b1 in M_B1:
            for t in M_TAILS:
                out[bytes((b0, b1)) + t] = None
    for b0 in M4_B0:
        for b1 in M4_B1:
            for b2 in M4_B2:
                for b3 in M4_B3:
                    out[bytes((b0, b1, b2, b3))] = None
    return tuple(out)


def utf8_matrix_thin():
    """The matrix thinned along b1 only: every lead with b1 in {41, 80, BF}, the E0/ED/F0/F4 rows in full."""
    return tuple(q for q in utf8_matrix() if q[1] in THIN_B1 or q[0] in FULL_ROWS)


def embed(q):
    return b"ab cd " + q + b" ef"


def py_error(doc):
    """None if doc is valid UTF-8, else the offset of the first invalid byte: UnicodeDecodeError.start of a
    strict decode, which is also Rust's Utf8Error::valid_up_to()."""
    try:
        bytes(doc).decode("utf-8")
    except UnicodeDecodeError as e:
        return e.start
    return None


# truncated sequences at a document's end: 1, 2 or 3 bytes of a 2-, 3- and 4-byte codepoint
TRUNCATED = (b"\xc3", b"\xe2", b"\xe2\x82", b"\xf0", b"\xf0\x9f", b"\xf0\x9f\x98")
