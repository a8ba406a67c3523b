"""CPU tests of the codepoint classes and of the references the GPU Unicode tests lean on.

The fixture tests/golden/uclass_runs.json holds the class of every Unicode scalar.  Here it is checked,
for all 1,112,064 scalars, against the product table (the text of uclass_table.inc, by the formula in its
own header), the oracle's oracle_class(), the live `regex` module (when it is the recorded version) and
stdlib `unicodedata` (an independent source).  Then the two references of tests/test_gpu_unicode.py are tied
together: the by-construction tokens of uclass_util.sweep() against the oracle's tokenizer and word count,
and Python's strict UTF-8 decoder against oracle_validate_utf8 over the acceptance matrix."""
import ctypes
import os
import re
import unicodedata

import numpy as np
import pytest

import oracle_lib as O
import uclass_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "uclass_table.inc")

# PropList.txt, White_Space: stable since Unicode 6.3 (25 scalars)
WHITE_SPACE = ([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
               [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
JOIN_CONTROL = [0x200C, 0x200D]


def scalars():
    return np.concatenate([np.arange(0, 0xD800), np.arange(0xE000, 0x110000)])


def first_diff(a, b):
    bad = np.nonzero(a != b)[0]
    return None if bad.size == 0 else ("U+%04X" % bad[0], int(a[bad[0]]), int(b[bad[0]]), int(bad.size))


def test_fixture_shape():
    cls = U.classes()
    fx = U.fixture()
    runs = fx["runs"]
    assert runs[0][0] == 0 and all(a < b for (a, _), (b, _) in zip(runs, runs[1:]))
    assert all(c in (0, 1, 2) for _, c in runs) and all(c != d for (_, c), (_, d) in zip(runs, runs[1:]))
    assert len(runs) == 1623
    assert (cls[0xD800:0xE000] == 0).all()
    assert int((cls == U.W).sum()) == 149_366 and int((cls == U.S).sum()) == 25
    assert scalars().size == U.NSCALARS == 1_112_064
    assert fx["unicode_version"] == "17.0.0" and fx["regex_version"]


FORMULA = ("class(cp) = (MRG_UCLASS_STAGE2[MRG_UCLASS_STAGE1[cp >> 8] * 64 + ((cp & 255) >> 2)] "
           ">> (2 * (cp & 3))) & 3")


def parse_table():
    text = open(TABLE).read()

    def init(name):
        body = re.search(r"#define %s \{(.*?)\}" % name, text, re.S)
        assert body, name
        return np.array([int(x) for x in re.findall(r"\d+", body.group(1))], dtype=np.int64)
    nblocks = int(re.search(r"#define MRG_UCLASS_NBLOCKS (\d+)", text).group(1))
    return text, init("MRG_UCLASS_STAGE1_INIT"), init("MRG_UCLASS_STAGE2_INIT"), nblocks


def test_fixture_matches_product_table():
    """uclass_table.inc as text, looked up for every codepoint by the formula its header comment gives: the
    comment must state FORMULA word for word, and the same formula is written out in numpy below."""
    text, stage1, stage2, nblocks = parse_table()
    assert "// " + FORMULA + "\n" in text, "the header comment of uclass_table.inc no longer states this formula"
    assert stage1.size == 0x1100 and stage2.size == nblocks * 64 and stage1.max() == nblocks - 1
    assert stage2.min() >= 0 and stage2.max() < 256
    cp = np.arange(0x110000, dtype=np.int64)
    got = (stage2[stage1[cp >> 8] * 64 + ((cp & 255) >> 2)] >> (2 * (cp & 3))) & 3
    assert first_diff(got, U.classes()) is None
    assert (got[0xD800:0xE000] == 0).all()


def test_fixture_matches_oracle_class_everywhere():
    f = O.lib().oracle_class
    got = np.fromiter((f(c) for c in range(0x110000)), dtype=np.uint8, count=0x110000)
    assert first_diff(got, U.classes()) is None


def test_fixture_matches_live_regex():
    regex = pytest.importorskip("regex")
    want = U.fixture()["regex_version"]
    if regex.__version__ != want:
        pytest.skip(f"regex {regex.__version__} is installed; the fixture records {want}")
    w, s = regex.compile(r"\w"), regex.compile(r"\s")
    got = np.zeros(0x110000, dtype=np.uint8)
    for c in scalars().tolist():
        ch = chr(c)
        got[c] = 2 if s.match(ch) else (1 if w.match(ch) else 0)
    assert first_diff(got, U.classes()) is None


def test_white_space_and_join_control():
    """White_Space is exactly the standard's 25 scalars (stable since Unicode 6.3); Join_Control is W."""
    cls = U.classes()
    assert sorted(np.nonzero(cls == U.S)[0].tolist()) == sorted(WHITE_SPACE) and len(WHITE_SPACE) == 25
    assert all(cls[c] == U.W for c in JOIN_CONTROL)


def test_fixture_against_unicodedata():
    """An independent source: every scalar assigned in the stdlib's Unicode version with category L*, M*, Nd
    or Pc is W (all of these are in \\w by UTS#18); none of category P* (but Pc), Z*, Cc, Sm, Sc or Sk is W.
    The general category of an assigned character may change between versions, so the rules are applied
    only while the stdlib's version is not newer than the fixture's."""
    cls = U.classes()
    ver = tuple(int(x) for x in unicodedata.unidata_version.split("."))
    if ver > tuple(int(x) for x in U.fixture()["unicode_version"].split(".")):
        pytest.skip(f"unicodedata {unicodedata.unidata_version} is newer than the fixture's Unicode "
                    f"{U.fixture()['unicode_version']}: regenerate the fixture")
    must, never = [], []
    for c in scalars().tolist():
        cat = unicodedata.category(chr(c))
        if cat[0] in "LM" or cat in ("Nd", "Pc"):
            if cls[c] != U.W:
                must.append(hex(c))
        elif (cat[0] in "PZ" or cat in ("Cc", "Sm", "Sc", "Sk")) and cls[c] == U.W:
            never.append(hex(c))
    assert not must and not never, (must[:10], never[:10])


def test_boundary_set():
    b = U.boundary_set()
    assert 2000 < len(b) < 10000 and list(b) == sorted(set(b))
    assert all(c in b for c in U.SEAMS) and not any(U.is_surrogate(c) for c in b)
    for a, _ in U.fixture()["runs"]:
        for c in (a - 1, a):
            assert c in b or c < 0 or U.is_surrogate(c)
    assert {int(k) for k in set(U.classes()[list(b)])} == {0, 1, 2}


def test_sweep_by_construction_matches_oracle():
    docs, toks = U.full_sweep()
    assert len(docs) == 17 and sum(map(len, docs)) == 12_164_720 and sum(map(len, toks)) == 1_112_089
    for p in range(17):
        got = O.tokens(docs[p])
        assert len(got) == len(toks[p]), p
        bad = [i for i in range(len(got)) if got[i] != toks[p][i]]
        assert not bad, (p, toks[p][bad[0]], got[bad[0]], len(bad))
    exp = U.lines(toks)
    assert exp[-1].startswith(b"z ") and exp[-1] == b"z 25\n"
    assert O.wc(docs, 1, O.FAST)[0] + exp[-1] == b"".join(exp)       # R = 1: the oracle drops the last group


def test_sweep_with_prefix_matches_oracle():
    pre = b"L" * 14
    doc, toks = U.sweep(U.boundary_set(), pre)
    assert O.tokens(doc) == toks
    # all keys are long (> 16 bytes) but the "z" after an S scalar and the keys of a few scalars below U+0100
    short = [t for t in toks if len(t) <= 16]
    assert len(short) < 40 and all(t == b"z" or int(t[14:].rstrip(b"z"), 16) < 0x100 for t in short)


def oracle_error(doc):
    at = ctypes.c_size_t(0xDEAD)
    rc = O.lib().oracle_validate_utf8(doc, len(doc), ctypes.byref(at))
    return None if rc == 0 else at.value


def test_matrix_references_agree():
    m = U.utf8_matrix()
    assert len(m) == 1611 and len(set(m)) == len(m) and all(len(q) == 4 for q in m)
    invalid = [q for q in m if U.py_error(q) is not None]
    assert len(invalid) == 1497
    assert {q[0] for q in m} == set(U.M_B0) and {q[0] for q in U.utf8_matrix_thin()} == set(U.M_B0)
    for q in m:
        for doc in (q, U.embed(q)):
            assert U.py_error(doc) == oracle_error(doc), doc
        if U.py_error(q) is not None:
            assert 6 <= U.py_error(U.embed(q)) <= 9, q
    for t in U.TRUNCATED:
        for doc in (t, b"ab cd " + t, b"x" * 2047 + t):
            assert U.py_error(doc) == oracle_error(doc) == len(doc) - len(t), doc
