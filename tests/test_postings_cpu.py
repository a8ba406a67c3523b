"""CPU tests of mrg_vocab_postings at the ABI boundary: the symbol and mrg_postings_info are exported and
bound, the header and the Rust declarations carry it, the two constants mirror the device header, a NULL
context comes back as MRG_EINVAL with a message (never a crash), and the numpy helper that the GPU tests
take their expected index from equals a plain dict-of-lists implementation.  No GPU is needed: every call
here fails before it reaches the device."""
import ctypes as C
import os
import random
import re

import numpy as np

from postings_util import expected_postings, expected_postings_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    from mapreduce_rust_amd import native
    return native.load()


def test_header_and_rust_declare_it():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_postings" in hdr
    assert "#define MRG_ABI_VERSION 6" in hdr
    c = re.search(r"^int mrg_vocab_postings\(([^)]*)\);", hdr, re.M)
    r = re.search(r"pub fn mrg_vocab_postings\(([^)]*)\) -> c_int;", rs, re.S)
    assert c and r
    assert c.group(1).count(",") + 1 == 12 == r.group(1).count(",") + 1
    assert "mrg_postings_info" not in hdr                    # a diagnostic, like mrg_terms_info


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    assert hasattr(raw, "mrg_vocab_postings") and hasattr(raw, "mrg_postings_info")
    assert "mrg_vocab_postings" in native.exported_symbols()
    assert lib().mrg_vocab_postings.restype is C.c_int and len(lib().mrg_vocab_postings.argtypes) == 12
    for m in ("postings", "postings_info"):
        assert callable(getattr(M.Context, m))
    assert b"abi 6" in lib().mrg_version()


def test_constants_mirror_the_device_header():
    from mapreduce_rust_amd import native
    dev = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "mrg_device.h")).read()
    for name in ("POST_LDS_WORDS", "POST_TILE"):
        m = re.search(r"^#define MRG_%s (\d+)u$" % name, dev, re.M)
        assert m and int(m.group(1)) == getattr(native, name), name
    # 4 workgroups of the count kernel per CU: 4 histograms of 4-byte bins in 160 KiB of LDS
    assert 256 < native.POST_LDS_WORDS and 4 * 4 * native.POST_LDS_WORDS <= 160 * 1024
    assert native.POST_TILE % 256 == 0


def test_null_context():
    from mapreduce_rust_amd import native
    L = lib()
    off = (C.c_uint64 * 2)(0, 3)
    ent = C.c_uint64(7)
    assert L.mrg_vocab_postings(None, None, None, None, off, 1, 0, None, None, None, 0, C.byref(ent)) == native.EINVAL
    assert "context" in L.mrg_last_error().decode()
    assert ent.value == 7 and list(off) == [0, 3]
    assert L.mrg_vocab_postings(None, None, None, None, None, 1, 0, None, None, None, 0, None) == native.EINVAL
    assert L.mrg_last_error().decode()
    f = L.mrg_postings_info
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    assert f(None, None, None) == native.EINVAL and "context" in L.mrg_last_error().decode()


def test_numpy_helper_equals_dict():
    rng = random.Random(20261020)
    seen = {"dup": 0, "unsorted": 0, "empty_row": 0, "first": 0, "base": 0}
    for case in range(200):
        n_words = rng.choice((1, 2, 3, 10, 1000))
        n_docs = rng.randrange(0, 7)
        first = rng.randrange(0, 4)
        doc_base = rng.choice((0, 0, 5, 2**32 - n_docs))
        row_off = [first]
        for _ in range(n_docs):
            row_off.append(row_off[-1] + rng.choice((0, 0, 1, 2, 5, 17)))
        n = row_off[-1] + 2                                  # two entries after the range, `first` before it
        terms = [rng.randrange(n_words) for _ in range(n)]   # any order inside a row, duplicates included
        counts = [rng.choice((0, 1, 2, 0xFFFFFFFF, rng.randrange(1 << 32))) for _ in range(n)]
        for i in range(n_docs):
            row = terms[row_off[i]:row_off[i + 1]]
            seen["dup"] += len(set(row)) < len(row)
            seen["unsorted"] += row != sorted(row)
            seen["empty_row"] += not row
        seen["first"] += first > 0
        seen["base"] += doc_base > 0
        off, docs, tf = expected_postings(np.array(terms, dtype=np.uint32), np.array(counts, dtype=np.uint32), row_off,
                                          n_words, doc_base)
        e_off, e_docs, e_tf = expected_postings_dict(terms, counts, row_off, n_words, doc_base)
        assert off.dtype == np.uint64 and docs.dtype == np.uint32 and tf.dtype == np.uint32
        assert off.tolist() == e_off and docs.tolist() == e_docs and tf.tolist() == e_tf, case
        assert off[0] == 0 and off[-1] == row_off[-1] - row_off[0] and len(off) == n_words + 1
        for w in range(n_words):                             # the documents of a word never descend
            d = e_docs[e_off[w]:e_off[w + 1]]
            assert d == sorted(d)
    assert all(v > 10 for v in seen.values()), seen
