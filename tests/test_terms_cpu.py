"""CPU tests of mrg_vocab_term_counts at the ABI boundary: the symbol and mrg_terms_info are exported and
bound, the header and the Rust declarations carry it, a NULL context comes back as MRG_EINVAL with a
message (never a crash), and the numpy helper that the GPU tests take their expected rows from equals a
plain collections.Counter implementation.  No GPU is needed: every call here fails before it reaches
the device."""
import ctypes as C
import os
import random
import re

import numpy as np

from terms_util import UNK, expected_rows, expected_rows_counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib():
    from mapreduce_rust_amd import native
    return native.load()


def test_header_and_rust_declare_it():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_term_counts" in hdr
    assert "#define MRG_ABI_VERSION 6" in hdr
    c = re.search(r"^int mrg_vocab_term_counts\(([^)]*)\);", hdr, re.M)
    r = re.search(r"pub fn mrg_vocab_term_counts\(([^)]*)\) -> c_int;", rs, re.S)
    assert c and r
    assert c.group(1).count(",") + 1 == 10 == r.group(1).count(",") + 1
    assert "mrg_terms_info" not in hdr                       # a diagnostic, like mrg_decode_info


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    assert hasattr(raw, "mrg_vocab_term_counts") and hasattr(raw, "mrg_terms_info")
    assert "mrg_vocab_term_counts" in native.exported_symbols()
    assert lib().mrg_vocab_term_counts.restype is C.c_int and len(lib().mrg_vocab_term_counts.argtypes) == 10
    for m in ("term_counts", "terms_info"):
        assert callable(getattr(M.Context, m))
    assert b"abi 6" in lib().mrg_version()


def test_constants_mirror_the_device_header():
    from mapreduce_rust_amd import native
    dev = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "mrg_device.h")).read()
    for name in ("TERMS_WAVE_MAX", "TERMS_WG_MAX"):
        m = re.search(r"^#define MRG_%s (\d+)u$" % name, dev, re.M)
        assert m and int(m.group(1)) == getattr(native, name), name
    assert 64 <= native.TERMS_WAVE_MAX < native.TERMS_WG_MAX


def test_null_context():
    from mapreduce_rust_amd import native
    L = lib()
    tok = (C.c_uint64 * 2)(0, 3)
    off = (C.c_uint64 * 2)(7, 7)
    unk = (C.c_uint64 * 1)(7)
    assert L.mrg_vocab_term_counts(None, None, None, tok, 1, None, None, 0, off, unk) == native.EINVAL
    assert "context" in L.mrg_last_error().decode()
    assert list(off) == [7, 7] and list(unk) == [7]
    assert L.mrg_vocab_term_counts(None, None, None, None, 1, None, None, 0, None, None) == native.EINVAL
    assert L.mrg_last_error().decode()
    f = L.mrg_terms_info
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    assert f(None, None, None) == native.EINVAL and "context" in L.mrg_last_error().decode()


def test_numpy_helper_equals_counter():
    rng = random.Random(20261020)
    for case in range(200):
        n_words = rng.choice((1, 2, 3, 10, 1000))
        n_docs = rng.randrange(0, 6)
        first = rng.randrange(0, 4)
        tok = [first]
        for _ in range(n_docs):
            tok.append(tok[-1] + rng.choice((0, 0, 1, 2, 5, 17, 40)))
        p_unk = rng.choice((0.0, 0.1, 0.9, 1.0))
        ids = [UNK if rng.random() < p_unk else rng.randrange(n_words) for _ in range(tok[-1] + 2)]
        off, terms, counts, unk = expected_rows(np.array(ids, dtype=np.uint32), tok)
        e_off, e_terms, e_counts, e_unk = expected_rows_counter(ids, tok)
        assert off == e_off and unk == e_unk, case
        assert terms.dtype == np.uint32 and counts.dtype == np.uint32
        assert terms.tolist() == e_terms and counts.tolist() == e_counts, case
        assert UNK not in terms.tolist()
        for d in range(n_docs):
            assert sum(e_counts[off[d]:off[d + 1]]) + unk[d] == tok[d + 1] - tok[d]
