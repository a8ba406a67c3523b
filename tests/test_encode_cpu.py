"""CPU tests of the vocabulary / encode surface (mrg_job_vocab, mrg_vocab_*): the symbols are
exported and bound, and null arguments come back as MRG_EINVAL with a message, never an abort."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["mrg_job_vocab", "mrg_vocab_size", "mrg_vocab_copy_text", "mrg_vocab_free", "mrg_vocab_encode"]
EINVAL = -1


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    lib = C.CDLL(M.lib_path())
    for f in FIVE:
        assert hasattr(lib, f), f
        assert f in native.exported_symbols(), f
    assert hasattr(lib, "mrg_encode_info")          # diagnostics, not in the header
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    assert "mrg_encode_info" not in hdr
    assert re.search(r"^#define MRG_ID_UNK 0xFFFFFFFFu", hdr, re.M)
    assert native.ID_UNK == M.ID_UNK == 0xFFFFFFFF
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "pub const MRG_ID_UNK: u32 = 0xFFFF_FFFF;" in rs


def test_null_arguments_are_einval():
    from mapreduce_rust_amd import native
    L = native.load()
    L.mrg_vocab_free(None)                          # a no-op
    n, b = C.c_uint64(7), C.c_uint64(7)
    assert L.mrg_vocab_size(None, C.byref(n), C.byref(b)) == EINVAL
    assert L.mrg_last_error()
    out = C.c_void_p(1234)
    assert L.mrg_job_vocab(None, 10, 1, C.byref(out)) == EINVAL
    assert L.mrg_last_error() and out.value is None  # *out is NULL on failure
    assert L.mrg_job_vocab(None, 10, 1, None) == EINVAL
    off = (C.c_uint64 * 2)(0, 0)
    tok = (C.c_uint64 * 2)()
    assert L.mrg_vocab_encode(None, None, None, off, 1, None, 0, tok) == EINVAL
    assert L.mrg_last_error()
    assert L.mrg_vocab_copy_text(None, None, 0) == EINVAL
