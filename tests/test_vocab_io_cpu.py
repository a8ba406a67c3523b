"""CPU tests of mrg_vocab_from_text / mrg_vocab_decode at the ABI boundary: both symbols are exported
and bound, bad arguments come back as MRG_EINVAL with a message (never a crash), *out is NULL on failure,
and the header and the Rust declarations carry them.  No GPU is needed: every call here fails before it
reaches the device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mrg_vocab_from_text", "mrg_vocab_decode"]


def lib():
    from mapreduce_rust_amd import native
    return native.load()


def last_error():
    return lib().mrg_last_error().decode()


def test_symbols_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    for f in NEW:
        assert hasattr(raw, f), f
        assert f in native.exported_symbols()
        assert getattr(lib(), f).restype is C.c_int
    assert len(lib().mrg_vocab_from_text.argtypes) == 5 and len(lib().mrg_vocab_decode.argtypes) == 10
    for m in ("vocab_from_text", "vocab_load", "decode"):
        assert callable(getattr(M.Context, m))
    assert callable(M.Vocab.save)
    assert b"abi 6" in lib().mrg_version()


def test_from_text_null_arguments():
    from mapreduce_rust_amd import native
    L = lib()
    out = C.c_void_p(0xDEAD)
    assert L.mrg_vocab_from_text(None, b"a 1\n", 4, 0, C.byref(out)) == native.EINVAL
    assert out.value is None, "*out must be NULL on failure"
    assert "context" in last_error()
    assert L.mrg_vocab_from_text(None, b"a 1\n", 4, 0, None) == native.EINVAL
    assert last_error()
    out = C.c_void_p(0xDEAD)
    assert L.mrg_vocab_from_text(None, None, 0, 0, C.byref(out)) == native.EINVAL    # an empty text still needs a context
    assert out.value is None and last_error()


def test_decode_null_arguments():
    from mapreduce_rust_amd import native
    L = lib()
    tok = (C.c_uint64 * 2)(0, 0)
    off = (C.c_uint64 * 2)(7, 7)
    assert L.mrg_vocab_decode(None, None, None, tok, 1, None, 0, None, 0, off) == native.EINVAL
    assert "context" in last_error()
    assert list(off) == [7, 7]
    assert L.mrg_vocab_decode(None, None, None, None, 1, None, 0, None, 0, None) == native.EINVAL
    assert last_error()


def test_header_and_rust_declare_them():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_from_text, mrg_vocab_decode" in hdr
    assert "#define MRG_ABI_VERSION 6" in hdr
    for f, arity in (("mrg_vocab_from_text", 5), ("mrg_vocab_decode", 10)):
        c = re.search(r"^int %s\(([^)]*)\);" % f, hdr, re.M)
        r = re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % f, rs, re.S)
        assert c and r, f
        assert c.group(1).count(",") + 1 == arity == r.group(1).count(",") + 1
