"""CPU tests of mrg_vocab_postings_merge at the ABI boundary -- the symbol is exported, bound and declared with
matching arity, the tile constant mirrors the device header, a NULL context comes back as MRG_EINVAL with a
message -- and of the helper the GPU tests rest on (tests/pmerge_util.py): the merge of the shards of a CSR, cut on
the host, is the index of the CSR in one piece.  No GPU is needed: every call here fails before it reaches the
device."""
import ctypes as C
import os
import re

import numpy as np

from pmerge_util import expected_merge, synth_shard
from postings_util import expected_postings
from shard_util import split_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, ARITY = "mrg_vocab_postings_merge", 12
N_WORDS = 120


def lib():
    from mapreduce_rust_amd import native
    return native.load()


# ---- the ABI

def test_header_and_rust_declare_it():
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert "(6, additive): mrg_vocab_postings_merge" in hdr and "#define MRG_ABI_VERSION 6" in hdr
    c = re.search(r"^int %s\(([^)]*)\);" % NAME, hdr, re.M)
    r = re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % NAME, rs, re.S)
    assert c and r
    assert c.group(1).count(",") + 1 == ARITY == r.group(1).count(",") + 1


def test_symbol_exported_and_bound():
    import mapreduce_rust_amd as M
    from mapreduce_rust_amd import native
    raw = C.CDLL(M.lib_path())
    assert hasattr(raw, NAME) and hasattr(raw, "mrg_postings_merge_info")
    assert NAME in native.exported_symbols()
    f = getattr(lib(), NAME)
    assert f.restype is C.c_int and len(f.argtypes) == ARITY
    for m in ("postings_merge", "postings_merge_info"):
        assert callable(getattr(M.Context, m))
    assert b"abi 6" in lib().mrg_version()


def test_tile_mirrors_the_device_header():
    from mapreduce_rust_amd import native
    dev = open(os.path.join(ROOT, "mapreduce_rust_amd", "csrc", "mrg_device.h")).read()
    m = re.search(r"^#define MRG_PMERGE_TILE (\d+)u$", dev, re.M)
    assert m and int(m.group(1)) == native.PMERGE_TILE
    assert native.PMERGE_TILE % 1024 == 0                   # whole rounds of 256 threads x one 16-byte store


def test_null_context():
    from mapreduce_rust_amd import native
    L = lib()
    total = C.c_uint64(77)
    tab = (C.c_void_p * 1)(None)
    ent = (C.c_uint64 * 1)(0)
    assert L.mrg_vocab_postings_merge(None, None, 1, tab, tab, tab, ent, None, None, None, 0, C.byref(total)) == native.EINVAL
    assert "context" in L.mrg_last_error().decode() and total.value == 77
    assert L.mrg_vocab_postings_merge(None, None, 0, None, None, None, None, None, None, None, 0, None) == native.EINVAL
    assert L.mrg_last_error().decode()
    info, ms = (C.c_uint64 * 8)(), (C.c_double * 3)()
    L.mrg_postings_merge_info.restype = C.c_int
    L.mrg_postings_merge_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    assert L.mrg_postings_merge_info(None, info, ms) == native.EINVAL and "context" in L.mrg_last_error().decode()


# ---- the helper

def random_csr(seed, n_docs=300, n_words=N_WORDS):
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n_words - 1, rng.integers(0, 14), replace=False)) for _ in range(n_docs)]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    terms = np.concatenate(rows).astype(np.uint32)
    counts = rng.integers(0, 9, len(terms)).astype(np.uint32)   # 0 included: copied as it is
    return terms, counts, row_off, np.zeros(n_docs, dtype=np.uint32)


def test_merge_of_the_shards_of_a_csr_is_the_index_in_one_piece():
    for seed, base in ((1, 0), (2, 7)):
        csr = random_csr(seed)
        terms, counts, row_off, _ = csr
        whole = expected_postings(terms, counts, row_off, N_WORDS, base)
        for cuts in ([0, 1, 64, 64, 300], [0, 300], [0, 0, 299, 300]):   # a one-row and an empty shard
            shards = split_host(csr, cuts, N_WORDS, base)
            assert any(len(s[3]) == 1 for s in shards) or len(cuts) == 2
            got = expected_merge(shards, N_WORDS)
            for g, w in zip(got, whole):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (seed, cuts)
        # the order of the shards matters: the helper is sensitive to it
        a, b = split_host(csr, [0, 150, 300], N_WORDS, base)
        assert expected_merge([b, a], N_WORDS)[1].tobytes() != whole[1].tobytes()


def test_merge_of_synthetic_shards_by_a_dict_of_lists():
    rng = np.random.default_rng(3)
    n_words = 9
    shards = [synth_shard(rng, rng.integers(0, 6, n_words), 100 * s, 50) for s in range(4)]
    shards.insert(2, synth_shard(rng, np.zeros(n_words, dtype=np.int64), 0, 1))   # an empty shard
    po, docs, tf = expected_merge(shards, n_words)
    want_d, want_f, want_po = [], [], [0]
    for w in range(n_words):
        for o, d, f in shards:
            want_d += [int(x) for x in d[int(o[w]):int(o[w + 1])]]
            want_f += [int(x) for x in f[int(o[w]):int(o[w + 1])]]
        want_po.append(len(want_d))
    assert po.tolist() == want_po and docs.tolist() == want_d and tf.tolist() == want_f
    for w in range(n_words):                                 # ascending shard ranges: every merged word ascends strictly
        lst = docs[int(po[w]):int(po[w + 1])].astype(np.int64)
        assert (np.diff(lst) > 0).all()
