"""ctypes binding of libmrgpu.so (include/mrgpu.h).  No CPU fallback: a missing library raises.

Every entry point of the C ABI is bound here with its exact signature; MrgError carries the
status code and mrg_last_error() text.  Device buffers are passed as raw device pointers (ints);
callers typically own them as torch CUDA tensors (plumbing only, never in the ABI).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

APP_WC = 0
APP_INDEXER = 1
FLAG_NO_COMPAT_DROP_LAST = 0x1
FLAG_FINAL_TXT = 0x2
FLAG_STREAM = 0x4  # run_job only: map each GPU's files in batches while the next batch is read
XREC_BYTES = 24  # include/mrgpu.h MRG_XREC_BYTES (ABI 3)
ABI_VERSION = 6  # include/mrgpu.h MRG_ABI_VERSION
ID_UNK = 0xFFFFFFFF  # MRG_ID_UNK: mrg_vocab_encode's id of a word that is not in the vocabulary

OK, EINVAL, EUTF8, EHIP, ENOMEM, EIO, ECOMM = 0, -1, -2, -3, -4, -5, -6
_CODES = {EINVAL: "EINVAL", EUTF8: "EUTF8", EHIP: "EHIP", ENOMEM: "ENOMEM", EIO: "EIO", ECOMM: "ECOMM"}
COMM_ID_BYTES = 128
# term_counts: the longest document (in ids) sorted by one wave / by one workgroup (MRG_TERMS_WAVE_MAX,
# MRG_TERMS_WG_MAX of csrc/mrg_device.h); longer ones take the radix-sort path
TERMS_WAVE_MAX = 256
TERMS_WG_MAX = 4096
# postings: terms below POST_LDS_WORDS are counted in LDS, the others with global atomics; one workgroup
# finds the rows of POST_TILE consecutive entries (MRG_POST_LDS_WORDS, MRG_POST_TILE of csrc/mrg_device.h)
POST_LDS_WORDS = 8192
POST_TILE = 2048
# search: one workgroup accumulates the postings of a query position inside one window of SEARCH_TILE postings;
# a query returns at most SEARCH_MAX_K documents (MRG_SEARCH_TILE, MRG_SEARCH_MAX_K of csrc/mrg_device.h)
SEARCH_TILE = 4096
SEARCH_MAX_K = 1024
# search_merge: at most SEARCH_MAX_SHARDS rows per query; they are staged in LDS when n_shards * k_in is at most
# MERGE_LDS_KEYS, and read from global memory otherwise (MRG_SEARCH_MAX_SHARDS, MRG_MERGE_LDS_KEYS of csrc/mrg_device.h)
SEARCH_MAX_SHARDS = 64
# search_bool: the role of a query position (MRG_Q_SHOULD, MRG_Q_MUST, MRG_Q_MUST_NOT of include/mrgpu.h)
Q_SHOULD, Q_MUST, Q_MUST_NOT = 0, 1, 2
MERGE_LDS_KEYS = 8192
# postings_merge: one workgroup copies PMERGE_TILE consecutive entries of one shard (MRG_PMERGE_TILE of
# csrc/mrg_device.h)
PMERGE_TILE = 2048


def debug_hash_bits(n):
    """MRG_FLAG_DEBUG_HASH_BITS(n): truncate internal hashes to n bits (forces collisions)."""
    return (n & 0xFF) << 8


def flag_top(k):
    """MRG_FLAG_TOP(k): run_job also writes out_dir/top.txt, the k (1..65535) most frequent lines."""
    return (k & 0xFFFF) << 16


def kernel_source_sha():
    """sha256 over the sources libmrgpu.so is built from (kernels, headers, host layer): keys the
    committed PMC traffic figure (profiles/map_traffic.json) to the code it was measured on."""
    import hashlib
    d = os.path.join(_HERE, "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".inc", ".cpp")) and f != "mrgpu_cli.cpp":
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def lib_path():
    return os.environ.get("MRG_LIB", os.path.join(_HERE, "lib", "libmrgpu.so"))


class MrgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_CODES.get(code, code)}: {msg}")
        self.code = code


class Stats(C.Structure):
    _fields_ = [("input_bytes", C.c_uint64), ("tokens", C.c_uint64), ("long_tokens", C.c_uint64),
                ("map_records", C.c_uint64), ("distinct_keys", C.c_uint64), ("output_bytes", C.c_uint64),
                ("ms_map", C.c_double), ("ms_aggregate", C.c_double), ("ms_sort", C.c_double),
                ("ms_format", C.c_double), ("map_launches", C.c_uint32), ("agg_launches", C.c_uint32),
                ("overflow_keys", C.c_uint64), ("ms_exchange", C.c_double), ("exchange_sent", C.c_uint64),
                ("exchange_recv", C.c_uint64), ("map_spill", C.c_uint64),
                ("nonascii_tiles", C.c_uint64), ("tail_records_16", C.c_uint64), ("spec_agg", C.c_uint32),
                ("agg_path", C.c_uint32), ("map_kind", C.c_uint32), ("map_batches", C.c_uint32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class RunStats(C.Structure):
    """mrg_run_stats: wall-clock phases of the last mrg_run_job on this thread."""
    _fields_ = [("ms_total", C.c_double), ("ms_open", C.c_double), ("ms_read", C.c_double), ("ms_map", C.c_double),
                ("ms_shuffle", C.c_double), ("ms_reduce", C.c_double), ("ms_write", C.c_double),
                ("input_bytes", C.c_uint64), ("output_bytes", C.c_uint64), ("n_gpus", C.c_int),
                ("ms_map_alloc", C.c_double), ("ms_map_kernel", C.c_double), ("ms_aggregate_kernel", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None
_vp = C.c_void_p
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)

_SIGS = {
    "mrg_last_error": (C.c_char_p, []),
    "mrg_version": (C.c_char_p, []),
    "mrg_open": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mrg_close": (C.c_int, [_vp]),
    "mrg_set_stream": (C.c_int, [_vp, _vp]),
    "mrg_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mrg_set_timing": (C.c_int, [_vp, C.c_int]),
    "mrg_job_begin": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32]),
    "mrg_job_set_doc_names": (C.c_int, [_vp, C.POINTER(C.c_char_p), C.c_uint32]),
    "mrg_job_set_input": (C.c_int, [_vp, _vp, _u64p, C.c_uint32, _u32p]),
    "mrg_job_map": (C.c_int, [_vp]),
    "mrg_job_map_add": (C.c_int, [_vp]),
    "mrg_job_export_sizes": (C.c_int, [_vp, C.c_uint32, _u64p, _u64p]),
    "mrg_job_export": (C.c_int, [_vp, _vp, _vp]),
    "mrg_job_import": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p, C.c_uint32]),
    "mrg_job_reduce": (C.c_int, [_vp, _u64p]),
    "mrg_job_output": (C.c_int, [_vp, C.POINTER(_vp), _u64p]),
    "mrg_job_copy_output": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrg_job_final": (C.c_int, [_vp, C.POINTER(_vp), _u64p]),
    "mrg_job_copy_final": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrg_job_topk": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp), _u64p, _u64p]),
    "mrg_job_copy_topk": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrg_job_vocab": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "mrg_vocab_size": (C.c_int, [_vp, _u64p, _u64p]),
    "mrg_vocab_copy_text": (C.c_int, [_vp, _vp, C.c_uint64]),
    "mrg_vocab_free": (None, [_vp]),
    "mrg_vocab_encode": (C.c_int, [_vp, _vp, _vp, _u64p, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "mrg_vocab_from_text": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "mrg_vocab_decode": (C.c_int, [_vp, _vp, _vp, _u64p, C.c_uint32, C.c_char_p, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "mrg_vocab_term_counts": (C.c_int, [_vp, _vp, _vp, _u64p, C.c_uint32, _vp, _vp, C.c_uint64, _u64p, _u64p]),
    "mrg_vocab_postings": (C.c_int, [_vp, _vp, _vp, _vp, _u64p, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _u64p]),
    "mrg_vocab_search": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, _u64p, C.c_uint32,
                                   C.c_float, C.c_float, C.c_uint32, _vp, _vp, _u32p]),
    "mrg_vocab_stats_add": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _u64p]),
    "mrg_vocab_search_shard": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64,
                                         C.c_uint64, _vp, _u64p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, _vp, _vp, _u32p]),
    "mrg_vocab_search_bool": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, C.c_char_p, _u64p,
                                        C.c_uint32, C.c_float, C.c_float, C.c_uint32, _vp, _vp, _u32p]),
    "mrg_vocab_search_bool_shard": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64,
                                              C.c_uint64, _vp, C.c_char_p, _u64p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                              _vp, _vp, _u32p]),
    "mrg_search_merge": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _u32p, C.c_uint32, _vp, _vp, _u32p]),
    "mrg_vocab_postings_merge": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _u64p, _vp, _vp,
                                           _vp, C.c_uint64, _u64p]),
    "mrg_map": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                          C.POINTER(_vp)]),
    "mrg_parts_get": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp), _u64p, C.POINTER(_vp), _u64p]),
    "mrg_parts_free": (None, [_vp]),
    "mrg_reduce": (C.c_int, [_vp, C.c_int, C.c_uint32, C.POINTER(_vp), C.c_size_t, C.c_uint32, C.c_uint32,
                             C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "mrg_map_text": (C.c_int, [_vp, C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(_vp), _u64p]),
    "mrg_reduce_text": (C.c_int, [_vp, C.POINTER(C.c_char_p), _u64p, C.c_size_t, C.c_uint32, C.POINTER(_vp),
                                  C.POINTER(C.c_size_t)]),
    "mrg_run_job": (C.c_int, [C.POINTER(C.c_char_p), C.c_size_t, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32,
                              C.c_int]),
    "mrg_run_get_stats": (C.c_int, [C.POINTER(RunStats)]),
    "mrg_run_get_stream_stats": (C.c_int, [_u32p, _u64p]),
    "mrg_comm_get_id": (C.c_int, [_vp]),
    "mrg_comm_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "mrg_comm_destroy": (C.c_int, [_vp]),
    "mrg_job_shuffle": (C.c_int, [_vp, _vp]),
    "mrg_comm_count": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "mrg_pool_stats": (C.c_int, [_vp, _u64p, _u64p]),
    "mrg_pool_alloc_stats": (C.c_int, [_vp, _u64p, _u64p, C.POINTER(C.c_double)]),
    "mrg_free": (None, [_vp]),
    "mrg_gen_zipf": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double]),
    "mrg_gen_unique": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "mrg_gen_text": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_uint32]),
}


def load():
    """Load libmrgpu.so and bind every exported entry point (raises if it is missing)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: when torch (the device-memory / stream / torch.distributed
        # plumbing) is present, import it first so libmrgpu.so binds to the libamdhip64.so.7 torch
        # already mapped (same soname) instead of loading a second runtime beside it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"libmrgpu.so not built ({path}); run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return list(_SIGS)


def _check(rc):
    if rc != OK:
        raise MrgError(rc, load().mrg_last_error().decode(errors="replace"))


def _u64arr(xs):
    return (C.c_uint64 * max(len(xs), 1))(*xs)


def _roles_arg(q_roles, q_off):
    """h_q_role of the Boolean searches: None, or one byte per query id up to q_off[-1]"""
    if q_roles is None:
        return None
    q_roles = bytes(q_roles)
    if len(q_roles) < q_off[-1]:
        raise ValueError(f"q_roles needs q_off[-1] = {q_off[-1]} entries (indexed like the query ids), has {len(q_roles)}")
    return q_roles


def clause_roles(tok_off):
    """The roles and query offsets of Boolean queries that were encoded as three consecutive "documents" each --
    the must, should and must-not texts of a query, any of them empty -- in one encode() call: tok_off is the
    3 * n_queries + 1 token offsets encode() returned.  Returns (roles, q_off): query q is the ids
    tok_off[3 q] .. tok_off[3 q + 3] with the roles by clause, as search_bool() takes them beside the ids
    encode() wrote.  No id is copied; the entries of roles below tok_off[0] are not read by the search."""
    tok_off = [int(x) for x in tok_off]
    if len(tok_off) < 1 or (len(tok_off) - 1) % 3:
        raise ValueError("tok_off needs 3 * n_queries + 1 entries: the must, should and must-not text of every query")
    roles = bytearray(tok_off[-1])
    for i in range(len(tok_off) - 1):
        if tok_off[i + 1] < tok_off[i]:
            raise ValueError(f"tok_off must be non-decreasing (entry {i})")
        role = (Q_MUST, Q_SHOULD, Q_MUST_NOT)[i % 3]
        roles[tok_off[i]:tok_off[i + 1]] = bytes([role]) * (tok_off[i + 1] - tok_off[i])
    return bytes(roles), tok_off[::3]


def _voc_info(name, ctx, info_keys, ms_keys):
    """One of the mrg_*_info diagnostics (not in include/mrgpu.h): 8 counters and len(ms_keys) HIP-event ms, as a
    dict under the given names."""
    f = getattr(load(), name)
    f.restype = C.c_int
    f.argtypes = [_vp, _u64p, C.POINTER(C.c_double)]
    info, ms = (C.c_uint64 * 8)(), (C.c_double * len(ms_keys))()
    _check(f(ctx.h, info, ms))
    return {**dict(zip(info_keys, info)), **dict(zip(ms_keys, ms))}


class Parts:
    """One map task's output (mrg_parts): per-partition exchange records + long-key heap."""

    def __init__(self, handle, n_reduce):
        self.h = handle
        self.n_reduce = n_reduce

    def get(self, r):
        L = load()
        rec, heap = _vp(), _vp()
        nrec, nheap = C.c_uint64(), C.c_uint64()
        _check(L.mrg_parts_get(self.h, r, C.byref(rec), C.byref(nrec), C.byref(heap), C.byref(nheap)))
        return (C.string_at(rec, nrec.value * XREC_BYTES) if nrec.value else b"",
                C.string_at(heap, nheap.value) if nheap.value else b"")

    def free(self):
        if self.h:
            load().mrg_parts_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Vocab:
    """mrg_vocab: words as ids 0..n-1, from a job's most frequent words (Context.vocab) or from
    "word count\\n" text (Context.vocab_from_text, Context.vocab_load).  Owns its device memory; outlives
    the job and the context that made it."""

    def __init__(self, handle):
        self.h = handle

    def size(self):
        """(words, bytes of the "word count\\n" text)"""
        n, b = C.c_uint64(), C.c_uint64()
        _check(load().mrg_vocab_size(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def text(self):
        """The "word count\\n" lines in id order (bytes)."""
        _, nb = self.size()
        buf = C.create_string_buffer(max(nb, 1))
        _check(load().mrg_vocab_copy_text(self.h, buf, nb))
        return buf.raw[:nb]

    def words(self):
        """The words in id order (list of bytes)."""
        return [ln.rsplit(b" ", 1)[0] for ln in self.text().split(b"\n") if ln]

    def save(self, path):
        """Write the text to a file that Context.vocab_load reads back, on any device."""
        with open(path, "wb") as f:
            f.write(self.text())

    def close(self):
        if self.h:
            load().mrg_vocab_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One mrg_ctx: a device, a stream, device workspaces, and the current job."""

    def __init__(self, device=0):
        L = load()
        h = _vp()
        _check(L.mrg_open(device, C.byref(h)))
        self.h = h
        self.device = device
        self.n_reduce = 0

    def close(self):
        if self.h:
            load().mrg_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_ptr):
        _check(load().mrg_set_stream(self.h, stream_ptr))

    def pool_stats(self):
        """mrg_pool_stats: (device blocks handed out and not returned, bytes the pool holds)."""
        n, b = C.c_uint64(), C.c_uint64()
        _check(load().mrg_pool_stats(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def pool_alloc_stats(self):
        """mrg_pool_alloc_stats: (hipMalloc calls, bytes, host ms spent in them) since the context opened."""
        n, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        _check(load().mrg_pool_alloc_stats(self.h, C.byref(n), C.byref(b), C.byref(ms)))
        return n.value, b.value, ms.value

    def set_timing(self, on=True):
        _check(load().mrg_set_timing(self.h, 1 if on else 0))

    def pool_fail(self, k):
        """mrg_test_pool_fail (tests of the error exits): the k-th device block this context asks its pool
        for from now on fails with ENOMEM, once; 0 disarms."""
        f = load().mrg_test_pool_fail
        f.restype = C.c_int
        f.argtypes = [_vp, C.c_uint64]
        _check(f(self.h, k))

    def stats(self):
        s = Stats()
        _check(load().mrg_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    # ---- device-resident job
    def job_begin(self, app, n_reduce, flags=0):
        _check(load().mrg_job_begin(self.h, app, n_reduce, flags))
        self.n_reduce = n_reduce

    def set_doc_names(self, names):
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        _check(load().mrg_job_set_doc_names(self.h, arr, len(names)))

    def set_input(self, dev_ptr, doc_off, doc_ids=None):
        if len(doc_off) < 1:
            raise ValueError("doc_off needs n_docs + 1 entries (at least [0])")
        n = len(doc_off) - 1
        off = _u64arr(doc_off)
        ids = (C.c_uint32 * max(n, 1))(*doc_ids) if doc_ids is not None else None
        _check(load().mrg_job_set_input(self.h, dev_ptr, off, n, ids))

    def map(self):
        _check(load().mrg_job_map(self.h))

    def map_add(self):
        """mrg_job_map_add: map the input set by set_input() and ADD its tokens to the job's keys.
        Repeat set_input() + map_add() per batch of whole documents; the consumers then see one map
        over all batches.  The batch's buffer may be overwritten once this returns."""
        _check(load().mrg_job_map_add(self.h))

    def acc_info(self):
        """Diagnostics of the map_add accumulator: table slots, short and long keys, long-key heap
        bytes, rehashes and batches so far, and the last batch's fold time (with set_timing)."""
        f = load().mrg_test_acc_info
        f.restype = C.c_int
        f.argtypes = [_vp, _u64p, C.POINTER(C.c_double)]
        info, ms = (C.c_uint64 * 6)(), C.c_double()
        _check(f(self.h, info, C.byref(ms)))
        return {"slots": info[0], "short_keys": info[1], "long_keys": info[2], "long_heap_bytes": info[3],
                "rehashes": info[4], "batches": info[5], "ms_fold": ms.value}

    def export_sizes(self, n_owners):
        rec = (C.c_uint64 * n_owners)()
        heap = (C.c_uint64 * n_owners)()
        _check(load().mrg_job_export_sizes(self.h, n_owners, rec, heap))
        return list(rec), list(heap)

    def export(self, d_rec, d_heap):
        _check(load().mrg_job_export(self.h, d_rec, d_heap))

    def import_(self, d_rec, n_rec, d_heap, heap_bytes, seg_recs=None, seg_heap=None):
        if seg_recs is None:
            _check(load().mrg_job_import(self.h, d_rec, n_rec, d_heap, heap_bytes, None, None, 0))
        else:
            _check(load().mrg_job_import(self.h, d_rec, n_rec, d_heap, heap_bytes, _u64arr(seg_recs),
                                         _u64arr(seg_heap), len(seg_recs)))

    def shuffle(self, comm):
        """mrg_job_shuffle: the exchange over RCCL (collective over comm's ranks)."""
        _check(load().mrg_job_shuffle(self.h, comm.h))

    def reduce(self):
        n = C.c_uint64()
        _check(load().mrg_job_reduce(self.h, C.byref(n)))
        return n.value

    def output(self):
        d = _vp()
        off = (C.c_uint64 * (self.n_reduce + 1))()
        _check(load().mrg_job_output(self.h, C.byref(d), off))
        return d.value, list(off)

    def copy_output(self):
        _, off = self.output()
        buf = C.create_string_buffer(max(off[-1], 1))
        _check(load().mrg_job_copy_output(self.h, buf, off[-1]))
        return buf.raw[:off[-1]], off

    def copy_output_to(self, host_ptr, n):
        """mrg_job_copy_output into caller memory (e.g. a pinned buffer) of at least n bytes."""
        _check(load().mrg_job_copy_output(self.h, C.c_void_p(host_ptr), n))

    def outputs(self):
        """mr-{r}.txt contents for every partition r."""
        data, off = self.copy_output()
        return [data[off[r]:off[r + 1]] for r in range(self.n_reduce)]

    def final(self):
        """final.txt (src/run.sh:16-20, LC_ALL=C) of this job, built on the device."""
        d = _vp()
        n = C.c_uint64()
        _check(load().mrg_job_final(self.h, C.byref(d), C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(load().mrg_job_copy_final(self.h, buf, n.value))
        return buf.raw[:n.value]

    def topk(self, k):
        """The k most frequent lines of final.txt (count descending, then key bytes), selected on the
        device without sorting the keys (mrg_job_topk); wc only."""
        d = _vp()
        n, lines = C.c_uint64(), C.c_uint64()
        _check(load().mrg_job_topk(self.h, k, C.byref(d), C.byref(n), C.byref(lines)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(load().mrg_job_copy_topk(self.h, buf, n.value))
        return buf.raw[:n.value]

    def topk_info(self):
        """Diagnostics of the last topk(): distinct keys, candidates the select kept, select passes
        run, candidates dropped as their partition's last key, and the bytes each pass read."""
        f = load().mrg_test_topk_info
        f.restype = C.c_int
        f.argtypes = [_vp, _u64p, _u64p]
        info, pb = (C.c_uint64 * 4)(), (C.c_uint64 * 24)()
        _check(f(self.h, info, pb))
        return {"n": info[0], "candidates": info[1], "passes": info[2], "dropped": info[3],
                "pass_bytes": [b for b in pb if b]}

    def vocab(self, max_words=0, min_count=1):
        """mrg_job_vocab: the job's max_words (0: all) most frequent words with at least min_count
        occurrences, as a Vocab whose ids are the ranks of topk(max_words); wc only."""
        h = _vp()
        _check(load().mrg_job_vocab(self.h, max_words, min_count, C.byref(h)))
        return Vocab(h)

    def encode(self, vocab, dev_ptr, doc_off, out_ptr=None, cap=0):
        """mrg_vocab_encode: the tokens of every document (layout of set_input) as vocabulary ids, in
        input order, into the device buffer out_ptr of cap uint32 (None: count only).  Returns tok_off:
        document i's ids are out[tok_off[i]:tok_off[i + 1]]; ID_UNK marks words not in the vocabulary."""
        if len(doc_off) < 1:
            raise ValueError("doc_off needs n_docs + 1 entries (at least [0])")
        n = len(doc_off) - 1
        tok = (C.c_uint64 * (n + 1))()
        _check(load().mrg_vocab_encode(self.h, vocab.h, dev_ptr, _u64arr(doc_off), n, out_ptr, cap, tok))
        return list(tok)

    def vocab_from_text(self, text, flags=0):
        """mrg_vocab_from_text: a Vocab on this context's device from "word count\\n" lines (bytes): the
        text of another Vocab, or the top.txt / final.txt of a word-count run_job.  Line i's word gets id i.
        flags: debug_hash_bits(n) only."""
        text = bytes(text)
        h = _vp()
        _check(load().mrg_vocab_from_text(self.h, text, len(text), flags, C.byref(h)))
        return Vocab(h)

    def vocab_load(self, path, flags=0):
        """vocab_from_text of a file's bytes (Vocab.save, top.txt, final.txt)."""
        with open(path, "rb") as f:
            return self.vocab_from_text(f.read(), flags)

    def decode(self, vocab, ids_ptr, tok_off, out_ptr=None, cap=0, unk=b""):
        """mrg_vocab_decode: the ids of every document (layout of encode's output: uint32 ids at the device
        pointer ids_ptr, document i = ids[tok_off[i]:tok_off[i + 1]]) as text on the device: each word and a
        ' ', a '\\n' after a document's last word.  Returns out_off (len(tok_off) entries): document i's
        text is out[out_off[i]:out_off[i + 1]].  out_ptr None: sizes only.  unk: the bytes written for
        ID_UNK (empty: ID_UNK is an error)."""
        if len(tok_off) < 1:
            raise ValueError("tok_off needs n_docs + 1 entries (at least [0])")
        n = len(tok_off) - 1
        off = (C.c_uint64 * (n + 1))()
        unk = bytes(unk)
        _check(load().mrg_vocab_decode(self.h, vocab.h, ids_ptr, _u64arr(tok_off), n, unk, len(unk), out_ptr, cap, off))
        return list(off)

    def decode_info(self):
        """Diagnostics of the last decode(): ids, output bytes, 256-id chunks, scratch bytes; HIP-event ms
        per pass and of the last vocab_from_text() (with set_timing)."""
        return _voc_info("mrg_decode_info", self, ("ids", "output_bytes", "chunks", "scratch_bytes"),
                         ("ms_count", "ms_offsets", "ms_emit", "ms_from_text"))

    def term_counts(self, vocab, ids_ptr, tok_off, terms_ptr=None, counts_ptr=None, cap=0):
        """mrg_vocab_term_counts: per-document term counts of the ids of every document (layout of decode's
        input) in CSR form: row i = the distinct ids of document i other than ID_UNK, ascending, in the device
        buffer terms_ptr, and their occurrences in counts_ptr (cap uint32 each; both None: sizes only).
        Returns (row_off, unk): row i is [row_off[i], row_off[i + 1]) of both buffers, unk[i] the ID_UNK of
        document i."""
        if len(tok_off) < 1:
            raise ValueError("tok_off needs n_docs + 1 entries (at least [0])")
        n = len(tok_off) - 1
        off, unk = (C.c_uint64 * (n + 1))(), (C.c_uint64 * max(n, 1))()
        _check(load().mrg_vocab_term_counts(self.h, vocab.h, ids_ptr, _u64arr(tok_off), n, terms_ptr, counts_ptr, cap,
                                            off, unk))
        return list(off), list(unk)[:n]

    def terms_info(self):
        """Diagnostics of the last term_counts(): ids, row entries, ID_UNK ids, documents taken by the wave,
        workgroup and large path, large-path slices, scratch bytes; HIP-event ms per phase (with set_timing)."""
        return _voc_info("mrg_terms_info", self, ("ids", "entries", "unk", "wave_docs", "wg_docs", "large_docs", "slices",
                                                  "scratch_bytes"),
                         ("ms_count_lds", "ms_count_large", "ms_emit_lds", "ms_emit_large"))

    def postings(self, vocab, terms_ptr, counts_ptr, row_off, post_off_ptr, docs_ptr=None, tf_ptr=None, cap=0, doc_base=0):
        """mrg_vocab_postings: the inverted index of a CSR in term_counts' layout (uint32 terms and counts at
        the device pointers, row i = [row_off[i], row_off[i + 1]), its document doc_base + i): post_off_ptr
        (uint64, the vocabulary's words + 1) receives the offsets, whose differences are the document
        frequencies; docs_ptr and tf_ptr (cap uint32 each) the documents of every word, ascending, and the
        term frequencies.  docs_ptr and tf_ptr None: document frequencies only; tf_ptr None: documents only.
        Returns the number of entries."""
        if len(row_off) < 1:
            raise ValueError("row_off needs n_docs + 1 entries (at least [0])")
        n = len(row_off) - 1
        e = C.c_uint64()
        _check(load().mrg_vocab_postings(self.h, vocab.h, terms_ptr, counts_ptr, _u64arr(row_off), n, doc_base,
                                         post_off_ptr, docs_ptr, tf_ptr, cap, C.byref(e)))
        return e.value

    def postings_info(self):
        """Diagnostics of the last postings(): entries, words, the largest document frequency, radix passes
        run, entries counted in LDS and with global atomics, scratch bytes; HIP-event ms per phase (with
        set_timing)."""
        return _voc_info("mrg_postings_info", self, ("entries", "words", "max_df", "passes", "lds_entries", "global_entries",
                                                     "scratch_bytes"),
                         ("ms_count", "ms_scan", "ms_pack", "ms_sort", "ms_unpack"))

    def search(self, vocab, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs, q_ids_ptr, q_off, k,
               top_docs_ptr, top_scores_ptr, k1=1.2, b=0.75, doc_base=0):
        """mrg_vocab_search: the k best documents of every query by BM25 over the index postings() wrote
        (post_off_ptr, docs_ptr, tf_ptr, its n_entries) for the documents doc_base .. doc_base + n_docs - 1, whose
        lengths in ids are the uint32 at doc_len_ptr.  Query q is the ids q_ids[q_off[q]:q_off[q + 1]] at the
        device pointer q_ids_ptr (encode's output for the query texts).  Returns top_n: row q of the results is
        top_docs[q * k:q * k + top_n[q]] (uint32) with top_scores (float32) at the same positions, by score
        descending, then document ascending; the rest of a row is not written."""
        if len(q_off) < 1:
            raise ValueError("q_off needs n_queries + 1 entries (at least [0])")
        n = len(q_off) - 1
        top = (C.c_uint32 * max(n, 1))()
        _check(load().mrg_vocab_search(self.h, vocab.h, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs,
                                       doc_base, q_ids_ptr, _u64arr(q_off), n, k1, b, k, top_docs_ptr, top_scores_ptr, top))
        return list(top)[:n]

    def stats_add(self, vocab, post_off_ptr, doc_len_ptr, n_docs, df_ptr, coll=(0, 0)):
        """mrg_vocab_stats_add: one shard's part of the collection statistics of a sharded search.  df_ptr (uint64,
        the vocabulary's words, zeroed before the first shard) receives the shard's document frequencies added in;
        coll = (documents, sum of the lengths) so far.  Returns the new coll."""
        h = (C.c_uint64 * 2)(int(coll[0]), int(coll[1]))
        _check(load().mrg_vocab_stats_add(self.h, vocab.h, post_off_ptr, doc_len_ptr, n_docs, df_ptr, h))
        return h[0], h[1]

    def search_shard(self, vocab, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs, q_ids_ptr, q_off, k,
                     top_docs_ptr, top_scores_ptr, df_ptr, coll, k1=1.2, b=0.75, doc_base=0):
        """mrg_vocab_search_shard: search() over one shard of a collection, scored with the collection's statistics:
        df_ptr and coll = (documents, sum of the lengths) as stats_add left them after the last shard.  The rows
        of the shards go through search_merge()."""
        if len(q_off) < 1:
            raise ValueError("q_off needs n_queries + 1 entries (at least [0])")
        n = len(q_off) - 1
        top = (C.c_uint32 * max(n, 1))()
        _check(load().mrg_vocab_search_shard(self.h, vocab.h, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs,
                                             doc_base, df_ptr, int(coll[0]), int(coll[1]), q_ids_ptr, _u64arr(q_off), n, k1, b,
                                             k, top_docs_ptr, top_scores_ptr, top))
        return list(top)[:n]

    def search_bool(self, vocab, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs, q_ids_ptr, q_roles, q_off, k,
                    top_docs_ptr, top_scores_ptr, k1=1.2, b=0.75, doc_base=0):
        """mrg_vocab_search_bool: search() with a role for every query position.  q_roles (bytes or a sequence of
        ints, indexed like the query ids: q_roles[j] belongs to q_ids[j]; None: all Q_SHOULD) holds Q_SHOULD,
        Q_MUST or Q_MUST_NOT.  A hit stands in the postings of every MUST word and of no MUST_NOT word; SHOULD and
        MUST positions score, MUST_NOT positions do not.  clause_roles() makes q_roles and q_off from encode()'s
        offsets."""
        if len(q_off) < 1:
            raise ValueError("q_off needs n_queries + 1 entries (at least [0])")
        n = len(q_off) - 1
        top = (C.c_uint32 * max(n, 1))()
        _check(load().mrg_vocab_search_bool(self.h, vocab.h, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs,
                                            doc_base, q_ids_ptr, _roles_arg(q_roles, q_off), _u64arr(q_off), n, k1, b, k,
                                            top_docs_ptr, top_scores_ptr, top))
        return list(top)[:n]

    def search_bool_shard(self, vocab, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr, n_docs, q_ids_ptr, q_roles,
                          q_off, k, top_docs_ptr, top_scores_ptr, df_ptr, coll, k1=1.2, b=0.75, doc_base=0):
        """mrg_vocab_search_bool_shard: search_bool() over one shard of a collection, scored with the collection's
        statistics as search_shard() is.  A shard filters its own documents; the rows go through search_merge()."""
        if len(q_off) < 1:
            raise ValueError("q_off needs n_queries + 1 entries (at least [0])")
        n = len(q_off) - 1
        top = (C.c_uint32 * max(n, 1))()
        _check(load().mrg_vocab_search_bool_shard(self.h, vocab.h, post_off_ptr, docs_ptr, tf_ptr, n_entries, doc_len_ptr,
                                                  n_docs, doc_base, df_ptr, int(coll[0]), int(coll[1]), q_ids_ptr,
                                                  _roles_arg(q_roles, q_off), _u64arr(q_off), n, k1, b, k, top_docs_ptr,
                                                  top_scores_ptr, top))
        return list(top)[:n]

    def search_merge(self, n_shards, n_queries, k_in, in_docs_ptr, in_scores_ptr, in_top_n, k_out, top_docs_ptr,
                     top_scores_ptr):
        """mrg_search_merge: the rows of n_shards searches over the same queries -> the collection's rows.  Row
        (s, q) of the input is in_docs[(s * n_queries + q) * k_in:][:in_top_n[s * n_queries + q]] with in_scores at
        the same positions.  Returns top_n: row q of the output is top_docs[q * k_out:q * k_out + top_n[q]], by
        score descending, then document ascending, then shard ascending; the rest of a row is not written."""
        in_top_n = [int(x) for x in in_top_n]
        if len(in_top_n) != n_shards * n_queries:
            raise ValueError("in_top_n needs n_shards * n_queries entries")
        top = (C.c_uint32 * max(n_queries, 1))()
        _check(load().mrg_search_merge(self.h, n_shards, n_queries, k_in, in_docs_ptr, in_scores_ptr,
                                       (C.c_uint32 * max(len(in_top_n), 1))(*in_top_n), k_out, top_docs_ptr, top_scores_ptr, top))
        return list(top)[:n_queries]

    def postings_merge(self, vocab, shards, post_off_ptr, docs_ptr=None, tf_ptr=None, cap=0):
        """mrg_vocab_postings_merge: the indexes of the shards of one collection -> one index, which search() takes.
        shards is a sequence of (post_off_ptr, docs_ptr, tf_ptr, n_entries), what postings() wrote and returned for
        consecutive document ranges, in order (docs_ptr and tf_ptr may be None where they are not merged, or with 0
        entries).  post_off_ptr (uint64, the vocabulary's words + 1) receives the summed offsets; docs_ptr and tf_ptr
        (cap uint32 each) the postings of every word: shard 0's, then shard 1's, ...  docs_ptr and tf_ptr None:
        offsets only; tf_ptr None: documents only.  Returns the number of entries."""
        shards = list(shards)
        n = len(shards)
        col = lambda j: (_vp * max(n, 1))(*[s[j] for s in shards])
        total = C.c_uint64()
        _check(load().mrg_vocab_postings_merge(self.h, vocab.h, n, col(0), col(1), col(2),
                                               _u64arr([int(s[3]) for s in shards]), post_off_ptr, docs_ptr, tf_ptr, cap,
                                               C.byref(total)))
        return total.value

    def postings_merge_info(self):
        """Diagnostics of the last postings_merge(): entries, words, shards, copy tiles, copy tiles inside one word,
        scratch bytes; HIP-event ms per phase (with set_timing)."""
        return _voc_info("mrg_postings_merge_info", self, ("entries", "words", "shards", "tiles", "single_word_tiles",
                                                           "scratch_bytes"),
                         ("ms_sum", "ms_place", "ms_copy"))

    def search_info(self):
        """Diagnostics of the last search(), search_shard(), search_bool() or search_bool_shard(): queries, query
        positions, postings visited, chunks, accumulate launches, scratch bytes (with the match states of a Boolean
        search); HIP-event ms per phase, summed over the chunks (with set_timing)."""
        return _voc_info("mrg_search_info", self, ("queries", "positions", "postings", "chunks", "acc_launches",
                                                   "scratch_bytes"),
                         ("ms_plan", "ms_accumulate", "ms_select", "ms_order"))

    def encode_info(self):
        """Diagnostics of the last encode(): tokens, UNK and long tokens, non-ASCII 1 KiB chunks, table
        probes, input and scratch bytes; HIP-event ms per pass and of the last vocab() (with set_timing)."""
        return _voc_info("mrg_encode_info", self, ("tokens", "unk", "long_tokens", "nonascii_chunks", "probes",
                                                   "input_bytes", "scratch_bytes"),
                         ("ms_count", "ms_offsets", "ms_emit", "ms_vocab"))

    # ---- plugin surface (host buffers)
    def map_task(self, app, data, doc, doc_id, n_reduce, flags=0):
        h = _vp()
        _check(load().mrg_map(self.h, app, data, len(data), doc.encode(), doc_id, n_reduce, flags, C.byref(h)))
        return Parts(h, n_reduce)

    def reduce_task(self, app, r, parts, n_reduce, flags=0, doc_names=()):
        arr = (_vp * max(len(parts), 1))(*[p.h for p in parts])
        names = (C.c_char_p * max(len(doc_names), 1))(*[n.encode() for n in doc_names])
        out = _vp()
        n = C.c_size_t()
        _check(load().mrg_reduce(self.h, app, r, arr, len(parts), n_reduce, flags, names, len(doc_names),
                                 C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value) if n.value else b""
        load().mrg_free(out)
        return data

    # ---- the reference's text intermediates (wc)
    def map_text(self, data, n_reduce):
        """mr-{m}-{r}.txt contents of one map task (worker.rs:117-140), for r < n_reduce."""
        out = _vp()
        off = (C.c_uint64 * (n_reduce + 1))()
        _check(load().mrg_map_text(self.h, data, len(data), n_reduce, C.byref(out), off))
        blob = C.string_at(out, off[n_reduce]) if off[n_reduce] else b""
        load().mrg_free(out)
        return [blob[off[r]:off[r + 1]] for r in range(n_reduce)]

    def reduce_text(self, files, flags=0):
        """mr-{r}.txt from the contents of the intermediate files mr-{m}-{r}.txt (worker.rs:79-109)."""
        arr = (C.c_char_p * max(len(files), 1))(*files)
        sizes = _u64arr([len(f) for f in files])
        out = _vp()
        n = C.c_size_t()
        _check(load().mrg_reduce_text(self.h, arr, sizes, len(files), flags, C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value) if n.value else b""
        load().mrg_free(out)
        return data

    # ---- synthetic inputs (bench)
    def gen_zipf(self, dev_ptr, n_bytes, seed, file_index, vocab=1 << 20, s=1.1):
        _check(load().mrg_gen_zipf(self.h, dev_ptr, n_bytes, seed, file_index, vocab, s))

    def gen_text(self, dev_ptr, n_bytes, seed, file_index, vocab=1 << 20, s=1.1, style=1):
        """style 0: ASCII (= gen_zipf); 1: Gutenberg-like Unicode (MRG_TEXT_GUTENBERG)."""
        _check(load().mrg_gen_text(self.h, dev_ptr, n_bytes, seed, file_index, vocab, s, style))

    def gen_unique(self, dev_ptr, n_bytes, seed, file_index):
        _check(load().mrg_gen_unique(self.h, dev_ptr, n_bytes, seed, file_index))


def run_job(files, n_reduce, app=APP_WC, out_dir=".", flags=0, n_gpus=1):
    """mrg_run_job: the whole job over files on disk; returns its phase timings (mrg_run_get_stats)."""
    arr = (C.c_char_p * max(len(files), 1))(*[f.encode() for f in files])
    _check(load().mrg_run_job(arr, len(files), n_reduce, app, out_dir.encode(), flags, n_gpus))
    st = RunStats()
    _check(load().mrg_run_get_stats(C.byref(st)))
    return st.as_dict()


def run_stream_stats():
    """mrg_run_get_stream_stats: (batches mapped, peak bytes of device input buffers) of this thread's
    last run_job; 0 batches without FLAG_STREAM (the peak is then the whole input)."""
    b, p = C.c_uint32(), C.c_uint64()
    _check(load().mrg_run_get_stream_stats(C.byref(b), C.byref(p)))
    return b.value, p.value


def stream_plan(sizes, batch_bytes):
    """The batch plan of FLAG_STREAM over one GPU's file sizes (test entry, no GPU needed): the index
    of each batch's first file."""
    L = load()
    f = L.mrg_test_stream_plan
    f.restype = C.c_int
    f.argtypes = [_u64p, C.c_size_t, C.c_uint64, _u32p, C.POINTER(C.c_size_t)]
    first = (C.c_uint32 * max(len(sizes), 1))()
    n = C.c_size_t()
    _check(f(_u64arr(sizes), len(sizes), batch_bytes, first, C.byref(n)))
    return list(first[:n.value])


def merge_sorted_lines(runs):
    """The host k-way merge of per-GPU sorted final.txt runs (test entry, no GPU needed)."""
    L = load()
    f = L.mrg_test_merge_sorted_lines
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_char_p), _u64p, C.c_size_t, C.POINTER(_vp), _u64p]
    arr = (C.c_char_p * max(len(runs), 1))(*runs)
    out, n = _vp(), C.c_uint64()
    _check(f(arr, _u64arr([len(r) for r in runs]), len(runs), C.byref(out), C.byref(n)))
    data = C.string_at(out, n.value) if n.value else b""
    L.mrg_free(out)
    return data


def merge_top_lines(runs, k):
    """The host merge of per-GPU top-k runs (count descending, key ascending), first k lines (test
    entry, no GPU needed)."""
    L = load()
    f = L.mrg_test_merge_top_lines
    f.restype = C.c_int
    f.argtypes = [C.POINTER(C.c_char_p), _u64p, C.c_size_t, C.c_uint64, C.POINTER(_vp), _u64p]
    arr = (C.c_char_p * max(len(runs), 1))(*runs)
    out, n = _vp(), C.c_uint64()
    _check(f(arr, _u64arr([len(r) for r in runs]), len(runs), k, C.byref(out), C.byref(n)))
    data = C.string_at(out, n.value) if n.value else b""
    L.mrg_free(out)
    return data


def comm_id():
    """A fresh RCCL communicator id (bytes) for Comm(); made by one rank, shared out of band."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().mrg_comm_get_id(buf))
    return buf.raw


class Comm:
    """mrg_comm: this rank's membership of an RCCL communicator (one per GPU / context)."""

    def __init__(self, ctx, uid, n_ranks, rank):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("communicator id must be %d bytes" % COMM_ID_BYTES)
        h = _vp()
        _check(load().mrg_comm_init(ctx.h, uid, n_ranks, rank, C.byref(h)))
        self.h = h
        self.n_ranks = n_ranks
        self.rank = rank

    def count(self):
        """mrg_comm_count: ranks of the RCCL communicator (ncclCommCount)."""
        n = C.c_int()
        _check(load().mrg_comm_count(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            _check(load().mrg_comm_destroy(self.h))
            self.h = None
