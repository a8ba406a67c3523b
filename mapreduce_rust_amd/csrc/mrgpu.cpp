// mrgpu.cpp -- the context of libmrgpu.so and its C ABI (include/mrgpu.h): mrg_open .. mrg_get_stats, the error
// text, the version, the pool statistics; job_begin; the mrg_job_* entry points, each a guard around the unit that
// does the work; the test and diagnostics entries that only read the context; the mrg_gen_* generators.
// Owns: g_err, the one DeviceCache, check_sort_n and env_u64 (used by every job unit).
// Calls: mrg_map.cpp (flush_stage, job_map), mrg_agg.cpp (keysbuf_release, acc_release, job_map_add),
// mrg_reduce.cpp (job_reduce, job_final, job_topk), mrg_exchange.cpp (export_sizes, export_pack, job_import),
// mrg_plugin.cpp (check_names).  What the host units share is mrg_host.h.
//
// Pipeline of one job, all on one HIP stream of the context:
//   map     k_map (tokenize + LDS combine)                         wc.rs:6-13, worker.rs:117-131      mrg_map.cpp
//   agg     HBM table insert/compact + long-key fingerprint sort   worker.rs:165-184 (grouping)       mrg_agg.cpp
//           + SipHash-1-3 % R per distinct key                     worker.rs:111-115, 129
//   [shuffle: export by owner = r % G, exchange by the caller (RCCL all-to-all), import]              mrg_exchange.cpp
//   reduce  radix sort by (r, key bytes[, doc]) + format lines     worker.rs:162-184, wc.rs:15-17     mrg_reduce.cpp
// The text intermediates and the plugin surface are mrg_plugin.cpp, mrg_run_job is mrg_run.cpp, the vocabulary
// calls are mrg_vocab.cpp.
// Errors never cross the ABI as exceptions or aborts: every entry point returns a status code.
#include "mrg_host.h"

using namespace mrg_host;

thread_local std::string mrg_host::g_err;

DeviceCache &DeviceCache::get() {
    static DeviceCache *c = new DeviceCache();
    return *c;
}

namespace mrg_host __attribute__((visibility("hidden"))) {

// The radix sorts index records with 32-bit offsets (k_sort.hip): refuse larger inputs loudly.
void check_sort_n(uint64_t n, const char *what) {
    if (n > 0xFFFFFFFFull) raise(MRG_ENOMEM, "%s: %llu records exceed the radix sort's 32-bit index", what,
                                 (unsigned long long)n);
}

// Test knobs (env, read once per map): shrink the map's tail regions and overflow lists on the first
// launch so the spill and grow-and-rerun paths run on small inputs.
uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *v = getenv(name);
    return v && *v ? strtoull(v, nullptr, 10) : dflt;
}

void job_begin(mrg_ctx *c, int app, uint32_t R, uint32_t flags) {
    if (app != MRG_APP_WC && app != MRG_APP_INDEXER) raise(MRG_EINVAL, "unknown app %d", app);
    if (R == 0) raise(MRG_EINVAL, "n_reduce must be > 0");
    sync(c);
    flush_stage(c);     // (nothing is pending between jobs: every map launch flushes first)
    c->stage_used = 0;  // the previous job's staged copies are done
    c->pend_lo = 0;
    keysbuf_release(c->pool, c->keys);
    c->wide.release(c->pool);
    acc_release(c);
    c->keyed = false;
    c->job = true;
    c->app = app;
    c->R = R;
    c->flags = flags;
    c->d_in = nullptr;
    c->doc_off.clear();
    c->doc_ids.clear();
    c->mapped = c->reduced = false;
    c->n_owners = 0;
    c->out_bytes = 0;
    c->extra_first = 0;
    c->part_off.assign(R + 1, 0);
    c->final_bytes = 0;
    c->finalized = false;
    c->topped = false;
    c->st = mrg_stats{};
}

}  // namespace mrg_host

// ===================================================================== C ABI

extern "C" {

const char *mrg_last_error(void) { return g_err.c_str(); }
const char *mrg_version(void) { return "mrgpu 0.6 (gfx950, abi 6)"; }

int mrg_open(int device, mrg_ctx **out) {
    return guard([&] {
        if (!out) raise(MRG_EINVAL, "null out");
        int ndev = 0;
        HIPCHK(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) raise(MRG_EINVAL, "device %d not present (%d devices)", device, ndev);
        HIPCHK(hipSetDevice(device));
        mrg_ctx *c = new mrg_ctx();
        c->device = device;
        c->pool.set_device(device);
        HIPCHK(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
        c->stream = c->own;
        HIPCHK(hipMalloc(&c->d_cnt, sizeof(unsigned long long) * CNT_N));
        // CNT_N counters + pinned scratch (h_cnt[CNT_N]: the key sort's oversized-bucket count)
        // [CNT_N, CNT_N + 8): scratch; [CNT_N + 8, + MRG_NBUCKET / 2): the map's overflow-list fill (u32)
        HIPCHK(hipHostMalloc(&c->h_cnt, sizeof(unsigned long long) * (CNT_N + 8 + MRG_NBUCKET / 2), hipHostMallocDefault));
        HIPCHK(hipHostMalloc(&c->h_stage, MRG_STAGE_BYTES, hipHostMallocDefault));
        HIPCHK(hipMalloc(&c->d_stage, MRG_STAGE_BYTES));
        for (auto &e : c->ev) HIPCHK(hipEventCreate(&e));
        if (const char *v = getenv("MRG_LDS_CAP")) c->lds_cap = atoi(v);
        *out = c;
    });
}

int mrg_close(mrg_ctx *c) {
    return guard([&] {
        if (!c) return;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (auto &e : c->ev) (void)hipEventDestroy(e);
        for (VocDiag *d : {&c->enc, &c->dec, &c->terms, &c->post, &c->srch, &c->pmrg}) d->destroy();
        (void)hipFree(c->d_cnt);
        (void)hipHostFree(c->h_cnt);
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        if (c->d_stage) (void)hipFree(c->d_stage);
        if (c->own) (void)hipStreamDestroy(c->own);
        delete c;
    });
}

int mrg_set_stream(mrg_ctx *c, void *hip_stream) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        sync(c);
        c->stream = hip_stream ? (hipStream_t)hip_stream : c->own;
    });
}

int mrg_set_timing(mrg_ctx *c, int enable) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        c->timing = enable != 0;
    });
}

int mrg_get_stats(mrg_ctx *c, mrg_stats *out) {
    return guard([&] {
        if (!c || !out) raise(MRG_EINVAL, "null argument");
        *out = c->st;
    });
}

int mrg_job_begin(mrg_ctx *c, int app, uint32_t n_reduce, uint32_t flags) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        HIPCHK(hipSetDevice(c->device));
        job_begin(c, app, n_reduce, flags);
    });
}

int mrg_job_set_doc_names(mrg_ctx *c, const char *const *names, uint32_t n_names) {
    return guard([&] {
        need_job(c);
        check_names(names, n_names);
        c->names.assign(names, names + n_names);
    });
}

int mrg_job_set_input(mrg_ctx *c, const uint8_t *d_bytes, const uint64_t *h_doc_off, uint32_t n_docs,
                      const uint32_t *h_doc_ids) {
    return guard([&] {
        need_job(c);
        if (!h_doc_off) raise(MRG_EINVAL, "null document offsets (h_doc_off needs n_docs + 1 entries)");
        if (n_docs && !d_bytes) raise(MRG_EINVAL, "null input");
        if (n_docs == 0xFFFFFFFFu) raise(MRG_EINVAL, "n_docs out of range");
        if ((uintptr_t)d_bytes & 15u) raise(MRG_EINVAL, "input buffer must be 16-byte aligned");
        for (uint32_t i = 0; i < n_docs; ++i)
            if (h_doc_off[i + 1] < h_doc_off[i]) raise(MRG_EINVAL, "document offsets must be non-decreasing");
        c->d_in = d_bytes;
        c->doc_off.assign(h_doc_off, h_doc_off + n_docs + 1);
        if (h_doc_ids) c->doc_ids.assign(h_doc_ids, h_doc_ids + n_docs);
        else c->doc_ids.clear();
        c->mapped = c->reduced = false;
    });
}

int mrg_job_map(mrg_ctx *c) {
    return guard([&] {
        need_job(c);
        acc_release(c);  // replaces the job's keys: what mrg_job_map_add accumulated goes too
        c->st.map_batches = 0;
        job_map(c);
    });
}

int mrg_job_map_add(mrg_ctx *c) {
    return guard([&] { job_map_add(c); });
}

int mrg_job_export_sizes(mrg_ctx *c, uint32_t n_owners, uint64_t *h_rec_counts, uint64_t *h_heap_bytes) {
    return guard([&] { export_sizes(c, n_owners, h_rec_counts, h_heap_bytes); });
}

int mrg_job_export(mrg_ctx *c, void *d_rec, void *d_heap) {
    return guard([&] { export_pack(c, d_rec, d_heap); });
}

int mrg_job_import(mrg_ctx *c, const void *d_rec, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                   const uint64_t *h_seg_recs, const uint64_t *h_seg_heap, uint32_t n_segs) {
    return guard([&] { job_import(c, d_rec, n_rec, d_heap, heap_bytes, h_seg_recs, h_seg_heap, n_segs); });
}

int mrg_job_reduce(mrg_ctx *c, uint64_t *h_out_bytes) {
    return guard([&] {
        job_reduce(c);
        if (h_out_bytes) *h_out_bytes = c->out_bytes;
    });
}

int mrg_job_output(mrg_ctx *c, const uint8_t **d_out, uint64_t *h_part_off) {
    return guard([&] {
        need_job(c);
        if (!c->reduced) raise(MRG_EINVAL, "no output: call mrg_job_reduce first");
        if (d_out) *d_out = c->d_out;
        if (h_part_off) memcpy(h_part_off, c->part_off.data(), 8ull * (c->R + 1));
    });
}

int mrg_job_copy_output(mrg_ctx *c, uint8_t *h_dst, uint64_t cap) {
    return guard([&] {
        need_job(c);
        if (!c->reduced) raise(MRG_EINVAL, "no output: call mrg_job_reduce first");
        if (cap < c->out_bytes) raise(MRG_EINVAL, "destination too small (%llu < %llu)", (unsigned long long)cap,
                                      (unsigned long long)c->out_bytes);
        if (c->out_bytes)
            HIPCHK(hipMemcpyAsync(h_dst, c->d_out, c->out_bytes, hipMemcpyDeviceToHost, c->stream));
        sync(c);
    });
}

int mrg_job_final(mrg_ctx *c, const uint8_t **d_out, uint64_t *h_bytes) {
    return guard([&] {
        job_final(c);
        if (d_out) *d_out = c->d_final;
        if (h_bytes) *h_bytes = c->final_bytes;
    });
}

int mrg_job_copy_final(mrg_ctx *c, uint8_t *h_dst, uint64_t cap) {
    return guard([&] {
        need_job(c);
        if (!c->finalized) raise(MRG_EINVAL, "no final.txt: call mrg_job_final first");
        if (cap < c->final_bytes) raise(MRG_EINVAL, "destination too small (%llu < %llu)", (unsigned long long)cap,
                                        (unsigned long long)c->final_bytes);
        if (c->final_bytes)
            HIPCHK(hipMemcpyAsync(h_dst, c->d_final, c->final_bytes, hipMemcpyDeviceToHost, c->stream));
        sync(c);
    });
}

int mrg_job_topk(mrg_ctx *c, uint64_t k, const uint8_t **d_out, uint64_t *h_bytes, uint64_t *h_lines) {
    return guard([&] {
        job_topk(c, k);
        if (d_out) *d_out = c->d_top;
        if (h_bytes) *h_bytes = c->top_bytes;
        if (h_lines) *h_lines = c->top_lines;
    });
}

int mrg_job_copy_topk(mrg_ctx *c, uint8_t *h_dst, uint64_t cap) {
    return guard([&] {
        need_job(c);
        if (!c->topped) raise(MRG_EINVAL, "no top-k lines: call mrg_job_topk first");
        if (cap < c->top_bytes) raise(MRG_EINVAL, "destination too small (%llu < %llu)", (unsigned long long)cap,
                                      (unsigned long long)c->top_bytes);
        if (c->top_bytes) {
            if (!h_dst) raise(MRG_EINVAL, "null argument");
            HIPCHK(hipMemcpyAsync(h_dst, c->d_top, c->top_bytes, hipMemcpyDeviceToHost, c->stream));
        }
        sync(c);
    });
}

int mrg_pool_stats(mrg_ctx *c, uint64_t *outstanding, uint64_t *held_bytes) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        if (outstanding) *outstanding = c->pool.outstanding();
        if (held_bytes) *held_bytes = c->pool.held_bytes();
    });
}

int mrg_pool_alloc_stats(mrg_ctx *c, uint64_t *n_allocs, uint64_t *alloc_bytes, double *alloc_ms) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        c->pool.alloc_stats(n_allocs, alloc_bytes, alloc_ms);
    });
}

// Fault injection for the tests of the error exits (not in include/mrgpu.h; tests/test_gpu_pool_errors.py):
// the k-th block this context's pool is asked for from now on fails with MRG_ENOMEM ("injected allocation
// failure") before anything is taken, once; k = 0 disarms.
int mrg_test_pool_fail(mrg_ctx *c, uint64_t k) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        c->pool.fail_in(k);
    });
}

// Diagnostics of the accumulator (not in include/mrgpu.h; tools/time_stream.py): h_info[0..6) = table
// slots, short keys, long keys, long-key heap bytes, rehashes so far, batches; *ms_fold = the last
// batch's fold (HIP events, with mrg_set_timing: aggregation end .. fold end).  Either may be NULL.
int mrg_test_acc_info(mrg_ctx *c, uint64_t *h_info, double *ms_fold) {
    return guard([&] {
        need_job(c);
        const Acc &A = c->acc;
        if (h_info) {
            const uint64_t v[6] = {A.T.cap, A.n, A.lng.n, A.lng.heap_bytes, A.rehashes, A.batches};
            memcpy(h_info, v, sizeof v);
        }
        if (ms_fold) *ms_fold = A.ms_fold;
    });
}

// Diagnostics of the last mrg_job_topk (not in include/mrgpu.h; tools/time_topk.py): h_info[0..4) =
// distinct keys, candidates, select passes run, candidates dropped as their partition's last key;
// h_pass_bytes[24] = bytes each select pass read (0: pass not run).  Either may be NULL.
int mrg_test_topk_info(mrg_ctx *c, uint64_t *h_info, uint64_t *h_pass_bytes) {
    return guard([&] {
        need_job(c);
        if (!c->topped) raise(MRG_EINVAL, "no top-k lines: call mrg_job_topk first");
        if (h_info) memcpy(h_info, c->top_info, 4 * sizeof(uint64_t));
        if (h_pass_bytes) memcpy(h_pass_bytes, c->top_pass_bytes, sizeof c->top_pass_bytes);
    });
}

void mrg_free(void *p) { free(p); }

int mrg_gen_zipf(mrg_ctx *c, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index, uint32_t vocab,
                 double s) {
    return guard([&] {
        if (!c || (n_bytes && !d_dst)) raise(MRG_EINVAL, "null argument");
        HIPCHK(hipSetDevice(c->device));
        if (mrg_gen_zipf_impl(d_dst, n_bytes, seed, file_index, vocab, s, 0, c->stream))
            raise(MRG_EHIP, "zipf generator failed: %s", hipGetErrorString(hipGetLastError()));
    });
}

int mrg_gen_text(mrg_ctx *c, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index, uint32_t vocab,
                 double s, uint32_t style) {
    return guard([&] {
        if (!c || (n_bytes && !d_dst)) raise(MRG_EINVAL, "null argument");
        if (style > MRG_TEXT_GUTENBERG) raise(MRG_EINVAL, "unknown text style %u", style);
        HIPCHK(hipSetDevice(c->device));
        if (mrg_gen_zipf_impl(d_dst, n_bytes, seed, file_index, vocab, s, style, c->stream))
            raise(MRG_EHIP, "text generator failed: %s", hipGetErrorString(hipGetLastError()));
    });
}

int mrg_gen_unique(mrg_ctx *c, uint8_t *d_dst, uint64_t n_bytes, uint64_t seed, uint64_t file_index) {
    return guard([&] {
        if (!c || (n_bytes && !d_dst)) raise(MRG_EINVAL, "null argument");
        HIPCHK(hipSetDevice(c->device));
        if (mrg_gen_unique_impl(d_dst, n_bytes, seed, file_index, c->stream))
            raise(MRG_EHIP, "unique generator failed: %s", hipGetErrorString(hipGetLastError()));
    });
}

}  // extern "C"
