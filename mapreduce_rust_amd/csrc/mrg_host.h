// mrg_host.h -- what the host units of libmrgpu.so share (mrgpu.cpp, mrg_map.cpp, mrg_agg.cpp, mrg_reduce.cpp,
// mrg_exchange.cpp, mrg_plugin.cpp, mrg_run.cpp, mrg_vocab.cpp): the guard that ends the error path at the C ABI,
// the device-block pool, the context and the vocabulary, a few helpers, and -- at the end, one block per defining
// unit -- the functions of the job side that another unit calls, with the structs their signatures need.  A unit's
// other helpers stay in its own anonymous namespace.  The error path itself (MrgError, raise, HIPCHK) and the
// pool's scope guard (Scratch) live in mrg_internal.h, because the .hip files' host functions use them too; the
// RCCL communicator is mrg_comm.h, for the two units that need it.
// Host only: no .hip file includes it.  Nothing here joins the library's exported symbols.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "mrg_device.h"
#include "mrg_internal.h"
#include "mrgpu.h"

namespace mrg_host __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;  // mrg_last_error() of this thread (defined in mrgpu.cpp)

template <class F>
int guard(F &&f) {
    try {
        f();
        return MRG_OK;
    } catch (const MrgError &e) {
        g_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        g_err = "host out of memory";
        return MRG_ENOMEM;
    } catch (...) {
        g_err = "unexpected internal error";
        return MRG_EINVAL;
    }
}

// ---------------------------------------------------------------- caching device allocator
// Process-wide cache of the device blocks of closed contexts, per device (r06).  A worker process runs
// one task after another (src/bin/mrworker.rs:43-149); every mrg_run_job opens fresh contexts, and
// without this each call re-allocated -- and the GPU re-touched -- its multi-GiB workspaces (the first
// job's map ran 1.2x its steady time).  Capped at MRG_POOL_KEEP_GIB per device (default: half the
// device's memory; 0 = off); blocks beyond the cap are freed.  Never destroyed: no hipFree may run
// after the HIP runtime's own teardown at process exit.
class DeviceCache {
   public:
    static DeviceCache &get();  // the one instance (defined in mrgpu.cpp)
    // a cached block of `dev` of at least c bytes and at most c + c / 4 (any size >= c when `any`: the
    // device is full) -- its size in *got -- else null
    void *take(int dev, size_t c, size_t *got, bool any = false) {
        std::lock_guard<std::mutex> lk(mu_);
        auto &f = free_[dev];
        auto it = f.lower_bound(c);
        if (it == f.end() || (!any && it->first > c + (c >> 2))) return nullptr;
        void *p = it->second;
        *got = it->first;
        bytes_[dev] -= it->first;
        f.erase(it);
        return p;
    }
    // a block of a closing context (its work on the device finished); the current device is `dev`
    void give(int dev, void *p, size_t c) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (bytes_[dev] + c <= keep(dev)) {
                free_[dev].insert({c, p});
                bytes_[dev] += c;
                return;
            }
        }
        (void)hipFree(p);
    }
    void trim(int dev) {  // the device is full: give the cached blocks back to the driver
        std::multimap<size_t, void *> f;
        {
            std::lock_guard<std::mutex> lk(mu_);
            f.swap(free_[dev]);
            bytes_[dev] = 0;
        }
        for (auto &kv : f) (void)hipFree(kv.second);
    }

   private:
    DeviceCache() {
        if (const char *v = getenv("MRG_POOL_KEEP_GIB")) keep_env_ = (long long)(atof(v) * (double)((size_t)1 << 30));
    }
    // bytes of `dev` (the current device) kept: MRG_POOL_KEEP_GIB, else half the device's memory.  A
    // block handed back to the driver is wiped before any allocation can reuse it (a fresh context
    // after one that freed ~100 GiB waited 4.6 s in hipMalloc: profiles/r06/v13), so one C5-sized
    // job's blocks (67-83 GiB at 13.4 GB of input) are worth keeping
    size_t keep(int dev) {
        if (keep_env_ >= 0) return (size_t)keep_env_;
        auto it = keep_dev_.find(dev);
        if (it != keep_dev_.end()) return it->second;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
            (void)hipGetLastError();
            tot = (size_t)128 << 30;
        }
        return keep_dev_[dev] = tot / 2;
    }
    std::mutex mu_;
    std::map<int, std::multimap<size_t, void *>> free_;
    std::map<int, size_t> bytes_;
    std::map<int, size_t> keep_dev_;
    long long keep_env_ = -1;
};

class Pool : public DevPool {
   public:
    void set_device(int dev) { dev_ = dev; }
    void *get(size_t bytes) override {
        if (fail_in_ && --fail_in_ == 0) raise(MRG_ENOMEM, "injected allocation failure");
        const size_t c = cls(bytes ? bytes : 1);
        // smallest free block of this class or up to two classes above (record counts drift by a few
        // between jobs over the same input: an exact-class pool would then miss, run out of device
        // memory and trim everything)
        auto it = free_.lower_bound(c);
        if (it != free_.end() && it->first <= c + (c >> 2)) {
            void *p = it->second;
            free_.erase(it);
            return p;
        }
        if (dev_ >= 0) {  // a block a closed context of this device left behind
            size_t got = 0;
            if (void *q = DeviceCache::get().take(dev_, c, &got)) {
                size_[q] = got;
                ++reused_;
                return q;
            }
        }
        void *p = nullptr;
        if (debug_) fprintf(stderr, "[mrgpu] pool: allocating %zu bytes\n", c);
        const auto t0 = std::chrono::steady_clock::now();
        if (hipMalloc(&p, c) != hipSuccess) {
            (void)hipGetLastError();
            // the device is full: a larger cached block first (memory handed back to the driver is
            // wiped before it can be allocated again: a trim costs seconds)
            if (dev_ >= 0) {
                size_t got = 0;
                if (void *q = DeviceCache::get().take(dev_, c, &got, true)) {
                    alloc_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                    size_[q] = got;
                    ++reused_;
                    return q;
                }
            }
            if (debug_) fprintf(stderr, "[mrgpu] pool: device full, trimming %zu free blocks\n", free_.size());
            trim();
            if (hipMalloc(&p, c) != hipSuccess) {
                (void)hipGetLastError();
                raise(MRG_ENOMEM, "device allocation of %zu bytes failed", c);
            }
        }
        alloc_ms_ += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ++allocs_;
        alloc_bytes_ += c;
        size_[p] = c;
        return p;
    }
    void put(void *p) override {
        if (!p) return;
        auto it = size_.find(p);
        if (it != size_.end()) free_.insert({it->second, p});
    }
    void trim() {
        (void)hipDeviceSynchronize();
        for (auto &kv : free_) {
            (void)hipFree(kv.second);
            size_.erase(kv.second);
        }
        free_.clear();
        if (dev_ >= 0) DeviceCache::get().trim(dev_);
    }
    // blocks handed out and not returned; bytes held by the pool (handed out or cached)
    uint64_t outstanding() const { return size_.size() - free_.size(); }
    uint64_t held_bytes() const {
        uint64_t b = 0;
        for (auto &kv : size_) b += kv.second;
        return b;
    }
    // device allocations made so far (hipMalloc calls, bytes, host milliseconds inside them): a fresh
    // context's first job pays them, later jobs reuse the cached blocks
    void alloc_stats(uint64_t *n, uint64_t *bytes, double *ms) const {
        if (n) *n = allocs_;
        if (bytes) *bytes = alloc_bytes_;
        if (ms) *ms = alloc_ms_;
    }
    uint64_t reused() const { return reused_; }  // blocks taken from the process-wide device cache
    void fail_in(uint64_t k) { fail_in_ = k; }   // mrg_test_pool_fail: the k-th get from now throws, once (0: none)
    ~Pool() override {  // (the caller has made dev_ current)
        (void)hipDeviceSynchronize();
        for (auto &kv : size_) {
            if (dev_ >= 0) DeviceCache::get().give(dev_, kv.first, kv.second);
            else (void)hipFree(kv.first);
        }
    }

   private:
    static size_t cls(size_t b) {
        if (b <= 4096) return (b + 255) & ~(size_t)255;
        size_t p = 4096;
        while (p < b) p <<= 1;
        const size_t step = p >> 3;  // 8 classes per octave: <= 12.5% slack
        return ((b + step - 1) / step) * step;
    }
    std::multimap<size_t, void *> free_;
    std::unordered_map<void *, size_t> size_;
    bool debug_ = getenv("MRG_DEBUG") != nullptr;
    uint64_t allocs_ = 0, alloc_bytes_ = 0, reused_ = 0, fail_in_ = 0;
    int dev_ = -1;
    double alloc_ms_ = 0.0;
};

struct KeysBuf {
    KeySet ks{};
    uint64_t n = 0, cap = 0;
    uint8_t *heap = nullptr;
    uint64_t heap_bytes = 0;
    bool any_long = false;
    bool sorted = false;  // keys already in (partition, key) order (wide aggregation, no long keys)
};

// Result of the wide (sample-sort) aggregation, k_wide.hip: distinct keys in output order, per leaf,
// with gaps between leaves; formatted directly, or made a dense KeySet for the other consumers.
struct WideRes {
    bool ready = false;
    uint32_t B1 = 0, B1r = 0;
    uint64_t *kout = nullptr, *ocnt = nullptr;
    uint32_t *nleaf = nullptr, *leaf_nd = nullptr, *leaf_last = nullptr, *leaf_pk = nullptr;
    uint64_t *leaf_out = nullptr, *leaf_bytes = nullptr;
    uint64_t distinct = 0;
    void release(Pool &p) {
        p.put(kout); p.put(ocnt); p.put(nleaf); p.put(leaf_nd); p.put(leaf_last); p.put(leaf_out); p.put(leaf_bytes);
        p.put(leaf_pk);
        *this = WideRes{};
    }
};

// The accumulator of mrg_job_map_add (k_acc.hip): the job's keys over all its
// batches.  Short keys live in a persistent open-addressing table, long keys (rare) beside it as rows
// of a KeysBuf with their heap; c->keys is then only a view, emitted on demand for the consumers.
struct Acc {
    bool on = false;      // the job's keys live here
    bool dirty = false;   // c->keys does not show them (a fold, or a failed batch, since the last emit)
    bool seeded = false;  // started from keys the job already held (mrg_job_map / mrg_job_import)
    AccTable T{};
    uint64_t n = 0;       // short keys in the table (exact: the fold counts the slots it claims)
    KeysBuf lng;          // long keys: dense rows (k0, k1 = prefix, cnt, hoff, doc, len, part) + heap
    uint64_t in_bytes = 0, tokens = 0, long_tokens = 0;  // totals over the batches (mrg_stats)
    uint32_t batches = 0, rehashes = 0;
    double ms_fold = 0.0;  // last batch, HIP events (mrg_set_timing): end of the aggregation .. end of the fold
};

// The diagnostics of one kind of vocabulary call, read by its mrg_*_info entry point: counters, the HIP-event
// milliseconds of its passes (mrg_set_timing), and the events, which make() creates on first use and only when
// timing is on.  What a call clears before it works (clear(n_ms): info and ms[0, n_ms)):
//   mrg_vocab_encode        info and ms[0..2]; ms[3], the time of the last mrg_job_vocab, stays
//   mrg_vocab_decode        info and ms[0..2]; ms[3], the time of the last mrg_vocab_from_text, stays
//   mrg_vocab_term_counts, mrg_vocab_postings, mrg_vocab_search   everything (they write ms[0..3], ms[0..4], ms[0..3])
//   mrg_vocab_search_shard, mrg_vocab_search_bool, mrg_vocab_search_bool_shard  as mrg_vocab_search, in the same
//   record; mrg_vocab_stats_add and mrg_search_merge keep none
//   mrg_vocab_postings_merge  everything (it writes ms[0..2])
struct VocDiag {
    uint64_t info[8] = {};
    double ms[5] = {};
    hipEvent_t ev[6] = {};
    void clear(int n_ms) { memset(info, 0, sizeof info); std::fill(ms, ms + n_ms, 0.0); }
    void make(mrg_ctx *c);
    void rec(mrg_ctx *c, int i);               // record ev[i] on the context's stream
    double elapsed(mrg_ctx *c, int a, int b);  // ms from ev[a] to ev[b] (waits for ev[b]); 0 without timing
    void destroy() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }  // mrg_close
};

}  // namespace mrg_host

struct mrg_ctx {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    mrg_host::Pool pool;
    unsigned long long *d_cnt = nullptr;  // CNT_N counters
    unsigned long long *h_cnt = nullptr;  // pinned mirror
    // pinned staging of the small per-job host tables (document offsets, region bases, map args): one
    // bump region, reset by job_begin (after its sync), so their copies are plain async DMA
    uint8_t *h_stage = nullptr;
    size_t stage_used = 0;
    // batched small writes (stage_h2d / stage_fill): their device copy of the staging buffer, the ops
    // not yet issued, and the first staging byte they use
    uint8_t *d_stage = nullptr;
    std::vector<StageOp> pend;
    size_t pend_lo = 0;
    bool timing = false;
    hipEvent_t ev[8] = {};
    int lds_cap = 4096;
    int map_grid = 0;
    uint64_t long_hint = 0, ovf_hint = 0;
    uint64_t lper_hint = 0;  // long-token records per map workgroup region (grown on a rerun)
    uint32_t agg_nsub = 1;  // bucket-aggregation workgroups per bucket (grown when the tables overflow)
    std::vector<double> bcap_rate;  // tail records per (bucket, map workgroup) per input byte of the workgroup
    std::vector<double> bcap16_rate;  // the same for the 16-byte regions (wc keys of 13..16 bytes)
    uint64_t ocap_hint = 0;         // records per bucket overflow list
    bool spec_agg = false, spec_c32 = false;  // last wc job took the bucket path (with 32-bit counts)
    bool wide_hint = false;   // last wc job took the wide aggregation (the next one may take the wide map)
    bool wc_sized = false;    // a wc job of >= 64 MiB has run on this context (its path is a measured hint)
    uint64_t wcap_hint = 0;   // wide map: records per (L1 bucket, workgroup) region the last run needed
    bool w12_off = false;     // wide map: a job overflowed the 16-byte lists of the 12-byte regions
    // job
    bool job = false;
    int app = 0;
    uint32_t R = 0, flags = 0;
    const uint8_t *d_in = nullptr;
    std::vector<uint64_t> doc_off;
    std::vector<uint32_t> doc_ids;
    std::vector<std::string> names;
    mrg_host::KeysBuf keys;
    mrg_host::WideRes wide;
    mrg_host::Acc acc;
    bool keyed = false;   // keys / wide hold the complete result of a map or an import
    bool mapped = false;
    uint32_t n_owners = 0;
    std::vector<uint64_t> exp_rec, exp_heap;
    uint64_t xrec_vmax = MRG_XREC_VMAX;  // count per short export record (test knob MRG_TEST_XREC_VMAX)
    uint8_t *d_out = nullptr;
    uint64_t out_cap = 0, out_bytes = 0;
    std::vector<uint64_t> part_off;
    bool reduced = false;
    uint8_t *d_final = nullptr;     // final.txt (mrg_job_final)
    uint64_t final_cap = 0, final_bytes = 0;
    bool finalized = false;
    uint8_t *d_top = nullptr;       // the K most frequent lines (mrg_job_topk)
    uint64_t top_cap = 0, top_bytes = 0, top_lines = 0;
    bool topped = false;
    uint64_t top_info[8] = {};      // last mrg_job_topk: keys, candidates, select passes, dropped candidates
    uint64_t top_pass_bytes[MRG_TOPK_DIGITS] = {};  // bytes each of its select passes read (0: pass not run)
    uint64_t extra_first = 0;       // text reduce: values of empty-key lines, folded into the first group
    mrg_stats st{};
    // last mrg_vocab_encode, _decode, _term_counts, _postings, _search, _postings_merge (the slots: mrg_*_info in
    // mrg_vocab.cpp)
    mrg_host::VocDiag enc, dec, terms, post, srch, pmrg;
};

// A vocabulary (mrg_job_vocab, mrg_vocab_from_text): one device allocation of its own -- the "word count\n"
// lines in id order, the byte offset of every line, the word -> id table over them (k_encode.hip), and
// the id-indexed word lengths and packed words of the decoder (k_decode.hip).  Read-only once built.
struct mrg_vocab {
    int device = 0;
    uint64_t n = 0, text_bytes = 0;
    void *block = nullptr;
    VocTable T{};
    VocWords W{};
};

namespace mrg_host __attribute__((visibility("hidden"))) {

inline uint32_t hash_bits(const mrg_ctx *c) { return (c->flags >> 8) & 0xFFu; }
inline bool is_idx(const mrg_ctx *c) { return c->app == MRG_APP_INDEXER; }
inline void sync(mrg_ctx *c) { HIPCHK(hipStreamSynchronize(c->stream)); }

// Timing events (mrg_set_timing) of one of the context's event arrays: c->ev (made by mrg_open), or a VocDiag's
inline void ev_rec(mrg_ctx *c, hipEvent_t *ev, int i) {
    if (c->timing) HIPCHK(hipEventRecord(ev[i], c->stream));
}
inline double ev_ms(mrg_ctx *c, hipEvent_t *ev, int a, int b) {
    if (!c->timing) return 0.0;
    float ms = 0;
    HIPCHK(hipEventSynchronize(ev[b]));
    HIPCHK(hipEventElapsedTime(&ms, ev[a], ev[b]));
    return ms;
}
inline void VocDiag::make(mrg_ctx *c) {
    if (!c->timing) return;
    for (auto &e : ev)
        if (!e) HIPCHK(hipEventCreate(&e));
}
inline void VocDiag::rec(mrg_ctx *c, int i) { ev_rec(c, ev, i); }
inline double VocDiag::elapsed(mrg_ctx *c, int a, int b) { return ev_ms(c, ev, a, b); }

inline uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 1024;
    while (p < x) p <<= 1;
    return p;
}

// the number of bytes a value up to maxval can set
inline uint32_t bytes_for(uint64_t maxval) {
    uint32_t b = 0;
    while (maxval) { ++b; maxval >>= 8; }
    return b;
}

inline void need_job(mrg_ctx *c) {
    if (!c) raise(MRG_EINVAL, "null context");
    if (!c->job) raise(MRG_EINVAL, "no job: call mrg_job_begin first");
}

// ---------------------------------------------------------------- the job side: what one unit calls of another

// the context's pinned staging region and its device copy (made by mrg_open, filled by mrg_map.cpp)
constexpr size_t MRG_STAGE_BYTES = 256u << 10;

// ---- mrgpu.cpp
void check_sort_n(uint64_t n, const char *what);
uint64_t env_u64(const char *name, uint64_t dflt);
void job_begin(mrg_ctx *c, int app, uint32_t R, uint32_t flags);

// ---- mrg_map.cpp
void flush_stage(mrg_ctx *c);
void read_counters(mrg_ctx *c);
void job_map(mrg_ctx *c);

// ---- mrg_agg.cpp
void keysbuf_release(Pool &p, KeysBuf &k);
void acc_release(mrg_ctx *c);

struct ShortSrc {
    const uint64_t *k0 = nullptr, *k1 = nullptr;
    const uint32_t *cnt = nullptr, *doc = nullptr;
    const XRec *x = nullptr;   // exchange records (short form only; long ones take the long path)
    const LRec *lx = nullptr;  // text-reduce line records
    uint64_t n = 0;
};
void aggregate(mrg_ctx *c, const ShortSrc &src, LongItems li);

// One launch of the per-bucket aggregation; owns its overflow list (B.ok0, ok1, ocnt, odoc).
struct AggLaunch {
    BucketArgs B{};
    uint64_t nlong = 0;  // long keys the launch reserved key slots for
    bool c32 = false;
    Scratch own;
    explicit AggLaunch(Pool &p) : own(p) {}
    AggLaunch(AggLaunch &&) = default;
    AggLaunch &operator=(AggLaunch &&) = default;
    bool live() const { return !own.b.empty(); }
    void drop() { own.put_all(); }  // the overflow list back to the pool
};
uint64_t agg_ocap(mrg_ctx *c);
AggLaunch agg_launch(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, uint64_t ocap, uint32_t nsub,
                     uint64_t nlong, bool c32, bool zero);
bool bucket_aggregate(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, LongItems li,
                      AggLaunch *pre = nullptr);

SortPlan part_key_plan(uint32_t R);
void wide_aggregate(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, LongItems li);
void wide_densify(mrg_ctx *c, uint64_t extra);

// MRG_DEBUG: the HIP-event time of the phases of one wide aggregation.  The first mark starts the clock; every
// later one ends a phase and names it.  The events are the clock's own and go with it on every exit.
struct PhaseClock {
    const bool on = getenv("MRG_DEBUG") != nullptr;
    hipStream_t s;
    std::vector<std::pair<hipEvent_t, const char *>> ev;
    explicit PhaseClock(hipStream_t st) : s(st) {}
    PhaseClock(const PhaseClock &) = delete;
    PhaseClock &operator=(const PhaseClock &) = delete;
    ~PhaseClock() {
        for (auto &m : ev) (void)hipEventDestroy(m.first);
    }
    void mark(const char *name) {
        if (!on) return;
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        ev.push_back({e, name});
        HIPCHK(hipEventRecord(e, s));
    }
    void report() {  // (the stream has reached the last mark)
        fprintf(stderr, "[mrgpu] wide phases (ms):");
        for (size_t i = 1; i < ev.size(); ++i) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, ev[i - 1].first, ev[i].first));
            fprintf(stderr, " %s %.2f", ev[i].second, ms);
        }
        fprintf(stderr, "\n");
    }
};

// What the first level hands to wide_finish: n records in L1 buckets, bucket b = partition * B1r + key
// range (bstart[b] .. bstart[b + 1]) -- L1's output K1, or (wm.rin) the wide map's regions -- the
// splitters that cut them, and the nw weighted keys (the flushed map tables, aggregated and sorted).
struct WideL1 {
    uint64_t n = 0, nw = 0;
    uint32_t B1 = 0, B1r = 0;
    uint64_t *K1 = nullptr;      // [2 (n + nw) + 2] L1's output, then the leaves' output keys
    uint64_t *bstart = nullptr;  // [B1 + 1]
    uint64_t *spl1 = nullptr;
    uint16_t *bid = nullptr;     // [n] L1 bucket, then L2 leaf, of each record
    uint64_t *wk0 = nullptr, *wk1 = nullptr, *wcnt = nullptr;
    uint32_t *wpart = nullptr;
    WmapIn wm;
};
void wide_finish(mrg_ctx *c, Scratch &own, const WideL1 &l1, LongItems li, PhaseClock &clock);

void acc_emit(mrg_ctx *c);
void job_map_add(mrg_ctx *c);

// ---- mrg_reduce.cpp
void job_reduce(mrg_ctx *c);
void job_final(mrg_ctx *c);
SortRec *job_topk(mrg_ctx *c, uint64_t k, Scratch *keep = nullptr);

// ---- mrg_exchange.cpp (its communicator side: mrg_comm.h)
void export_sizes(mrg_ctx *c, uint32_t n_owners, uint64_t *h_rec, uint64_t *h_heap);
void export_pack(mrg_ctx *c, void *d_rec, void *d_heap, bool wait = true);
void import_recs(mrg_ctx *c, const XRec *xr, const LRec *lr, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                 const uint64_t *seg_recs, const uint64_t *seg_heap, uint32_t n_segs);
void job_import(mrg_ctx *c, const void *d_rec, uint64_t n_rec, const void *d_heap, uint64_t heap_bytes,
                const uint64_t *seg_recs, const uint64_t *seg_heap, uint32_t n_segs);
void job_shuffle(mrg_ctx *c, mrg_comm *m);
void test_fail(const char *stage, int rank);

// ---- mrg_plugin.cpp
void check_names(const char *const *names, uint32_t n);

}  // namespace mrg_host
