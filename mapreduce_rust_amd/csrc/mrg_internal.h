// mrg_internal.h -- host-side declarations shared by the kernel files and the C-ABI layer: the kernels'
// argument records and launchers, and what every host function that takes pool blocks or waits for the
// device needs -- the error path (MrgError, raise, HIPCHK), the pool interface and its scope guard (Scratch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mrgpu.h"

#ifndef MRG_MAP_WAVES  // (timing variants override it: the r06 occupancy sweep)
#define MRG_MAP_WAVES 16        // waves per map workgroup (one workgroup per CU, one shared LDS table)
#endif
#define MRG_MAP_WG (64 * MRG_MAP_WAVES)
#define MRG_MAP_SEG 16          // input bytes per lane per tile
#define MRG_MAP_TILE (64 * MRG_MAP_SEG)  // 1 KiB tile per WAVE iteration (waves never synchronise)
#define MRG_MAP_HALO 64         // bytes after the tile staged in LDS (tokens crossing the tile end)
#define MRG_MAP_BEHIND 16       // bytes before the tile staged in LDS (previous codepoint)
#define MRG_MAP_NSUB 2          // 1 KiB tiles per wave iteration (one block, prefetched one block ahead)

// Tail records (LDS-table misses) are bucketed by key hash into MRG_NBUCKET buckets; every
// (bucket, map workgroup) pair owns a private region of the pool, so appending is an LDS atomic.
// One workgroup per bucket later sums them in LDS (k_keys.hip).
#ifndef MRG_NBUCKET_LOG2
#define MRG_NBUCKET_LOG2 8  // 256: half the open tail lines of 512 (map 8.1 -> 7.5 ms at C3)
#endif
#define MRG_NBUCKET (1 << MRG_NBUCKET_LOG2)
#define MRG_BA_CAP 7680          // max LDS table slots of the per-bucket aggregation kernel (k_keys.hip ba_cap)
// bytes of one tail record in MapArgs::pool: wc 12 ({k0, high word of k1}: keys of <= 12 bytes, whose
// k1 low word is 0 -- keys never contain NUL), the indexer 24 ({k0, k1, doc}); wc keys of 13..16
// bytes go to the 16-byte pool (MapArgs::pool16)
#define MRG_TAIL_BYTES(idx) ((idx) ? 24u : 12u)

// counters[] slots written by the kernels
enum {
    CNT_REC = 0,      // tail records written by the map kernel
    CNT_LONG = 1,     // long-token records
    CNT_TOKENS = 2,   // tokens
    CNT_ERRPOS = 3,   // first invalid UTF-8 byte (atomicMin), ~0 if none
    CNT_KEYS = 4,     // distinct keys appended to the KeySet
    CNT_OVF = 5,      // tail records that found neither region nor overflow-list room (rerun)
    CNT_OVF2 = 6,     // keys that did not fit their bucket's LDS table (exact overflow path)
    CNT_NONASCII = 7, // 1 KiB tiles that took the non-ASCII tokenizer
    CNT_REC16 = 8,    // of CNT_REC: 16-byte tail records (wc keys of 13..16 bytes)
    CNT_LONGX = 9,    // long-token records beyond their workgroup's region (the shared list)
    CNT_W16 = 10,     // wide map, 12-byte regions: keys of 13..16 bytes that found their bucket's list full
    CNT_N = 11
};

// Stream-ordered caching allocator interface (all work of a context runs on one stream, so a
// buffer released after its last enqueued use can be handed out again immediately).
struct DevPool {
    virtual void *get(size_t bytes) = 0;
    virtual void put(void *p) = 0;
    virtual ~DevPool() {}
};

namespace mrg_host __attribute__((visibility("hidden"))) {

// The error path of the C ABI: host code throws, the entry points turn it into a code (guard, mrg_host.h).
struct MrgError {
    int code;
    std::string msg;
};

[[noreturn]] inline void raise(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw MrgError{code, buf};
}

#define HIPCHK(x)                                                                                \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) ::mrg_host::raise(MRG_EHIP, "%s: %s", #x, hipGetErrorString(e_));  \
    } while (0)

// a block the caller owns from here on: only the context's long-lived members take blocks this way
template <class T>
T *pget(DevPool &p, uint64_t n) {
    return (T *)p.get(sizeof(T) * (n ? n : 1));
}

// The pool blocks of one scope, returned on every exit from it, an exception included.  A block goes
// back at the point the host reaches, while kernels that use it may still be queued on the context's
// stream: every later user of the block runs on that same stream, behind them.  put() returns one block
// early, so the allocations that follow can reuse it; release() hands one to an owner that outlives
// the scope (c->keys, c->wide, c->d_out, another Scratch).
struct Scratch {
    DevPool &p;
    std::vector<void *> b;
    explicit Scratch(DevPool &pool) : p(pool) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    Scratch(Scratch &&o) : p(o.p), b(std::move(o.b)) { o.b.clear(); }
    Scratch &operator=(Scratch &&o) {  // (of the same pool)
        put_all();
        b = std::move(o.b);
        o.b.clear();
        return *this;
    }
    template <class T>
    T *get(uint64_t n) {
        b.push_back(nullptr);
        return (T *)(b.back() = pget<T>(p, n));
    }
    template <class T>
    T *adopt(T *q) {
        if (q) b.push_back((void *)q);
        return q;
    }
    template <class T>
    T *release(T *q) {
        auto it = std::find(b.begin(), b.end(), (void *)q);
        if (it != b.end()) b.erase(it);
        return q;
    }
    template <class T>
    void put(T *q) {
        if (q) p.put((void *)release(q));
    }
    void put_all() {
        for (void *q : b) p.put(q);
        b.clear();
    }
    void keep() { b.clear(); }  // every block has found its longer-lived owner
    ~Scratch() { put_all(); }
};

}  // namespace mrg_host

// Workgroups of `block` threads that give each of n items a thread; at least one.
inline unsigned grid_for(uint64_t n, uint64_t block) { return (unsigned)std::max<uint64_t>(1, (n + block - 1) / block); }

struct MapArgs {
    const uint8_t *in;
    const uint64_t *doc_off;     // [n_docs + 1] byte offsets into `in`
    const uint64_t *chunk_base;  // [n_docs + 1] first tile index of each document
    const uint32_t *doc_id;      // [n_docs] global document id
    uint32_t n_docs;
    uint64_t n_chunks;
    // tail records (LDS-table misses, count 1): map workgroup w appends the records of bucket b to
    // pool records [rbase[b] + w * bcap[b], + bcap[b]); record i = MRG_TAIL_BYTES(indexer) bytes at
    // (uint8_t *)pool + i * MRG_TAIL_BYTES: wc {u64 k0, u32 high word of k1} for keys of <= 12 bytes,
    // the indexer {k0, k1, doc} (24 B)
    uint64_t *pool;
    const uint64_t *rbase;       // [NBUCKET] first record of bucket b's regions
    const uint32_t *bcap;        // [NBUCKET] records per (bucket, workgroup) region
    uint32_t *bcount;            // [grid * NBUCKET] records appended (may exceed bcap)
    // wc keys of 13..16 bytes: 16-byte records {k0, k1} in their own regions, the same layout
    uint64_t *pool16;
    const uint64_t *rbase16;
    const uint32_t *bcap16;
    uint32_t *bcount16;
    // records beyond their region's capacity: bucket b's overflow list, records
    // [b * ocap, b * ocap + min(onext[b], ocap)) of `ovf` (a full list forces a rerun)
    uint64_t *ovf;
    uint32_t *onext;             // [NBUCKET]
    uint32_t ocap;
    // LDS-table flush: workgroup g writes its entries to [g * CAP, ...) sorted by bucket;
    // foff[g * (NBUCKET + 1) + b] = start of bucket b in that region
    uint64_t *fk0, *fk1;
    uint32_t *fcnt, *fdoc, *foff;
    // long-key token records (> 16 key bytes): map workgroup w appends to its region, records
    // [w * lper, + lper), through an LDS cursor; beyond it to the shared list [grid * lper, + lovf)
    // (a device atomic each; a full list reruns the launch).  lcount[w] = records workgroup w produced
    // (may exceed lper); mrg_launch_long_compact packs them densely afterwards.
    uint64_t *lstart;
    uint32_t *llen, *ldoc;
    uint32_t lper;
    uint64_t lovf;
    uint32_t *lcount;
    // non-ASCII tiles, recorded by the main loop and processed after it: workgroup g appends the
    // index of each such tile (block * NSUB + tile, absolute) to gbits[g * kwords ..)
    uint32_t *gbits;
    uint32_t kwords;             // list capacity per workgroup (tiles of its share + its steal budget); bounds the appends
    unsigned long long *counters;
    uint32_t hash_bits;          // 0 = full; else truncate internal hashes (collision test knob)
    unsigned long long *prof;    // perf diagnostics (env MRG_PROF): per-phase wave clocks, [7]; else null
    // wide map (near-unique keys, wc): no LDS combine -- every short key goes
    // straight to its L1 bucket b = partition * wB1r + quantile (SipHash-1-3 % R, then the splitters of a
    // sample of the input), into the region of (b, this workgroup): records
    // [(b * grid + w) * wcap, + wcap) of wrec, 16 bytes {k0, k1} each; wcnt[b * grid + w] = records the
    // workgroup produced for b (may exceed wcap: the launch is then rerun with larger regions)
    uint64_t *wrec;
    uint32_t *wcnt;
    const uint64_t *wspl;        // [wR][wB1r - 1] splitter keys (k0, k1)
    const uint8_t *wix;          // [wR][MRG_WIDE_IX1] splitter index (null: binary search)
    uint32_t wR, wB1r, wcap;
    // w12: the regions hold 12-byte records {k0, high word of k1} (keys of <= 12 bytes; 4 bytes of slack
    // after the last region); a key of 13..16 bytes goes to its bucket's list of 16-byte records,
    // wl16 records [b * wl16cap, + wl16n[b]) (a device atomic each: such keys are rare when w12 is
    // chosen; a full list counts in CNT_W16 and reruns the launch with 16-byte regions)
    uint32_t w12, wl16cap;
    uint64_t *wl16;
    uint32_t *wl16n;
    // load balance (mrg_map.cpp map_steal): blocks [0, n_static) are split into
    // equal workgroup shares; blocks [n_static, n_chunks) are a pool in 8 parts, part j's next block at
    // pool_ctr[16 * j] (zeroed per launch), that a wave takes MRG_MAP_STEAL_K blocks at a time once its
    // workgroup's share is done, at most steal_max blocks per workgroup: a claim that would pass the
    // budget is not made (the per-workgroup capacities are sized for share + steal_max + one claim).
    // n_static = n_chunks: static shares only.  run: consecutive blocks of its workgroup's share a wave
    // claims per LDS atomic (MRG_MAP_RUN where a share is long enough, else shorter: mrg_map.cpp map_steal;
    // 1 = one block per claim).
    uint64_t n_static;
    uint32_t steal_max;
    uint32_t run;
    unsigned long long *pool_ctr;
};
// One staged small write of a job's setup (mrg_map.cpp stage_h2d / stage_fill): `n` bytes to `dst`, from
// offset `src` of the device copy of the pinned staging buffer, or the byte `fill` when src == ~0u.
// A batch of them is one host-to-device copy and one k_stage_scatter launch (was one copy or memset
// each, ~8 us apiece on the stream).
struct StageOp {
    uint64_t dst;
    uint32_t src, n, fill, pad;
};
void mrg_launch_stage_scatter(const uint8_t *d_stage, uint32_t table_off, uint32_t nops, hipStream_t s);

#ifndef MRG_MAP_STEAL_K
#define MRG_MAP_STEAL_K 4        // blocks a wave takes from the pool at a time
#endif
#ifndef MRG_MAP_RUN
#define MRG_MAP_RUN 4            // blocks of its workgroup's share a wave claims at a time (env MRG_MAP_RUN)
#endif
#define MRG_WMAP_MAXB1 4096      // L1 buckets the wide map's LDS cursors hold
#define MRG_WIDE_IX1 260         // bytes of one partition's L1 splitter index (257 entries + prefix bits)
#define MRG_WMAP_IXR 64          // partitions whose index fits the wide map's LDS

// A set of keys with counts (SoA).  len > 16 keys have their bytes at heap[hoff .. hoff+len).
struct KeySet {
    uint64_t *k0, *k1, *cnt, *hoff;
    uint32_t *doc, *len, *part;
};

struct TableArgs {
    uint64_t *tk0, *tk1, *tcnt;
    uint32_t *tdoc;
    uint64_t cap;                // power of two
    uint32_t hash_bits;
};

// Exchange record, MRG_XREC_BYTES = 24 (include/mrgpu.h).  Short form (len <= 16): a, b = the packed
// key, v = count (wc; a count above MRG_XREC_VMAX goes out as several records, which the receiver
// sums) or the doc id (indexer).  Long form (len > 16): a = heap offset of the key bytes in the
// sender's heap segment, b = count (wc) / 1 (indexer), v = doc id (indexer) / MRG_EMPTY_DOC (wc).
struct XRec {
    uint64_t a, b;
    uint32_t v, len;
};
static_assert(sizeof(XRec) == 24, "XRec layout");
#define MRG_XREC_VMAX 0xFFFFFFFFull
// Records per key of the export: short wc keys carry at most vmax (MRG_XREC_VMAX; smaller only as a
// test knob) of their count per record
__host__ __device__ inline uint64_t mrg_xrec_per_key(uint64_t cnt, uint32_t len, bool indexer, uint64_t vmax) {
    return (indexer || len > 16u || cnt <= vmax) ? 1ull : (cnt + vmax - 1u) / vmax;
}

// Line record of the text reduce (k_text.hip -> mrg_reduce_text): one "key value" line of an
// intermediate file; keys longer than 16 bytes are addressed in place in the file buffer.
struct LRec {
    uint64_t k0, k1, cnt;
    uint32_t doc, len;
    uint64_t heap;
};
static_assert(sizeof(LRec) == 40, "LRec layout");

// Long items: keys > 16 bytes, as raw byte ranges of `base` (input text or a received heap).
struct LongItems {
    const uint8_t *base;
    uint64_t *start;
    uint32_t *rawlen, *doc;
    uint64_t *cnt;               // null: 1 each
    uint64_t n;
    int verbatim;                // 1: the ranges hold the key bytes exactly (exchange heap, text keys);
                                 // 0: raw token bytes, X-class codepoints are dropped (wc.rs:7-8)
};

// ---- k_map.hip
// `dev_args` is device memory for one MapArgs (the kernel reads its arguments from there)
// h: the args to copy to dev_args first (nullptr: already there)
// tail64: the 64-bit tail cursors; false: the packed ones, valid only for a launch that passes
// map_tail_packed (mrg_map.cpp).  The wide map has neither.
void mrg_launch_map(const MapArgs *h, MapArgs *dev_args, int app, int grid, int lds_cap, hipStream_t s,
                    bool wide = false, bool tail64 = true);
uint64_t mrg_map_tiles(uint64_t doc_lo, uint64_t doc_hi);  // wave blocks (NSUB KiB) of a document (16-B grid)
int mrg_map_cap(int app, int lds_cap);  // LDS-table entries per map workgroup actually used for lds_cap
int mrg_map_max_grid(int app, int lds_cap, int device);
// Dense long-token records from the map's per-workgroup regions and shared list (A as launched):
// region w's min(lcount[w], lper) records, then min(counters[CNT_LONGX], lovf) list records, to
// [0, n) of (start, len, doc); n = their total (on the device: counters[CNT_LONG] when nothing was lost).
void mrg_launch_long_compact(const MapArgs &A, int grid, uint64_t *start, uint32_t *len, uint32_t *doc,
                             hipStream_t s);
void mrg_launch_long_prep(const uint8_t *base, const uint64_t *start, const uint32_t *rawlen, uint64_t n,
                          uint64_t *k0, uint64_t *k1, uint32_t *flen, uint64_t *flen64, uint64_t *fp,
                          uint32_t hash_bits, int verbatim, hipStream_t s);
void mrg_launch_long_gather(const uint8_t *base, const uint64_t *start, const uint32_t *rawlen, uint64_t n,
                            const uint64_t *dst_off, uint8_t *heap, int verbatim, hipStream_t s);

// ---- k_keys.hip
struct BucketArgs {
    const uint64_t *pool;        // MapArgs::pool (MRG_TAIL_BYTES records) and pool16 (wc, 16-byte records)
    const uint64_t *rbase;
    const uint32_t *bcap, *bcount;
    const uint64_t *pool16;
    const uint64_t *rbase16;
    const uint32_t *bcap16, *bcount16;
    const uint64_t *movf;        // map-side overflow lists (MapArgs::ovf / onext / ocap)
    const uint32_t *monext;
    uint32_t mocap;
    const uint64_t *fk0, *fk1;
    const uint32_t *fcnt, *fdoc, *foff;
    uint32_t nreg, regcap;       // map workgroups (flush regions) and entries per region
    // keys that do not fit a bucket's LDS table (exact overflow, aggregated in the HBM table)
    uint64_t *ok0, *ok1;
    uint32_t *ocnt, *odoc;
    uint64_t ocap;
    KeySet out;
    unsigned long long *counters;
    uint32_t hash_bits;
    uint32_t nsub;               // workgroups per bucket, each summing one hash sub-range (1 = whole bucket)
    uint64_t kcap;               // capacity of `out` (keys beyond it are counted, not written)
    uint32_t n_reduce;           // partition of every key written (SipHash-1-3 % n_reduce; 0 = leave to k_partition)
};
// count32: the job has fewer than 2^32 tokens (32-bit LDS counts, a larger table); nreg <= 1024 then
void mrg_launch_bucket_agg(const BucketArgs &a, bool indexer, bool count32, hipStream_t s);
// wide (sort-based) aggregation of the map records, wc only (k_keys.hip)
struct SortRec;
void mrg_launch_wide_counts(const BucketArgs &a, uint64_t *cnt, uint64_t nseg, hipStream_t s);
void mrg_launch_wide_gather(const BucketArgs &a, const uint64_t *off, uint64_t nseg, uint32_t n_reduce, SortRec *out,
                            hipStream_t s);
void mrg_launch_wide_heads(const SortRec *r, uint64_t n, uint64_t *head, uint64_t *cv, hipStream_t s);
void mrg_launch_wide_keys(const SortRec *r, uint64_t n, const uint64_t *head, const uint64_t *E, KeySet ks,
                          uint64_t *F, hipStream_t s);
void mrg_launch_wide_cnt(const uint64_t *F, uint64_t runs, uint64_t n, const uint64_t *C, uint64_t ctot, KeySet ks,
                         hipStream_t s);
void mrg_launch_table_clear(const TableArgs &t, bool indexer, hipStream_t s);
void mrg_launch_table_insert(const TableArgs &t, const uint64_t *k0, const uint64_t *k1, const uint32_t *cnt32,
                             const uint32_t *doc, uint64_t n, bool indexer, hipStream_t s);
void mrg_launch_table_insert_x(const TableArgs &t, const XRec *x, uint64_t n, bool indexer, hipStream_t s);
void mrg_launch_table_insert_l(const TableArgs &t, const LRec *x, uint64_t n, bool indexer, hipStream_t s);
void mrg_launch_table_compact(const TableArgs &t, bool indexer, KeySet out, unsigned long long *counter,
                              hipStream_t s);
void mrg_launch_partition(KeySet ks, const uint8_t *heap, uint64_t n, uint32_t n_reduce, hipStream_t s);
void mrg_launch_long_group(const uint64_t *fp_sorted, const uint32_t *idx_sorted, const uint32_t *doc,
                           const uint8_t *heap, const uint64_t *hoff, const uint32_t *flen, uint64_t n,
                           uint32_t *rep, hipStream_t s);
void mrg_launch_long_emit(const uint32_t *rep, const uint64_t *cnt_in, const uint64_t *k0, const uint64_t *k1,
                          const uint32_t *flen, const uint64_t *hoff, const uint32_t *doc, uint64_t n,
                          unsigned long long *acc, KeySet out, unsigned long long *counter, bool indexer,
                          hipStream_t s);
void mrg_launch_x_split_long(const XRec *x, uint64_t n, const uint64_t *seg_rec_end, const uint64_t *seg_heap_base,
                             uint32_t n_segs, LongItems li, unsigned long long *counter, bool indexer, hipStream_t s);
void mrg_launch_l_split_long(const LRec *x, uint64_t n, const uint64_t *seg_rec_end, const uint64_t *seg_heap_base,
                             uint32_t n_segs, LongItems li, unsigned long long *counter, hipStream_t s);
void mrg_launch_export_count(KeySet ks, uint64_t n, uint32_t n_owners, unsigned long long *rec_cnt,
                             unsigned long long *heap_cnt, bool indexer, uint64_t vmax, hipStream_t s);
void mrg_launch_export_pack(KeySet ks, const uint8_t *heap, uint64_t n, uint32_t n_owners,
                            const uint64_t *rec_base, const uint64_t *heap_base, unsigned long long *rec_cur,
                            unsigned long long *heap_cur, XRec *out, uint8_t *out_heap, bool indexer, uint64_t vmax,
                            hipStream_t s);
// carry (wc, counts not changed after the sort): count and length in the record's doc / pad words
void mrg_launch_make_sortrec(KeySet ks, uint64_t n, const uint32_t *doc_rank, void *recs, hipStream_t s,
                             bool carry = false);
// *d_max (zeroed by the caller) = the largest document id of the n keys (indexer: checked against the names)
void mrg_launch_max_doc(KeySet ks, uint64_t n, uint32_t *d_max, hipStream_t s);
void mrg_launch_fill_u32(uint32_t *p, uint32_t v, uint64_t n, hipStream_t s);
void mrg_launch_fill_u64(uint64_t *p, uint64_t v, uint64_t n, hipStream_t s);
void mrg_launch_iota_u32(uint32_t *p, uint64_t n, hipStream_t s);

// ---- k_sort.hip
uint64_t mrg_scan_tmp_elems(uint64_t n);
// exclusive scan of u64 values (in == out allowed); tmp holds mrg_scan_tmp_elems(n) u64
void mrg_scan_u64(const uint64_t *in, uint64_t *out, uint64_t n, uint64_t *tmp, hipStream_t s);
// the same for u32 values (tmp: mrg_scan_tmp_elems(n) u32)
void mrg_scan_u32(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *tmp, hipStream_t s);
struct SortRec {  // 32 bytes
    uint64_t k0, k1;
    uint32_t part, doc;
    uint32_t idx, pad;
};
struct SortPlan {
    bool use_doc, use_k1, use_k0, use_part;
    uint32_t part_bytes;   // bytes of `part` that can be non-zero
    uint32_t doc_bytes;
};
uint64_t mrg_sort_tmp_bytes(uint64_t n);
// Stable sort by (part, k0, k1, doc) ascending.  Returns the buffer (recs or alt) with the result.
SortRec *mrg_radix_sort(SortRec *recs, SortRec *alt, uint64_t n, const SortPlan &plan, void *tmp, hipStream_t s,
                        int *passes_run);
// Sort by (part, k0, k1, doc) ascending, not stable (keys distinct): MSD buckets on (part: pbits
// significant bits, leading key bits) + LDS bitonic sort per bucket; oversized buckets by the LSD
// sort.  Returns recs or alt; *n_big = oversized buckets (more than 16: the whole array went through
// the LSD sort).
SortRec *mrg_msd_sort(SortRec *recs, SortRec *alt, uint64_t n, uint32_t pbits, const SortPlan &plan, void *tmp,
                      hipStream_t s, uint32_t *n_big, uint32_t *h_pinned);
// The same in two halves, with no host wait in between: _launch enqueues the MSD passes and an async
// copy of the oversized-bucket count into *h_nbig (pinned); once the stream has reached it, _finish
// sorts the oversized buckets (if any) and returns recs or alt like mrg_msd_sort.
void mrg_msd_sort_launch(SortRec *recs, SortRec *alt, uint64_t n, uint32_t pbits, void *tmp, hipStream_t s,
                         uint32_t *h_nbig);
SortRec *mrg_msd_sort_finish(SortRec *recs, SortRec *alt, uint64_t n, const SortPlan &plan, void *tmp, hipStream_t s,
                             uint32_t nb);
// Stable sort of (u64 key, u32 val) pairs by key, in place in (keys, vals); kv_tmp holds 4n u64.
void mrg_radix_sort_u64(uint64_t *keys, uint32_t *vals, uint64_t *kv_tmp, uint64_t n, void *tmp, hipStream_t s);
// Bare u64 keys ascending, between keys and alt (n each); only the byte passes in byte_mask run (bit q =
// key bits [8 q, 8 q + 8); every other byte must be the same in all keys).  n < 2^32.  Returns the buffer
// (keys or alt) with the result; tmp holds mrg_sort_u64_keys_tmp_bytes(n) bytes.
uint64_t mrg_sort_u64_keys_tmp_bytes(uint64_t n);
uint64_t *mrg_radix_sort_u64_keys(uint64_t *keys, uint64_t *alt, uint64_t n, uint32_t byte_mask, void *tmp,
                                  hipStream_t s, int *passes_run);
// One entry of the document-term matrix on its way to the inverted index (k_postings.hip).
struct PostRec {  // 12 bytes
    uint32_t term, doc, tf;
};
// Stable sort of PostRecs by term ascending, between recs and alt (n each); only the byte passes in
// byte_mask run (bit q = term bits [8 q, 8 q + 8); every other byte of the term must be the same in all
// records).  n < 2^32.  Returns the buffer (recs or alt) with the result; tmp holds
// mrg_sort_post_tmp_bytes(n) bytes.
uint64_t mrg_sort_post_tmp_bytes(uint64_t n);
PostRec *mrg_radix_sort_post(PostRec *recs, PostRec *alt, uint64_t n, uint32_t byte_mask, void *tmp, hipStream_t s,
                             int *passes_run);

// ---- k_format.hip
struct FormatArgs {
    const SortRec *recs;        // sorted by (part, key prefix, doc rank)
    uint64_t n;
    KeySet ks;
    const uint8_t *heap;
    uint64_t heap_bytes;        // bytes of the long-key heap (bounds the wc output before it is sized)
    uint32_t n_reduce;
    int drop_last;
    int indexer;
    int any_long;
    int carried;                // wc: count and length carried in the records (mrg_launch_make_sortrec)
    const uint8_t *names;       // indexer: doc names concatenated in rank order
    const uint64_t *name_off;   // [n_docs + 1], by rank
};
// Writes every mr-{r}.txt (concatenated in r order) into *out_buf (grown from the pool) and the
// partition byte offsets to part_off_host[0..n_reduce].  Returns the total byte count.
uint64_t mrg_format(const FormatArgs &f, DevPool &pool, uint8_t **out_buf, uint64_t *out_cap,
                    uint64_t *part_off_host, hipStream_t s);
// Insertion-sort runs of equal (part, 16-byte prefix) that involve a long key by full key bytes.
void mrg_launch_fix_runs(SortRec *r, uint64_t n, KeySet ks, const uint8_t *heap, hipStream_t s);
// final.txt: part2[key] = 1 for the keys the per-partition pass drops (drop-last), else 0.
void mrg_launch_final_part(const SortRec *r, uint64_t n, KeySet ks, const uint8_t *heap, int drop_last,
                           uint32_t *part2, hipStream_t s);

// ---- k_text.hip: the reference's text intermediates (mr-{m}-{r}.txt)
struct TextTok {  // one token of a map task, input order
    uint64_t k0, k1, start;
    uint32_t rawlen, klen, part, pad;
};
uint64_t mrg_text_segments(uint64_t n);  // 64-byte segments (threads) over n bytes
void mrg_launch_text_tok(const uint8_t *in, uint64_t n, uint32_t n_reduce, const uint64_t *base, uint64_t *cnt,
                         TextTok *out, unsigned long long *err, hipStream_t s);
void mrg_launch_text_keys(const TextTok *t, uint64_t n, uint64_t *part, uint32_t *idx, hipStream_t s);
void mrg_launch_text_len(const TextTok *t, const uint32_t *idx, uint64_t n, uint64_t *L, hipStream_t s);
void mrg_launch_text_part_off(const uint64_t *part, const uint64_t *O, uint64_t n, uint32_t R, uint64_t total,
                              uint64_t *part_off, hipStream_t s);
void mrg_launch_text_write(const uint8_t *in, const TextTok *t, const uint32_t *idx, uint64_t n, const uint64_t *O,
                           uint8_t *out, hipStream_t s);
void mrg_launch_utf8_check(const uint8_t *in, uint64_t n, unsigned long long *err, hipStream_t s);
void mrg_launch_text_lines(const uint8_t *in, const uint64_t *fo, const uint64_t *fe, uint32_t nf, uint64_t nseg,
                           const uint64_t *base, uint64_t *cnt, LRec *out, unsigned long long *err,
                           unsigned long long *nempty, hipStream_t s);
void mrg_launch_add_first(const SortRec *r, KeySet ks, uint64_t v, hipStream_t s);

// ---- k_wide.hip: high-cardinality aggregation by a two-level sample sort
#define MRG_WIDE_T1 65536u       // records per L1 tile
#define MRG_WIDE_MAXB2 1024u     // leaves per L1 bucket; leaf id = bucket * MRG_WIDE_MAXB2 + j
struct WideLeafArgs {
    const uint64_t *kin;         // records in leaf order (2 words each)
    uint64_t *kout;              // distinct keys (2 words each) at leaf_out[leaf] + i
    const uint64_t *bstart;      // [B1 + 1]
    const uint32_t *nleaf;       // [B1]
    const uint64_t *leaf_lo, *leaf_lb;
    uint32_t B1r, R;
    const uint64_t *wk0, *wk1, *wcnt;  // weighted keys (flushed map tables), sorted by (part, key)
    const uint32_t *wpart;
    uint64_t nw;
    uint32_t maxd;               // 0 = default capacity
    uint64_t *ocnt;
    uint64_t *leaf_out;
    uint32_t *leaf_nd;
    uint64_t *leaf_bytes;
    uint32_t *leaf_last;
    uint32_t *ovf_list;
    unsigned long long *ovf_n;
    unsigned long long *nkeys;   // += distinct keys of every finished leaf
    uint64_t *wr;                // [B1 * MRG_WIDE_MAXB2][2] scratch: weighted-key range of each leaf
    unsigned long long *prof;    // diagnostics (builds with -DMRG_WIDE_PROF): leaf phase clocks [16]
    uint32_t *big_list;          // [B1 * MRG_WIDE_MAXB2] leaves passed from the one-wave to the workgroup kernel
    unsigned long long *big_n;   // their count (zeroed by the caller)
    uint32_t *leaf_pk;           // [B1 * MRG_WIDE_MAXB2] 1: the leaf's counts are packed into its key slots (zeroed by the caller)
    uint32_t pack;               // packing allowed: every count fits 32 bits (fewer than 2^32 tokens)
    const uint64_t *leaf_hi;     // [B1 * MAXB2] one past each leaf's last record in kin
};
void mrg_wide_launch_counts(const BucketArgs &a, uint64_t *cnt_main, uint64_t *segptr, uint64_t *cnt_flush,
                            hipStream_t s);
void mrg_wide_launch_flush_gather(const BucketArgs &a, const uint64_t *off, uint64_t *k0, uint64_t *k1, uint32_t *c,
                                  hipStream_t s);
void mrg_wide_launch_sample1(const BucketArgs &a, const uint64_t *off, uint64_t nseg, uint64_t n, uint32_t S,
                             uint32_t R, SortRec *out, hipStream_t s);
void mrg_wide_launch_split1(const SortRec *smp, uint32_t S, uint32_t R, uint32_t B1r, uint64_t *spl, hipStream_t s);
size_t mrg_wide_l1_lds(uint32_t R, uint32_t B1r, uint32_t B1);
void mrg_wide_launch_l1(const BucketArgs &a, const uint64_t *off, const uint64_t *segptr, uint64_t nseg, uint64_t n,
                        const uint64_t *spl1, uint32_t R, uint32_t B1r, uint32_t *cnt, uint32_t ntiles, uint64_t *out,
                        uint16_t *bid, uint8_t *ix1, bool scatter, hipStream_t s);
void mrg_wide_launch_bstart(const uint32_t *cnt, uint32_t B1, uint32_t ntiles, uint64_t n, uint64_t *bstart,
                            hipStream_t s);
// The wide map's regions as L2 input (MapArgs::wrec / w12 / wl16 layout); rin == null: L1's output
struct WmapIn {
    const uint64_t *rin = nullptr;
    const uint32_t *soff = nullptr;  // [B1][grid + 2] segment starts (mrg_wmap_launch_seg)
    uint32_t grid = 0, wcap = 0, w12 = 0, wl16cap = 0;
    const uint64_t *wl16 = nullptr;
};
void mrg_wide_l2_prof(unsigned long long out[8]);
void mrg_wide_launch_l2(const uint64_t *in, uint64_t *out, const uint64_t *bstart, const uint64_t *spl1, uint32_t B1,
                        uint32_t B1r, uint32_t target, uint32_t *nleaf, uint64_t *leaf_lo, uint64_t *leaf_hi,
                        uint64_t *leaf_lb, uint16_t *sub, hipStream_t s, const WmapIn &wm = WmapIn{});
// wide map (near-unique input): a sample of the input text's tokens (k_wsample_text), adjacent
// duplicates of the sorted sample, the L1 splitter index, the regions' per-bucket segment starts
void mrg_wide_launch_sample_text(const uint8_t *in, const uint64_t *doc_off, uint32_t n_docs, uint64_t total,
                                 uint32_t S, uint32_t R, SortRec *out, hipStream_t s);
void mrg_wide_launch_sample_dups(const SortRec *r, uint32_t S, unsigned long long *dups, hipStream_t s);
// the cold-context near-unique test: S (<= 8192) unsorted samples, dups[0] = repeats, dups[1] = 13..16-byte keys
void mrg_wide_launch_sample_uniq(const SortRec *r, uint32_t S, unsigned long long *dups, hipStream_t s);
void mrg_wide_launch_l1ix(const uint64_t *spl1, uint32_t R, uint32_t B1r, uint8_t *ix1, hipStream_t s);
// segment starts of bucket b: soff[b * (grid + 2) + w], w < grid the regions, w = grid the 16-byte list
// (wl16n null: empty), [grid + 1] the bucket's total, also in nb[b]
void mrg_wmap_launch_seg(const uint32_t *wcnt, uint32_t B1, uint32_t grid, uint32_t wcap, const uint32_t *wl16n,
                         uint32_t wl16cap, uint32_t *soff, uint64_t *nb, hipStream_t s);
void mrg_wide_launch_weights(const SortRec *r, uint64_t n, KeySet ks, uint64_t *wk0, uint64_t *wk1, uint64_t *wcnt,
                             uint32_t *wpart, hipStream_t s);
void mrg_wide_launch_leaf(const WideLeafArgs &w, uint32_t B1, hipStream_t s);
void mrg_wide_launch_fallback(const WideLeafArgs &w, const uint32_t *list, uint32_t nlist, DevPool &pool,
                              hipStream_t s);
void mrg_wide_launch_drop(const uint32_t *nleaf, uint32_t B1r, uint32_t R, const uint32_t *leaf_nd, uint64_t *leaf_bytes,
                          const uint32_t *leaf_last, uint32_t *leaf_drop, hipStream_t s);
void mrg_wide_launch_write(const uint64_t *keys, const uint64_t *ocnt, const uint32_t *leaf_pk, const uint32_t *nleaf,
                           const uint64_t *leaf_out, const uint32_t *leaf_nd, const uint32_t *leaf_drop,
                           const uint64_t *leaf_off, uint32_t B1, uint8_t *out, hipStream_t s);
void mrg_wide_launch_part_off(const uint64_t *leaf_off, uint32_t B1r, uint32_t R, uint64_t total, uint64_t *part_off,
                              hipStream_t s);
void mrg_wide_launch_dense(const uint64_t *keys, const uint64_t *ocnt, const uint32_t *leaf_pk, const uint64_t *leaf_out,
                           const uint32_t *leaf_nd, const uint32_t *dense_off, uint32_t B1, uint32_t B1r, KeySet ks,
                           hipStream_t s);

// ---- k_topk.hip: the K most frequent keys by a radix select, wc only
// Keys are ranked by the 24-byte composite (~count, k0, k1), big-endian, smaller first: count
// descending, then the 16-byte key prefix ascending.  The select finds, one byte ("digit") at a time,
// the composite prefix below or at which the `want` best keys lie; its state lives on the device and
// every pass reads it from there (no host round trip per pass).
#define MRG_TOPK_DIGITS 24
struct TopkState {
    uint64_t pre[3];             // composite prefix found so far: its first `digit` bytes count
    uint64_t want;               // rank still wanted among the keys tied on the prefix
    uint64_t better;             // keys strictly below the prefix (all of them candidates)
    uint64_t tied;               // keys equal to the prefix (candidates too: better + tied >= want)
    unsigned long long maxcnt;   // largest count (the select starts at its first non-zero byte)
    unsigned long long ncand;    // compaction cursor (mrg_topk_compact)
    unsigned long long ndrop;    // candidates that are their partition's dropped key (mrg_topk_count_keys)
    uint32_t digit;              // prefix bytes fixed so far = the next digit to select on
    uint32_t done;               // the select has finished (the tied keys are exactly the wanted ones, or digit 24)
    uint32_t passes, pad;        // histogram passes that streamed the keys
    uint64_t parts[MRG_TOPK_DIGITS];  // keys still tied when digit d was histogrammed (0: pass not run)
    unsigned long long hist[256];
};
// Enqueues the whole select for the `want` (< n) best of n keys; *st zeroed by the caller.
void mrg_topk_select(KeySet ks, uint64_t n, uint64_t want, TopkState *st, hipStream_t s);
// Candidates (keys whose composite, cut to st->digit bytes, is <= the prefix; all keys for a zeroed
// state) as SortRecs {k0, k1, part 0, idx = key index}, at most cap of them, in no particular order.
void mrg_topk_compact(KeySet ks, uint64_t n, TopkState *st, SortRec *out, uint64_t cap, hipStream_t s);
// cand_last[p] (zeroed) = 1 + position of the byte-largest candidate of partition p in r (key order)
void mrg_topk_cand_last(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, uint32_t *cand_last, hipStream_t s);
// exceeded[p] (zeroed) = 1 when some key of partition p is byte-greater than that candidate: one
// streaming pass over all n keys (part, k0; k1 and heap bytes only on ties)
void mrg_topk_exceed(KeySet ks, const uint8_t *heap, uint64_t n, const SortRec *r, uint32_t R,
                     const uint32_t *cand_last, uint32_t *exceeded, hipStream_t s);
// keys[j] = ~count of candidate j (all ones for a dropped one: it sorts last), vals[j] = j;
// cand_last == null: nothing is dropped.  st->ndrop += dropped candidates.
void mrg_topk_count_keys(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, const uint32_t *cand_last,
                         const uint32_t *exceeded, uint64_t *keys, uint32_t *vals, TopkState *st, hipStream_t s);
void mrg_topk_gather(const SortRec *r, const uint32_t *vals, uint64_t m, SortRec *out, hipStream_t s);

// ---- k_acc.hip: the accumulator of mrg_job_map_add
// Persistent open-addressing table of the job's short keys (<= 16 bytes), SoA; empty slot: k0 =
// MRG_EMPTY_K0, k1 = MRG_EMPTY_K1, doc = MRG_EMPTY_DOC, cnt = 0.  The host keeps keys <= cap / 2.
struct AccTable {
    uint64_t *k0, *k1, *cnt;
    uint32_t *doc, *part;
    uint64_t cap;                // power of two
    uint32_t hash_bits;          // 0 = full; else the slot comes from the truncated hash (collision test knob)
};
void mrg_acc_launch_clear(const AccTable &t, hipStream_t s);
// insert-or-add the short keys of ks[0, n) (distinct among themselves, partition attached); *created +=
// keys that were new to the table
void mrg_acc_launch_fold(const AccTable &t, KeySet ks, uint64_t n, bool indexer, unsigned long long *created,
                         hipStream_t s);
void mrg_acc_launch_rehash(const AccTable &from, const AccTable &to, bool indexer, hipStream_t s);
// the full slots as a dense KeySet out[*counter ...), at most out_cap keys
void mrg_acc_launch_emit(const AccTable &t, bool indexer, KeySet out, uint64_t out_cap, unsigned long long *counter,
                         hipStream_t s);
// the long keys of ks[0, n) as long items [first + j), j counted in *counter (zeroed), over a heap in
// which ks's heap starts at heap_base; items at or beyond cap are not written
void mrg_acc_launch_long(KeySet ks, uint64_t n, uint64_t heap_base, uint64_t first, uint64_t cap, uint64_t *start,
                         uint32_t *rawlen, uint32_t *doc, uint64_t *cnt, unsigned long long *counter, hipStream_t s);

// ---- k_encode.hip: the frozen word -> id table of a vocabulary and the encoder
// Open-addressing table over the vocabulary's words, SoA; empty slot: k0 = MRG_EMPTY_K0, k1 =
// MRG_EMPTY_K1, id = 0xFFFFFFFF.  A short word's slot holds its packed key; a long word's slot holds
// (hash of its bytes | 1 << 63, 0xFF << 56 | length) and is confirmed against text + line_off[id].
struct VocTable {
    uint64_t *k0, *k1;
    uint32_t *id;
    uint64_t cap;                // power of two, >= 2 n
    uint32_t hash_bits;          // 0 = full; else truncated hashes (collision test knob, from the job's flags)
    const uint8_t *text;         // "word count\n" lines in id order
    const uint64_t *line_off;    // [n + 1]
    uint64_t n;
};
// lines [0, m) of the ranked records `top` (idx = key index in ks): len64[j] = bytes of line j
// (len64[m] = 0), wlen[j] = the word's bytes, *nkeep (zeroed) = lines whose count is >= min_count
void mrg_voc_launch_lines(const SortRec *top, uint64_t m, KeySet ks, uint64_t min_count, uint64_t *len64,
                          uint32_t *wlen, unsigned long long *nkeep, hipStream_t s);
// clear the table and insert words [0, t.n); *fail (zeroed) counts words that found no slot (never)
void mrg_voc_launch_build(const VocTable &t, const uint32_t *wlen, unsigned long long *fail, hipStream_t s);
// One encode call.  Positions are byte offsets from `in` (16-byte aligned); the documents cover [lo, hi)
// with lo < 1024; ntiles = 1 KiB chunks over [0, hi).
struct EncPlan {
    const uint8_t *in;
    uint64_t lo, hi, ntiles;
    uint32_t *bnd;               // [mrg_enc_bitmap_words(ntiles)] zeroed: the document-boundary bitmap
    const uint64_t *doc_off;     // [n_docs + 1] device copy of the offsets
    uint32_t n_docs;
    uint64_t *cnt;               // [ntiles + 1] zeroed: tokens per chunk, then (scanned in place) chunk bases
    uint64_t *tok_off;           // [n_docs + 1]
    uint32_t *out;               // the ids (emit only)
    uint64_t out_n;              // their number (tok_off[n_docs])
    unsigned long long *err;     // all ones: first invalid UTF-8 byte
    unsigned long long *info;    // [8] zeroed: tokens, UNK, long tokens, non-ASCII chunks, table probes
};
uint64_t mrg_enc_bitmap_words(uint64_t ntiles);
void mrg_enc_launch_bounds(const EncPlan &p, hipStream_t s);
void mrg_enc_launch_count(const EncPlan &p, const VocTable &t, hipStream_t s);    // fills cnt, err, info[3]
void mrg_enc_launch_offsets(const EncPlan &p, const VocTable &t, hipStream_t s);  // after the scan of cnt
void mrg_enc_launch_emit(const EncPlan &p, const VocTable &t, hipStream_t s);
// The id-indexed side of a vocabulary (mrg_vocab_decode): wlen[i] = bytes of word i, pk[2 i], pk[2 i + 1]
// = its first 16 bytes as the table packs them (k0, k1).
struct VocWords {
    uint32_t *wlen;              // [n]
    uint64_t *pk;                // [2 n], 16-byte aligned
};
// pk of words [0, t.n) from t.text and w.wlen
void mrg_voc_launch_words(const VocTable &t, const VocWords &w, hipStream_t s);
// mrg_vocab_from_text: line i of t.text is [t.line_off[i], t.line_off[i + 1]), its '\n' included.  Checks
// the form "word count\n" and the word's codepoints, writes wlen[i]; *err (all ones) = min over the bad
// lines of line * 4 + reason (MRG_VOC_BAD_*).
#define MRG_VOC_BAD_FORM 0u      // not `word`, one ' ', 1..20 ASCII digits
#define MRG_VOC_BAD_UTF8 1u
#define MRG_VOC_BAD_CLASS 2u     // a codepoint that is not \w
void mrg_voc_launch_check(const VocTable &t, uint32_t *wlen, unsigned long long *err, hipStream_t s);
// after the build: word i must find id i; *dup (all ones) = the smallest line whose word finds another
void mrg_voc_launch_verify(const VocTable &t, const uint32_t *wlen, unsigned long long *dup, hipStream_t s);

// ---- k_decode.hip: ids -> text
// One decode call.  Positions are id indices from `in` (16-byte aligned); the documents' ids are
// [lo, hi) with lo < 4; nchunks = chunks of MRG_DEC_CHUNK ids over [0, hi).
#define MRG_DEC_CHUNK 256u
struct DecPlan {
    const uint32_t *in;
    uint64_t lo, hi, nchunks;
    uint32_t *bnd;               // [mrg_dec_bitmap_words(nchunks)] zeroed: bit p = id p is its document's last
    const uint64_t *tok_off;     // [n_docs + 1] device copy of the offsets (relative to `in`)
    uint32_t n_docs;
    uint64_t *cnt;               // [nchunks + 1] zeroed: output bytes per chunk, then (scanned in place) chunk bases
    uint64_t *out_off;           // [n_docs + 1]
    uint8_t *out;                // the text (emit only)
    uint64_t out_n;              // its bytes (out_off[n_docs])
    unsigned long long *err;     // all ones: position of the first id that is not in the vocabulary
    uint32_t unk_len;            // bytes written for MRG_ID_UNK (0: such an id is an error)
    uint64_t unk_k0, unk_k1;     // unk_len <= 16: the bytes, packed as a key
    const uint8_t *unk;          // unk_len > 16: the bytes, on the device
};
uint64_t mrg_dec_bitmap_words(uint64_t nchunks);
void mrg_dec_launch_bounds(const DecPlan &p, hipStream_t s);
void mrg_dec_launch_count(const DecPlan &p, const VocTable &t, const VocWords &w, hipStream_t s);    // fills cnt, err
void mrg_dec_launch_offsets(const DecPlan &p, const VocTable &t, const VocWords &w, hipStream_t s);  // after the scan of cnt
void mrg_dec_launch_emit(const DecPlan &p, const VocTable &t, const VocWords &w, hipStream_t s);

// ---- k_terms.hip: per-document term counts of id sequences
// One mrg_vocab_term_counts call.  Positions are id indices from `in`; lists hold document indices.
struct TermsPlan {
    const uint32_t *in;
    const uint64_t *tok_off;     // [n_docs + 1] device copy of the offsets
    uint64_t n_words;            // ids >= n_words other than MRG_ID_UNK are reported in *err
    uint64_t *len;               // [n_docs + 1] zeroed: distinct ids per document, then (scanned in place) row offsets
    uint64_t *unk;               // [n_docs] zeroed: MRG_ID_UNK per document
    uint32_t *terms, *counts;    // the rows (emit only)
    unsigned long long *err;     // all ones: smallest index of an id that is not in the vocabulary (atomicMin)
};
// The documents list[0, n) of at most MRG_TERMS_WAVE_MAX (wg: MRG_TERMS_WG_MAX) ids each, one wave (one
// workgroup) per document; emit: write the rows (len holds the row offsets), else count into len / unk.
void mrg_terms_launch_lds(const TermsPlan &p, const uint32_t *list, uint32_t n, bool wg, bool emit, hipStream_t s);
// A slice of the large path: documents ldoc[0, nd), whose ids stand concatenated at soff[j] (soff[nd] = m).
struct TermsSlice {
    const uint32_t *ldoc;        // [nd] document indices
    const uint64_t *soff;        // [nd + 1]
    uint32_t nd;
    uint64_t m;                  // ids of the slice (< 2^32)
};
// keys[i] = (rank j of the document in the slice) << 32 | min(id, n_words) (MRG_ID_UNK becomes n_words)
void mrg_terms_launch_keys(const TermsPlan &p, const TermsSlice &sl, uint64_t *keys, hipStream_t s);
// over the sorted keys: flag[i] = 1 where a run of a vocabulary id starts (flag[m] = 0)
void mrg_terms_launch_flags(const uint64_t *keys, uint64_t m, uint64_t n_words, uint32_t *flag, hipStream_t s);
// E = the exclusive scan of flag: len / unk of every document of the slice
void mrg_terms_launch_rows(const TermsPlan &p, const TermsSlice &sl, const uint64_t *keys, const uint32_t *E,
                           hipStream_t s);
// pos[E[i]] = i for every run start, then the rows from (keys, E, pos); p.len holds the row offsets
void mrg_terms_launch_write(const TermsPlan &p, const TermsSlice &sl, const uint64_t *keys, const uint32_t *E,
                            uint32_t *pos, hipStream_t s);

// ---- k_postings.hip: the inverted index over ids
// One mrg_vocab_postings call.  Positions are indices into `terms`; the entries are [lo, hi).
struct PostPlan {
    const uint32_t *terms, *counts;  // the CSR (counts may be null: tf = 0)
    const uint64_t *row_off;         // [n_docs + 1] device copy of the row offsets (pack only)
    uint32_t n_docs, doc_base;
    uint64_t lo, hi;                 // row_off[0], row_off[n_docs]
    uint64_t n_words;                // terms >= n_words are reported in stat[0]
    unsigned long long *df;          // [n_words + 1] zeroed: document frequencies, then (scanned in place) offsets
    // [4]: all ones, then the smallest index of a term that is not in the vocabulary (atomicMin); zero, then
    // the entries counted in LDS; those counted with global atomics; the largest document frequency
    unsigned long long *stat;
};
void mrg_post_launch_count(const PostPlan &p, hipStream_t s);  // fills df and stat[0..3)
void mrg_post_launch_max(const PostPlan &p, hipStream_t s);    // stat[3], before df is scanned
// out[i] = (term, doc_base + row, count) of entry lo + i; needs row_off
void mrg_post_launch_pack(const PostPlan &p, PostRec *out, hipStream_t s);
void mrg_post_launch_unpack(const PostRec *in, uint64_t n, uint32_t *docs, uint32_t *tf, hipStream_t s);  // tf may be null

// ---- k_search.hip: BM25 top-k over the inverted index
// The part of one (query, position) segment of postings that falls into one window of MRG_SEARCH_TILE
// postings: [lo, hi) of d_docs / d_tf, lo >= seg_lo = the segment's first posting; `row` is the query's
// accumulator row in its chunk, idf the float idf of the position's word.  In a Boolean search (section 34) the
// two top bits of `row` carry what the tile does besides or instead of scoring, SRCH_TILE_*; a plain search
// leaves them 0 (a chunk holds at most 65535 rows).
struct SearchTile {
    uint32_t lo, hi, seg_lo, row;
    float idf;
};
#define SRCH_TILE_ROW 0x3FFFFFFFu
#define SRCH_TILE_COUNT 0x40000000u    // scores, and adds 1 to the cell's match state: the first MUST of a word
#define SRCH_TILE_EXCLUDE 0x80000000u  // scores nothing, stores SRCH_EXCLUDED into the match state: MUST_NOT
// The match state of a cell: the distinct MUST words that hold the document, or SRCH_EXCLUDED + as many once a
// MUST_NOT word held it.  A query has at most 2^20 positions, so no count reaches the top bit: a cell passes
// the filter when its state equals the query's number of distinct MUST words, and an excluded cell never does,
// wherever the MUST_NOT stood in the query.
#define SRCH_EXCLUDED 0x80000000u
struct SearchFilterRow {
    uint32_t row, need;  // the row in the chunk; its query's distinct MUST words
};
// One mrg_vocab_search call (the index, the scoring constants, the error cell) and its current chunk of
// `rows` queries: everything below `rows` is chunk scratch, indexed by the row in the chunk.
struct SearchPlan {
    const uint32_t *docs, *tf, *doc_len;
    uint32_t n_docs, doc_base;
    uint32_t shift;              // (address of docs / 4) & 3: posting p stands in window (p + shift) / MRG_SEARCH_TILE
    uint32_t tf_vec;             // tf is 16-byte aligned where docs is
    float k1, k1p1, b, avgdl;    // k1p1 = k1 + 1 (float); avgdl > 0
    unsigned long long *err;     // all ones: smallest position in docs of a posting out of range or not ascending
    uint32_t rows, k;
    uint32_t q0;                 // the chunk's first query: row r is query q0 + r
    uint32_t want;               // min(k, n_docs): the rank the select looks for
    uint64_t stride;             // floats per accumulator row: n_docs rounded up to 4
    float *acc;                  // [rows * stride] zeroed: the scores
    uint32_t *match;             // [rows * stride] zeroed: the match states of a Boolean search; null otherwise
    uint32_t *hist;              // [rows * 256] zeroed: the select's histogram of the current byte
    uint32_t *sel;               // [rows * 4]: prefix, rank still wanted, scores above the prefix, top_n
    uint32_t ntile;              // tiles of MRG_SEARCH_SEL_TILE documents per row
    uint32_t *cnt;               // [rows * ntile * 2]: documents above / at the threshold per tile, then their scans
    uint32_t *cand_doc;          // [rows * k] the candidates: document index (without doc_base), score bits
    uint32_t *cand_bits;
    uint32_t *top_n;             // [n_queries] of the whole call
    uint32_t *out_docs;          // the call's outputs
    float *out_scores;
};
#define MRG_SEARCH_SEL_TILE 1024u
// po[2 i], po[2 i + 1] = post_off[id], post_off[id + 1] of query id i (0, 0 for an id >= n_words); with df
// (mrg_vocab_search_shard: the collection's document frequencies) also dfo[i] = df[id] (0 likewise)
void mrg_search_launch_gather(const uint32_t *q_ids, uint64_t n_ids, const uint64_t *post_off, uint64_t n_words,
                              uint64_t *po, hipStream_t s, const uint64_t *df = nullptr, uint64_t *dfo = nullptr);
void mrg_search_launch_sum(const uint32_t *doc_len, uint32_t n_docs, unsigned long long *sum, hipStream_t s);  // *sum zeroed
// acc[row][doc - doc_base] += w for the n tiles at `tiles`, which belong to one position of the chunk's queries
void mrg_search_launch_acc(const SearchPlan &p, const SearchTile *tiles, uint64_t n, hipStream_t s);
// the same for tiles that carry SRCH_TILE_* (p.match is set): the second instantiation of the kernel
void mrg_search_launch_acc_bool(const SearchPlan &p, const SearchTile *tiles, uint64_t n, hipStream_t s);
// acc[row][i] = 0 where match[row][i] != need, for the n rows at `rows`: before the select
void mrg_search_launch_filter(const SearchPlan &p, const SearchFilterRow *rows, uint32_t n, hipStream_t s);
// the chunk's rows -> top_n[q0 ..] and the candidates (select, ordered compaction) -> the output rows q0 ..
void mrg_search_launch_select(const SearchPlan &p, hipStream_t s);
void mrg_search_launch_order(const SearchPlan &p, hipStream_t s);

// ---- k_merge.hip: the statistics and the merge of a sharded search
// df[w] += post_off[w + 1] - post_off[w] for the n_words words; *err (all ones): the smallest word whose
// offsets descend
void mrg_stats_launch_df(const uint64_t *post_off, uint64_t n_words, unsigned long long *df, unsigned long long *err,
                         hipStream_t s);
// One mrg_search_merge call: row (s, q) of the input is in_docs / in_bits[(s * n_queries + q) * k_in ..] with
// in_n[s * n_queries + q] <= k_in entries (a device copy of the host counts); row q of the output has k_out slots.
struct MergePlan {
    const uint32_t *in_docs, *in_bits, *in_n;
    uint32_t n_shards, n_queries, k_in, k_out;
    uint32_t *out_docs, *out_bits;
    unsigned long long *err;     // all ones: smallest flat index of an entry that is no score or out of order
};
void mrg_merge_launch(const MergePlan &m, hipStream_t s);

// ---- k_postings_merge.hip: the indexes of the shards of one collection -> one index
struct PMergeShard {  // 40 bytes; a device table of n_shards
    const uint64_t *off;         // [n_words + 1] the shard's offsets
    const uint32_t *docs, *tf;   // its n entries (null where they are not merged, or n = 0)
    uint64_t n;
    uint64_t tile0;              // the copy grid's first tile of this shard: the tiles of the lower shards
};
// One mrg_vocab_postings_merge call.
struct PMergePlan {
    const PMergeShard *sh;
    uint32_t n_shards;
    uint64_t n_words;
    uint64_t n_tiles;            // of MRG_PMERGE_TILE source entries, over all shards
    uint64_t *post_off;          // [n_words + 1] the output: summed frequencies, then (scanned in place) offsets
    uint32_t *docs, *tf;         // the outputs (tf may be null)
    uint32_t *dst;               // [n_shards * n_words]: the output position of shard s's first posting of word w
    // [2]: all ones, then the smallest word * 64 + shard that fails a check (atomicMin); zero, then the tiles that
    // lie inside one word
    unsigned long long *stat;
};
void mrg_pmerge_launch_sum(const PMergePlan &p, hipStream_t s);    // checks the offsets, fills post_off (unscanned)
void mrg_pmerge_launch_place(const PMergePlan &p, hipStream_t s);  // needs the scanned post_off; fills dst, checks the seams
void mrg_pmerge_launch_copy(const PMergePlan &p, hipStream_t s);   // needs dst

// ---- k_gen.hip
int mrg_gen_zipf_impl(uint8_t *dst, uint64_t n, uint64_t seed, uint64_t file_index, uint32_t vocab, double s, uint32_t style,
                      hipStream_t st);
int mrg_gen_unique_impl(uint8_t *dst, uint64_t n, uint64_t seed, uint64_t file_index, hipStream_t st);
