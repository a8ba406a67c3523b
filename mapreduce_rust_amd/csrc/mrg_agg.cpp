// mrg_agg.cpp -- from records to the job's distinct keys: the HBM-table and long-key
// aggregation of records that arrive from outside (aggregate); the per-bucket aggregation of the LDS-combine map's
// output (agg_launch, bucket_aggregate); the wide, sort-based aggregation (wide_aggregate, its leaves wide_finish,
// the dense form wide_densify); and the accumulator of mrg_job_map_add (acc_*, job_map_add).
// Owns c->keys, c->wide and c->acc: keysbuf_release and acc_release give them back.
// Calls: mrg_map.cpp (read_counters, flush_stage, job_map -- job_map_add maps a batch, then folds it).
// Called by: mrgpu.cpp, mrg_map.cpp, mrg_reduce.cpp (acc_emit, wide_densify), mrg_exchange.cpp (aggregate,
// acc_emit, wide_densify, acc_release), mrg_run.cpp (job_map_add).  keys_reserve and finish_keys have no caller
// outside this unit and stay local.
#include "mrg_host.h"

using namespace mrg_host;

namespace {

void acc_table_put(Pool &p, AccTable &T) {
    p.put(T.k0); p.put(T.k1); p.put(T.cnt); p.put(T.doc); p.put(T.part);
    T = AccTable{};
}

// c->keys with room for `cap` keys; on a failure it is left empty
void keys_reserve(mrg_ctx *c, uint64_t cap) {
    keysbuf_release(c->pool, c->keys);  // (first: the new arrays may be the old blocks)
    Scratch sc(c->pool);
    KeySet ks{};
    ks.k0 = sc.get<uint64_t>(cap);
    ks.k1 = sc.get<uint64_t>(cap);
    ks.cnt = sc.get<uint64_t>(cap);
    ks.hoff = sc.get<uint64_t>(cap);
    ks.doc = sc.get<uint32_t>(cap);
    ks.len = sc.get<uint32_t>(cap);
    ks.part = sc.get<uint32_t>(cap);
    sc.keep();
    c->keys.ks = ks;
    c->keys.cap = cap;
}

// Sum short-key records in the HBM table (exact; device-scope CAS) and append the distinct keys to
// c->keys (counter CNT_KEYS, which the caller has initialised).
void table_aggregate(mrg_ctx *c, const ShortSrc &src) {
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const bool idx = is_idx(c);
    if (src.n) {
        TableArgs T{};
        T.cap = pow2_at_least(2 * src.n);
        T.tk0 = sc.get<uint64_t>(T.cap);
        T.tk1 = sc.get<uint64_t>(T.cap);
        T.tcnt = sc.get<uint64_t>(T.cap);
        T.tdoc = idx ? sc.get<uint32_t>(T.cap) : nullptr;
        T.hash_bits = hash_bits(c);
        mrg_launch_table_clear(T, idx, s);
        if (src.x) mrg_launch_table_insert_x(T, src.x, src.n, idx, s);
        else if (src.lx) mrg_launch_table_insert_l(T, src.lx, src.n, idx, s);
        else mrg_launch_table_insert(T, src.k0, src.k1, src.cnt, src.doc, src.n, idx, s);
        mrg_launch_table_compact(T, idx, c->keys.ks, &c->d_cnt[CNT_KEYS], s);
    }
}

// Long keys: fingerprint sort + full-byte tie-break grouping; appends to c->keys and owns the heap.
void long_aggregate(mrg_ctx *c, LongItems li) {
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const bool idx = is_idx(c);
    if (li.n) {
        const uint64_t n = li.n;
        uint64_t *k0 = sc.get<uint64_t>(n), *k1 = sc.get<uint64_t>(n), *fp = sc.get<uint64_t>(n);
        uint64_t *fl64 = sc.get<uint64_t>(n), *hoff = sc.get<uint64_t>(n), *acc = sc.get<uint64_t>(n);
        uint32_t *fl = sc.get<uint32_t>(n), *ix = sc.get<uint32_t>(n), *rep = sc.get<uint32_t>(n);
        uint64_t *scantmp = sc.get<uint64_t>(mrg_scan_tmp_elems(n));
        mrg_launch_long_prep(li.base, li.start, li.rawlen, n, k0, k1, fl, fl64, fp, hash_bits(c), li.verbatim, s);
        mrg_scan_u64(fl64, hoff, n, scantmp, s);
        uint64_t last[2];
        HIPCHK(hipMemcpyAsync(&last[0], hoff + (n - 1), 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&last[1], fl64 + (n - 1), 8, hipMemcpyDeviceToHost, s));
        sync(c);
        const uint64_t heap_bytes = last[0] + last[1];
        c->keys.heap = pget<uint8_t>(c->pool, heap_bytes + 16);
        c->keys.heap_bytes = heap_bytes;
        mrg_launch_long_gather(li.base, li.start, li.rawlen, n, hoff, c->keys.heap, li.verbatim, s);
        // fingerprint sort (collision-safe: k_long_group compares full bytes inside equal runs)
        uint64_t *fps = sc.get<uint64_t>(n);
        HIPCHK(hipMemcpyAsync(fps, fp, 8 * n, hipMemcpyDeviceToDevice, s));
        mrg_launch_iota_u32(ix, n, s);
        uint64_t *kv = sc.get<uint64_t>(4 * n);
        void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(n));
        check_sort_n(n, "long-key fingerprint sort");
        mrg_radix_sort_u64(fps, ix, kv, n, stmp, s);
        mrg_launch_long_group(fps, ix, idx ? li.doc : nullptr, c->keys.heap, hoff, fl, n, rep, s);
        HIPCHK(hipMemsetAsync(acc, 0, 8 * n, s));
        mrg_launch_long_emit(rep, li.cnt, k0, k1, fl, hoff, li.doc, n, (unsigned long long *)acc, c->keys.ks,
                             &c->d_cnt[CNT_KEYS], idx, s);
        c->keys.any_long = true;
    }
}

// Distinct-key count + partition of every key (worker.rs:129).
// Keys [0, parted) already carry their partition (the bucket aggregation computes it as it writes them).
void finish_keys(mrg_ctx *c, bool counters_fresh = false, uint64_t parted = 0) {
    if (!counters_fresh) read_counters(c);
    c->keys.n = c->h_cnt[CNT_KEYS];
    if (c->keys.n > c->keys.cap) raise(MRG_EINVAL, "internal: key set overflow");
    if (parted < c->keys.n) {
        KeySet rest = c->keys.ks;  // SoA: the same arrays from key `parted` on (the heap offsets are absolute)
        rest.k0 += parted; rest.k1 += parted; rest.cnt += parted; rest.hoff += parted;
        rest.doc += parted; rest.len += parted; rest.part += parted;
        mrg_launch_partition(rest, c->keys.heap, c->keys.n - parted, c->R, c->stream);
    }
    c->st.distinct_keys = c->keys.n;
}

// the LDS-combine map's output (tail regions, overflow lists, flushed tables) as the aggregations read it
BucketArgs map_output(const MapArgs &A, uint32_t nreg, uint32_t regcap) {
    BucketArgs B{};
    B.pool = A.pool; B.rbase = A.rbase; B.bcap = A.bcap; B.bcount = A.bcount;
    B.pool16 = A.pool16; B.rbase16 = A.rbase16; B.bcap16 = A.bcap16; B.bcount16 = A.bcount16;
    B.movf = A.ovf; B.monext = A.onext; B.mocap = A.ocap;
    B.fk0 = A.fk0; B.fk1 = A.fk1; B.fcnt = A.fcnt; B.fdoc = A.fdoc; B.foff = A.foff;
    B.nreg = nreg; B.regcap = regcap;
    return B;
}

// Wide (sort-based) aggregation for high-cardinality inputs (k_keys.hip k_wide_*): every map
// record is gathered with its partition, sorted by (partition, key) and summed per key; the key set
// comes out in output order.
void wide_aggregate_radix(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, LongItems li) {
    hipStream_t s = c->stream;
    Scratch sc(c->pool);
    const BucketArgs B = map_output(A, nreg, regcap);
    const uint64_t nseg = 2ull * nreg * MRG_NBUCKET + nreg + MRG_NBUCKET;
    uint64_t *segc = sc.get<uint64_t>(nseg + 1), *sego = sc.get<uint64_t>(nseg + 1);
    uint64_t *stmp1 = sc.get<uint64_t>(mrg_scan_tmp_elems(nseg + 1));
    HIPCHK(hipMemsetAsync(segc + nseg, 0, 8, s));
    mrg_launch_wide_counts(B, segc, nseg, s);
    mrg_scan_u64(segc, sego, nseg + 1, stmp1, s);  // sego[nseg] = total
    uint64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, sego + nseg, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    SortRec *a = sc.get<SortRec>(std::max<uint64_t>(n, 1)), *b = sc.get<SortRec>(std::max<uint64_t>(n, 1));
    mrg_launch_wide_gather(B, sego, nseg, c->R, a, s);
    sc.put(segc); sc.put(sego); sc.put(stmp1);
    void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(n));
    int passes = 0;
    check_sort_n(n, "wide aggregation");
    SortRec *r = mrg_radix_sort(a, b, n, part_key_plan(c->R), stmp, s, &passes);
    sc.put(stmp);
    uint64_t *head = sc.get<uint64_t>(n + 1), *cv = sc.get<uint64_t>(n + 1);
    uint64_t *E = sc.get<uint64_t>(n + 1), *C = sc.get<uint64_t>(n + 1);
    uint64_t *stmp2 = sc.get<uint64_t>(mrg_scan_tmp_elems(n + 1));
    mrg_launch_wide_heads(r, n, head, cv, s);
    mrg_scan_u64(head, E, n, stmp2, s);
    mrg_scan_u64(cv, C, n, stmp2, s);
    uint64_t tail[4] = {0, 0, 0, 0};
    if (n) {
        HIPCHK(hipMemcpyAsync(&tail[0], E + (n - 1), 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&tail[1], head + (n - 1), 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&tail[2], C + (n - 1), 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&tail[3], cv + (n - 1), 8, hipMemcpyDeviceToHost, s));
    }
    sync(c);
    const uint64_t runs = tail[0] + tail[1], ctot = tail[2] + tail[3];
    keys_reserve(c, runs + li.n + 1);
    uint64_t *F = sc.get<uint64_t>(runs + 1);
    mrg_launch_wide_keys(r, n, head, E, c->keys.ks, F, s);
    mrg_launch_wide_cnt(F, runs, n, C, ctot, c->keys.ks, s);
    HIPCHK(hipMemcpyAsync(&c->d_cnt[CNT_KEYS], &runs, 8, hipMemcpyHostToDevice, s));
    sync(c);  // `runs` is a host local
    sc.put_all();  // (the long keys' blocks may reuse them)
    c->st.overflow_keys = 0;
    c->keys.sorted = li.n == 0;
    long_aggregate(c, li);
    finish_keys(c);
}

// ---- the accumulator of mrg_job_map_add (k_acc.hip)

// a cleared table of `cap` slots; its arrays are blocks of sc until the caller has made it c->acc.T
AccTable acc_table_get(mrg_ctx *c, Scratch &sc, uint64_t cap) {
    AccTable T{};
    T.k0 = sc.get<uint64_t>(cap);
    T.k1 = sc.get<uint64_t>(cap);
    T.cnt = sc.get<uint64_t>(cap);
    T.doc = sc.get<uint32_t>(cap);
    T.part = sc.get<uint32_t>(cap);
    T.cap = cap;
    T.hash_bits = hash_bits(c);
    mrg_acc_launch_clear(T, c->stream);
    return T;
}

// Room for `more` further short keys at a load of at most 1/2, so a fold can never fill the table: the
// host knows the table's key count and the batch's.  Growth re-inserts every key into a table of twice
// the size or more (the only pass over the table beside the emit).  MRG_TEST_ACC_CAP: the first
// table's slots (rounded up to a power of two >= 1024), so that growth runs on small inputs.
void acc_reserve(mrg_ctx *c, uint64_t more) {
    Acc &A = c->acc;
    const uint64_t need = pow2_at_least(2 * (A.n + more));
    Scratch sc(c->pool);
    if (!A.T.cap) {
        const uint64_t t = env_u64("MRG_TEST_ACC_CAP", 0);
        A.T = acc_table_get(c, sc, t ? pow2_at_least(t) : need);
        sc.keep();
    }
    if (A.T.cap >= need) return;
    AccTable N = acc_table_get(c, sc, std::max<uint64_t>(need, 2 * A.T.cap));
    mrg_acc_launch_rehash(A.T, N, is_idx(c), c->stream);
    HIPCHK(hipGetLastError());
    acc_table_put(c->pool, A.T);  // (the pool is stream-ordered: reused only behind the rehash)
    A.T = N;
    sc.keep();
    ++A.rehashes;
    if (getenv("MRG_DEBUG"))
        fprintf(stderr, "[mrgpu] accumulator: %llu keys rehashed into %llu slots\n", (unsigned long long)A.n,
                (unsigned long long)N.cap);
}

// Fold a dense key set (distinct keys with their partitions; long keys on b.heap) into the accumulator
// and give b's blocks back.  Short keys: one insert-or-add each (k_acc_fold).  Long keys: regrouped
// with the accumulated ones by the existing long-key path, over one concatenated heap -- O(all long
// keys) per batch; they are rare.  Everything that can fail runs before the table is touched, and the
// new long rows replace the old ones only at the end: a failing fold leaves the accumulator as it was.
void acc_fold(mrg_ctx *c, KeysBuf &b) {
    Acc &A = c->acc;
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    const bool idx = is_idx(c);
    struct Batch {  // b's blocks back on every path
        Pool &p; KeysBuf &b;
        ~Batch() { keysbuf_release(p, b); }
    } batch{p, b};
    Scratch sc(p);
    A.dirty = true;  // (also when nothing is added: the view is rebuilt from the accumulator)
    if (!b.n) return;
    acc_reserve(c, b.n);
    unsigned long long *d_n = sc.get<unsigned long long>(2);  // [0] keys new to the table, [1] the batch's long keys
    HIPCHK(hipMemsetAsync(d_n, 0, 16, s));
    bool relong = false;
    if (b.any_long) {
        const uint64_t cap = A.lng.n + b.n;
        LongItems li{};
        li.start = sc.get<uint64_t>(cap);
        li.cnt = sc.get<uint64_t>(cap);
        li.rawlen = sc.get<uint32_t>(cap);
        li.doc = sc.get<uint32_t>(cap);
        uint8_t *heap = sc.get<uint8_t>(A.lng.heap_bytes + b.heap_bytes + 16);
        li.base = heap;
        li.verbatim = 1;  // both heaps hold exact key bytes
        if (A.lng.n) {  // the accumulated rows first, their heap in front
            HIPCHK(hipMemcpyAsync(li.start, A.lng.ks.hoff, 8 * A.lng.n, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(li.cnt, A.lng.ks.cnt, 8 * A.lng.n, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(li.rawlen, A.lng.ks.len, 4 * A.lng.n, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(li.doc, A.lng.ks.doc, 4 * A.lng.n, hipMemcpyDeviceToDevice, s));
            if (A.lng.heap_bytes)
                HIPCHK(hipMemcpyAsync(heap, A.lng.heap, A.lng.heap_bytes, hipMemcpyDeviceToDevice, s));
        }
        if (b.heap_bytes)
            HIPCHK(hipMemcpyAsync(heap + A.lng.heap_bytes, b.heap, b.heap_bytes, hipMemcpyDeviceToDevice, s));
        mrg_acc_launch_long(b.ks, b.n, A.lng.heap_bytes, A.lng.n, cap, li.start, li.rawlen, li.doc, li.cnt, &d_n[1], s);
        HIPCHK(hipGetLastError());
        uint64_t nl = 0;
        HIPCHK(hipMemcpyAsync(&nl, &d_n[1], 8, hipMemcpyDeviceToHost, s));
        sync(c);
        if (nl > b.n) raise(MRG_EHIP, "internal: accumulator long-key count");
        if (nl) {  // (a failure from here on leaves a partial set in c->keys: the callers drop it)
            li.n = A.lng.n + nl;
            keys_reserve(c, li.n + 1);  // (c->keys is free here: the caller moved the batch out of it)
            HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, sizeof(unsigned long long), s));
            long_aggregate(c, li);
            read_counters(c);
            c->keys.n = c->h_cnt[CNT_KEYS];
            if (c->keys.n > li.n) raise(MRG_EHIP, "internal: accumulator long-key set overflow");
            mrg_launch_partition(c->keys.ks, c->keys.heap, c->keys.n, c->R, s);
            HIPCHK(hipGetLastError());
            relong = true;
        }
    }
    mrg_acc_launch_fold(A.T, b.ks, b.n, idx, &d_n[0], s);
    HIPCHK(hipGetLastError());
    uint64_t made = 0;
    HIPCHK(hipMemcpyAsync(&made, &d_n[0], 8, hipMemcpyDeviceToHost, s));
    sync(c);
    A.n += made;
    if (relong) {
        keysbuf_release(p, A.lng);
        A.lng = c->keys;
        c->keys = KeysBuf{};
    }
    A.dirty = true;
}

}  // namespace

namespace mrg_host __attribute__((visibility("hidden"))) {

void keysbuf_release(Pool &p, KeysBuf &k) {
    p.put(k.ks.k0); p.put(k.ks.k1); p.put(k.ks.cnt); p.put(k.ks.hoff);
    p.put(k.ks.doc); p.put(k.ks.len); p.put(k.ks.part);
    p.put(k.heap);
    k = KeysBuf{};
}

// mrg_job_begin, mrg_job_map, mrg_job_import, mrg_close: the accumulator's blocks back to the pool
void acc_release(mrg_ctx *c) {
    acc_table_put(c->pool, c->acc.T);
    keysbuf_release(c->pool, c->acc.lng);
    c->acc = Acc{};
}

// Records that arrive as exchange records (shuffle import / plugin reduce): table + long path.
void aggregate(mrg_ctx *c, const ShortSrc &src, LongItems li) {
    keys_reserve(c, src.n + li.n + 1);
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, sizeof(unsigned long long), c->stream));
    table_aggregate(c, src);
    long_aggregate(c, li);
    finish_keys(c);
}

uint64_t agg_ocap(mrg_ctx *c) {
    uint64_t ocap = std::max<uint64_t>(c->ovf_hint, 1u << 20);
    if (const uint64_t t = env_u64("MRG_TEST_AGG_OCAP", 0)) ocap = t;  // test knob: force the regrow path
    return ocap;
}

// one launch of the per-bucket aggregation over the map's output (its overflow list goes back to the
// pool with the AggLaunch, or by drop()); zero: clear the two counters it adds to (the map launch
// zeroed them)
AggLaunch agg_launch(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, uint64_t ocap, uint32_t nsub,
                     uint64_t nlong, bool c32, bool zero) {
    hipStream_t s = c->stream;
    const bool idx = is_idx(c);
    // every workgroup (bucket, sub-range) may emit a full table of keys
    keys_reserve(c, (uint64_t)MRG_NBUCKET * std::max<uint32_t>(nsub, 1u) * MRG_BA_CAP + ocap + nlong + 1);
    AggLaunch L(c->pool);
    BucketArgs &B = L.B;
    B = map_output(A, nreg, regcap);
    B.ok0 = L.own.get<uint64_t>(ocap); B.ok1 = L.own.get<uint64_t>(ocap);
    B.ocnt = L.own.get<uint32_t>(ocap); B.odoc = idx ? L.own.get<uint32_t>(ocap) : nullptr;
    B.ocap = ocap;
    B.out = c->keys.ks;
    B.counters = c->d_cnt;
    B.hash_bits = hash_bits(c);
    B.nsub = nsub;
    B.kcap = c->keys.cap;
    B.n_reduce = c->R;
    if (zero) {
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, 8, s));
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_OVF2], 0, 8, s));
    }
    mrg_launch_bucket_agg(B, idx, c32, s);
    L.nlong = nlong;
    L.c32 = c32;
    return L;
}

// Map-side records: per-bucket LDS aggregation of tail chunks + flushed map tables, exact overflow
// through the HBM table, then the long keys.
// Returns false (nothing aggregated) when far more keys miss the per-bucket tables than the overflow
// path handles well (millions of distinct keys without the tail share that selects the wide path up
// front): the caller then runs the wide aggregation on the same map output.
// pre: a launch the caller made right behind the map (before its counters reached the host), used
// when its parameters still hold -- the counters read after the map are then already its own.
bool bucket_aggregate(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, LongItems li,
                      AggLaunch *pre) {
    if (nreg > 2048) raise(MRG_EINVAL, "internal: %u map workgroups exceed the aggregation's region table", nreg);
    const bool idx = is_idx(c);
    uint64_t ocap = agg_ocap(c);
    uint32_t agg_launches = 0;
    uint32_t nsub = c->agg_nsub;
    if (const uint64_t t = env_u64("MRG_TEST_AGG_NSUB", 0)) nsub = (uint32_t)t;
    const bool dirty = pre && pre->live();  // a launch since the map: its counters need clearing before another
    for (;;) {
        ++agg_launches;
        // 32-bit LDS counts (larger table) when no key can reach 2^32: fewer tokens than that
        const bool c32 = c->h_cnt[CNT_TOKENS] < 0xFFFFFFFFull && nreg <= 512;
        AggLaunch L(c->pool);  // (its overflow list goes back where an attempt ends: before the next one's blocks)
        // the queued launch is reused only when it ran with this job's parameters: sub-ranges, overflow
        // capacity, count width, and key slots for at least the long keys the map produced (the map
        // reruns whenever its long keys exceed their capacity, which drops the queued launch, so li.n <= nlong
        // holds here; it is checked rather than assumed)
        if (pre && pre->live() && agg_launches == 1 && pre->B.nsub == nsub && pre->B.ocap == ocap &&
            li.n <= pre->nlong &&
            pre->B.kcap >= (uint64_t)MRG_NBUCKET * std::max<uint32_t>(nsub, 1u) * MRG_BA_CAP + ocap + li.n + 1 &&
            pre->c32 == c32) {
            L = std::move(*pre);  // its counters came with the map's
            c->st.spec_agg = 1;
        } else {
            if (pre && pre->live()) c->st.spec_agg = 2;
            if (pre) pre->drop();
            L = agg_launch(c, A, nreg, regcap, ocap, nsub, li.n, c32, agg_launches > 1 || dirty);
            read_counters(c);
        }
        BucketArgs &B = L.B;
        if (c->h_cnt[CNT_KEYS] > c->keys.cap)
            raise(MRG_EINVAL, "internal: bucket aggregation emitted %llu keys for %llu slots",
                  (unsigned long long)c->h_cnt[CNT_KEYS], (unsigned long long)c->keys.cap);
        const uint64_t novf = c->h_cnt[CNT_OVF2];
        if (getenv("MRG_DEBUG"))
            fprintf(stderr, "[mrgpu] bucket agg: %llu keys, %llu overflow records (cap %llu)\n",
                    (unsigned long long)c->h_cnt[CNT_KEYS], (unsigned long long)novf, (unsigned long long)ocap);
        // Many keys missed the tables (more distinct keys per bucket than a table holds): split every
        // bucket over more workgroups (each reads the whole bucket and keeps one hash sub-range), up
        // to 16; the count is remembered by the context.  Beyond that, the wide aggregation.
        const uint64_t heavy = env_u64("MRG_TEST_AGG_WIDE_OVF", 4ull << 20);
        if (novf > heavy && nsub < 16 && !env_u64("MRG_TEST_AGG_NSUB", 0)) {
            nsub = c->agg_nsub = std::min<uint32_t>(16, 2 * nsub);  // overflow counts records, not keys: double
            if (getenv("MRG_DEBUG")) fprintf(stderr, "[mrgpu] bucket agg: %llu overflow records -> %u workgroups per bucket\n", (unsigned long long)novf, nsub);
            continue;
        }
        const char *wenv = getenv("MRG_WIDE");  // MRG_WIDE=0 pins the bucket path (tests of its overflow)
        if (!idx && novf > heavy && !(wenv && atoi(wenv) == 0)) {
            c->agg_nsub = 1;  // the next job starts from one workgroup per bucket (a low-cardinality job
                              // would otherwise stream every bucket 16 times)
            if (getenv("MRG_DEBUG")) fprintf(stderr, "[mrgpu] bucket agg: %llu overflow records -> wide\n", (unsigned long long)novf);
            return false;
        }
        if (novf > ocap) {  // overflow list too small: grow (remembered) and run again
            ocap = c->ovf_hint = novf + novf / 8 + 1024;
            continue;
        }
        if (novf) {
            ShortSrc src;
            src.k0 = B.ok0; src.k1 = B.ok1; src.cnt = B.ocnt; src.doc = B.odoc; src.n = novf;
            table_aggregate(c, src);
        }
        c->st.overflow_keys = novf;
        c->st.agg_launches = agg_launches;
        c->spec_agg = !idx;
        c->spec_c32 = c32;  // the width this job allowed (not the one a reused launch happened to use)
        c->st.agg_path = 1;
        c->wide_hint = false;
        {  // the next job's workgroups per bucket: enough sub-ranges for this job's key count, each
           // sub-range's table at most 5/6 full.  Each sub-range is one more pass over the bucket's
           // tail stream: zipf_u (2.9 M keys) aggregates in 6.9 ms at 1 (2 M records overflow to the
           // HBM table), 3.6 ms at 2 (81 % full, no overflow), 4.2 ms at 3 (profiles/r04/v34_*)
            const uint64_t slots = idx ? 4096u : (c32 ? 6912u : 6112u);  // k_keys.hip ba_cap
            const uint64_t per = (uint64_t)MRG_NBUCKET * (slots * 5u / 6u);
            c->agg_nsub = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, (c->h_cnt[CNT_KEYS] + per - 1) / per));
        }
        break;
    }
    // the counters read after the aggregation are still current unless more keys were appended; the
    // keys it wrote already carry their partition
    const bool fresh = c->st.overflow_keys == 0 && li.n == 0;
    const uint64_t parted = std::min<uint64_t>(c->h_cnt[CNT_KEYS], c->keys.cap);
    long_aggregate(c, li);
    finish_keys(c, fresh, parted);
    return true;
}

// radix sort by (partition < R, the 16 key bytes of a short key)
SortPlan part_key_plan(uint32_t R) {
    SortPlan plan{};
    plan.use_part = R > 1;
    plan.part_bytes = bytes_for(R - 1);
    plan.use_k0 = plan.use_k1 = true;
    return plan;
}

// The wide result as a dense KeySet (sorted by partition and key) for the consumers other than the
// line writer (export, final.txt, long keys appended); `extra` more slots are reserved.
void wide_densify(mrg_ctx *c, uint64_t extra) {
    WideRes &w = c->wide;
    if (!w.ready) return;
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint64_t nl = (uint64_t)w.B1 * MRG_WIDE_MAXB2;
    uint32_t *doff = sc.get<uint32_t>(nl + 1);
    uint32_t *tmp = sc.get<uint32_t>(mrg_scan_tmp_elems(nl + 1));
    mrg_scan_u32(w.leaf_nd, doff, nl, tmp, s);
    keys_reserve(c, w.distinct + extra + 1);
    mrg_wide_launch_dense(w.kout, w.ocnt, w.leaf_pk, w.leaf_out, w.leaf_nd, doff, w.B1, w.B1r, c->keys.ks, s);
    HIPCHK(hipMemcpyAsync(&c->d_cnt[CNT_KEYS], &w.distinct, 8, hipMemcpyHostToDevice, s));
    sync(c);
    c->keys.n = w.distinct;
    c->keys.sorted = true;
    w.release(c->pool);
}

// Wide aggregation by the two-level sample sort (k_wide.hip): the map's count-1 records go through
// L1 (partition + global quantile splitters) and L2 (per-bucket splitters) into leaves; the flushed
// map-table entries (weighted) are aggregated apart, sorted, and merged into their leaves.
// The wide aggregation after L1: L2 leaves inside every L1 bucket (input: the L1 output K1 in bucket
// order with bstart, or -- rin != null -- the wide map's regions, segments soff), the leaves, the
// overflowing leaves' fallback, then the long keys.  K1 becomes the output key array; bid holds the
// L2 leaf id of every record.  `own` holds K1 (kept in c->wide), bstart, spl1, bid and wk*; the blocks
// taken here join them, and all go back before the long keys' blocks are taken.
void wide_finish(mrg_ctx *c, Scratch &own, const WideL1 &l1, LongItems li, PhaseClock &clock) {
    hipStream_t s = c->stream;
    const uint32_t R = c->R, B1 = l1.B1, B1r = l1.B1r;
    const uint64_t n = l1.n, nw = l1.nw;
    uint64_t *K1 = l1.K1;
    const WmapIn &wm = l1.wm;
    // ---- L2: leaves inside every L1 bucket
    const uint64_t NL = (uint64_t)B1 * MRG_WIDE_MAXB2;
    uint64_t *K2 = own.get<uint64_t>(2 * (n + 1) + 2);
    uint32_t *nleaf = own.get<uint32_t>(B1);
    uint64_t *leaf_lo = own.get<uint64_t>(NL + 1), *leaf_lb = own.get<uint64_t>(2 * NL + 2);
    uint64_t *leaf_hi = own.get<uint64_t>(NL + 1);
    // records per leaf: the wide map's digit leaves come out near the target (320: r05 v61), the sampled
    // splitters' leaves vary like 8-sample gaps (256 keeps most under the one-wave capacity)
    const uint32_t target = (uint32_t)env_u64("MRG_TEST_LEAF_TARGET", wm.rin ? 320 : 256);
    mrg_wide_launch_l2(wm.rin ? nullptr : K1, K2, l1.bstart, l1.spl1, B1, B1r, target, nleaf, leaf_lo, leaf_hi, leaf_lb,
                       l1.bid, s, wm);
    own.put(l1.bid);
    clock.mark("L2");
    // ---- leaves: aggregate + sort + line bytes (K1 becomes the output key array)
    WideRes &w = c->wide;
    Pool &p = c->pool;
    w.release(p);
    w.B1 = B1;
    w.B1r = B1r;
    w.kout = own.release(K1);
    w.ocnt = pget<uint64_t>(p, n + nw + 1);
    w.nleaf = own.release(nleaf);
    w.leaf_out = pget<uint64_t>(p, NL);
    w.leaf_nd = pget<uint32_t>(p, NL + 1);
    w.leaf_bytes = pget<uint64_t>(p, NL + 1);
    w.leaf_last = pget<uint32_t>(p, NL);
    w.leaf_pk = pget<uint32_t>(p, NL);
    HIPCHK(hipMemsetAsync(w.leaf_pk, 0, 4 * NL, s));
    HIPCHK(hipMemsetAsync(w.leaf_nd, 0, 4 * (NL + 1), s));
    HIPCHK(hipMemsetAsync(w.leaf_bytes, 0, 8 * (NL + 1), s));
    uint32_t *ovf_list = own.get<uint32_t>(NL);
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, 8, s));
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_OVF2], 0, 8, s));
    WideLeafArgs L{};
    L.kin = K2; L.kout = K1; L.bstart = l1.bstart; L.nleaf = nleaf; L.leaf_lo = leaf_lo; L.leaf_lb = leaf_lb;
    L.leaf_hi = leaf_hi;
    L.B1r = B1r; L.R = R; L.wk0 = l1.wk0; L.wk1 = l1.wk1; L.wcnt = l1.wcnt; L.wpart = l1.wpart; L.nw = nw;
    L.maxd = (uint32_t)env_u64("MRG_TEST_LEAF_CAP", 0);
    L.ocnt = w.ocnt; L.leaf_out = w.leaf_out; L.leaf_nd = w.leaf_nd; L.leaf_bytes = w.leaf_bytes;
    L.leaf_last = w.leaf_last; L.ovf_list = ovf_list; L.ovf_n = &c->d_cnt[CNT_OVF2]; L.nkeys = &c->d_cnt[CNT_KEYS];
    L.wr = own.get<uint64_t>(2 * NL);
    L.prof = own.get<unsigned long long>(16);
    HIPCHK(hipMemsetAsync(L.prof, 0, 128, s));
    L.big_list = own.get<uint32_t>(NL);
    L.big_n = own.get<unsigned long long>(1);
    L.leaf_pk = w.leaf_pk;
    // counts packed into the key slots of leaves whose keys are <= 12 bytes: every count fits 32 bits
    // when the job has fewer than 2^32 tokens (MRG_TEST_NO_PACK: the unpacked layout everywhere)
    L.pack = (c->h_cnt[CNT_TOKENS] < 0xFFFFFFFFull && !getenv("MRG_TEST_NO_PACK")) ? 1u : 0u;
    HIPCHK(hipMemsetAsync(L.big_n, 0, 8, s));
    mrg_wide_launch_leaf(L, B1, s);
    clock.mark("leaves");
    read_counters(c);
    const uint64_t novf = c->h_cnt[CNT_OVF2];
    if (novf) mrg_wide_launch_fallback(L, ovf_list, (uint32_t)novf, p, s);
    clock.mark("fallback");
    read_counters(c);
    w.distinct = c->h_cnt[CNT_KEYS];
    w.ready = true;
    if (clock.on) {
        clock.report();
        unsigned long long pr[16], nbig = 0;
        HIPCHK(hipMemcpy(pr, L.prof, sizeof pr, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&nbig, L.big_n, 8, hipMemcpyDeviceToHost));
        fprintf(stderr, "[mrgpu] wide: %llu passed to the workgroup kernel (%llu by size, %llu by bucket)\n", nbig,
                pr[6], pr[7]);
        {  // leaf sizes (records)
            std::vector<uint32_t> hn(B1);
            std::vector<uint64_t> hlo(NL), hhi(NL);
            HIPCHK(hipMemcpy(hn.data(), nleaf, 4ull * B1, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hlo.data(), leaf_lo, 8ull * NL, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hhi.data(), leaf_hi, 8ull * NL, hipMemcpyDeviceToHost));
            std::vector<uint64_t> sz;
            for (uint32_t bb = 0; bb < B1; ++bb)
                for (uint32_t j = 0; j < hn[bb]; ++j) {
                    const uint64_t lid = (uint64_t)bb * MRG_WIDE_MAXB2 + j;
                    sz.push_back(hhi[lid] - hlo[lid]);
                }
            std::sort(sz.begin(), sz.end());
            if (!sz.empty())
                fprintf(stderr, "[mrgpu] wide: %zu leaves, records p10 %llu p50 %llu p63 %llu p87 %llu p99 %llu max %llu\n",
                        sz.size(), (unsigned long long)sz[sz.size() / 10], (unsigned long long)sz[sz.size() / 2],
                        (unsigned long long)sz[sz.size() * 63 / 100], (unsigned long long)sz[sz.size() * 87 / 100],
                        (unsigned long long)sz[sz.size() * 99 / 100], (unsigned long long)sz.back());
        }
        if (pr[0] | pr[1] | pr[5])
            fprintf(stderr, "[mrgpu] leaf phase clocks (wave 0, all WGs): clear %.3g insert %.3g list %.3g digits %.3g "
                            "order %.3g write %.3g\n", (double)pr[0], (double)pr[1], (double)pr[2], (double)pr[3],
                    (double)pr[4], (double)pr[5]);
        if (pr[8] | pr[12])
            fprintf(stderr, "[mrgpu] one-wave leaf phase clocks (all waves): load %.3g bits %.3g digits %.3g order %.3g "
                            "runs %.3g stats %.3g\n", (double)pr[8], (double)pr[9], (double)pr[10], (double)pr[11],
                    (double)pr[12], (double)pr[13]);
        {
            unsigned long long l2[8];
            mrg_wide_l2_prof(l2);
            if (l2[6])
                fprintf(stderr, "[mrgpu] L2 phase clocks (thread 0, all WGs, cumulative): segs %.3g sample %.3g sort %.3g "
                                "index %.3g hist %.3g scan %.3g scatter %.3g\n", (double)l2[0], (double)l2[1],
                        (double)l2[2], (double)l2[3], (double)l2[4], (double)l2[5], (double)l2[6]);
        }
        if (pr[14])
            fprintf(stderr, "[mrgpu] one-wave leaves: digits used %.3g, largest digit bucket %.3g (sums)\n", (double)pr[14],
                    (double)pr[15]);
    }
    if (getenv("MRG_DEBUG"))
        fprintf(stderr, "[mrgpu] wide: %llu records, %llu weighted, B1 %u (x%u), %llu distinct, %llu leaves overflowed\n",
                (unsigned long long)n, (unsigned long long)nw, B1, B1r, (unsigned long long)w.distinct,
                (unsigned long long)novf);
    own.put_all();
    c->st.overflow_keys = novf;
    c->keys.n = 0;
    c->st.distinct_keys = w.distinct;
    if (li.n) {  // long keys: the dense key set plus the long keys, sorted by the generic path
        wide_densify(c, li.n);
        long_aggregate(c, li);
        finish_keys(c);
        c->keys.sorted = false;
    }
}

void wide_aggregate(mrg_ctx *c, const MapArgs &A, uint32_t nreg, uint32_t regcap, LongItems li) {
    const uint32_t R = c->R;
    if (R > 4096) {  // the L1 histogram holds R x B1r buckets in LDS
        wide_aggregate_radix(c, A, nreg, regcap, li);
        return;
    }
    Scratch sc(c->pool);   // what the L1 passes need
    Scratch fin(c->pool);  // what wide_finish takes over
    hipStream_t s = c->stream;
    const BucketArgs B = map_output(A, nreg, regcap);
    PhaseClock clock(s);
    clock.mark("start");
    // ---- segment sizes: main (count 1) and flushed tables (weighted)
    const uint64_t nsm = 2ull * nreg * MRG_NBUCKET + MRG_NBUCKET;  // 12-byte regions, overflow lists, 16-byte regions
    uint64_t *cm = sc.get<uint64_t>(nsm + 1), *om = sc.get<uint64_t>(nsm + 1), *segptr = sc.get<uint64_t>(nsm);
    uint64_t *cf = sc.get<uint64_t>(nreg + 1), *of = sc.get<uint64_t>(nreg + 1);
    uint64_t *st1 = sc.get<uint64_t>(mrg_scan_tmp_elems(nsm + 1));
    HIPCHK(hipMemsetAsync(cm + nsm, 0, 8, s));
    HIPCHK(hipMemsetAsync(cf + nreg, 0, 8, s));
    mrg_wide_launch_counts(B, cm, segptr, cf, s);
    mrg_scan_u64(cm, om, nsm + 1, st1, s);
    mrg_scan_u64(cf, of, nreg + 1, st1, s);
    uint64_t nn[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&nn[0], om + nsm, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nn[1], of + nreg, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    const uint64_t n = nn[0], nf = nn[1];
    if (n >= 0xFFFFFFF0ull) raise(MRG_ENOMEM, "wide aggregation: %llu records exceed one GPU's 32-bit record index",
                                  (unsigned long long)n);
    // ---- weighted keys: HBM-table aggregation of the flushed entries, sorted by (partition, key)
    uint64_t nw = 0;
    uint64_t *wk0 = fin.get<uint64_t>(nf + 1), *wk1 = fin.get<uint64_t>(nf + 1), *wcnt = fin.get<uint64_t>(nf + 1);
    uint32_t *wpart = fin.get<uint32_t>(nf + 1);
    if (nf) {
        Scratch t(c->pool);
        uint64_t *fk0 = t.get<uint64_t>(nf), *fk1 = t.get<uint64_t>(nf);
        uint32_t *fc = t.get<uint32_t>(nf);
        mrg_wide_launch_flush_gather(B, of, fk0, fk1, fc, s);
        KeySet ks{};
        ks.k0 = t.get<uint64_t>(nf); ks.k1 = t.get<uint64_t>(nf); ks.cnt = t.get<uint64_t>(nf);
        ks.hoff = t.get<uint64_t>(nf); ks.doc = t.get<uint32_t>(nf); ks.len = t.get<uint32_t>(nf);
        ks.part = t.get<uint32_t>(nf);
        TableArgs T{};
        T.cap = pow2_at_least(2 * nf);
        T.tk0 = t.get<uint64_t>(T.cap); T.tk1 = t.get<uint64_t>(T.cap); T.tcnt = t.get<uint64_t>(T.cap);
        T.hash_bits = hash_bits(c);
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, 8, s));
        mrg_launch_table_clear(T, false, s);
        mrg_launch_table_insert(T, fk0, fk1, fc, nullptr, nf, false, s);
        mrg_launch_table_compact(T, false, ks, &c->d_cnt[CNT_KEYS], s);
        read_counters(c);
        nw = c->h_cnt[CNT_KEYS];
        mrg_launch_partition(ks, nullptr, nw, R, s);
        SortRec *ra = t.get<SortRec>(nw), *rb = t.get<SortRec>(nw);
        void *stmp = t.get<uint8_t>(mrg_sort_tmp_bytes(nw));
        mrg_launch_make_sortrec(ks, nw, nullptr, ra, s);
        int passes = 0;
        SortRec *srt = mrg_radix_sort(ra, rb, nw, part_key_plan(R), stmp, s, &passes);
        mrg_wide_launch_weights(srt, nw, ks, wk0, wk1, wcnt, wpart, s);
        sync(c);
    }
    clock.mark("weights");
    // ---- L1 buckets: R partitions x B1r quantile ranges of about 2^18 records
    uint32_t B1r = (uint32_t)std::min<uint64_t>((n + ((uint64_t)R << 18) - 1) / ((uint64_t)R << 18), 64);
    B1r = std::max<uint32_t>(1, std::min<uint32_t>(B1r, std::max<uint32_t>(1, 4096 / R)));
    const uint32_t B1 = R * B1r;
    uint64_t *spl1 = fin.get<uint64_t>(2ull * R * B1r + 2);
    if (B1r > 1 && n) {
        Scratch t(c->pool);
        const uint32_t S1 = (uint32_t)std::min<uint64_t>(64ull * B1, n);
        SortRec *sa = t.get<SortRec>(S1), *sb = t.get<SortRec>(S1);
        void *stmp = t.get<uint8_t>(mrg_sort_tmp_bytes(S1));
        mrg_wide_launch_sample1(B, om, nsm, n, S1, R, sa, s);
        int passes = 0;
        SortRec *srt = mrg_radix_sort(sa, sb, S1, part_key_plan(R), stmp, s, &passes);
        mrg_wide_launch_split1(srt, S1, R, B1r, spl1, s);
        sync(c);
    }
    clock.mark("splitters");
    const uint32_t ntiles = (uint32_t)std::max<uint64_t>(1, (n + MRG_WIDE_T1 - 1) / MRG_WIDE_T1);
    uint32_t *cnt1 = sc.get<uint32_t>((uint64_t)B1 * ntiles + 1);
    uint32_t *st2 = sc.get<uint32_t>(mrg_scan_tmp_elems((uint64_t)B1 * ntiles + 1));
    uint64_t *K1 = fin.get<uint64_t>(2 * (n + nw) + 2);
    uint64_t *bstart = fin.get<uint64_t>(B1 + 1);
    uint16_t *bid = fin.get<uint16_t>(std::max<uint64_t>(n, 1));   // L1 bucket, then L2 leaf, of each record
    uint8_t *ix1 = sc.get<uint8_t>(260ull * R);
    if (n) {
        mrg_wide_launch_l1(B, om, segptr, nsm, n, spl1, R, B1r, cnt1, ntiles, K1, bid, ix1, false, s);
        mrg_scan_u32(cnt1, cnt1, (uint64_t)B1 * ntiles, st2, s);
        mrg_wide_launch_l1(B, om, segptr, nsm, n, spl1, R, B1r, cnt1, ntiles, K1, bid, nullptr, true, s);
    } else {
        HIPCHK(hipMemsetAsync(cnt1, 0, 4ull * B1 * ntiles, s));
    }
    mrg_wide_launch_bstart(cnt1, B1, ntiles, n, bstart, s);
    sc.put_all();
    clock.mark("L1");
    WideL1 l1;
    l1.n = n; l1.nw = nw; l1.B1 = B1; l1.B1r = B1r;
    l1.K1 = K1; l1.bstart = bstart; l1.spl1 = spl1; l1.bid = bid;
    l1.wk0 = wk0; l1.wk1 = wk1; l1.wcnt = wcnt; l1.wpart = wpart;
    wide_finish(c, fin, l1, li, clock);
}

// The accumulator as the job's dense KeySet (unsorted, as after an import), for the consumers: at the
// first consumer call after a fold.  The table stays, so further batches can follow.
void acc_emit(mrg_ctx *c) {
    Acc &A = c->acc;
    if (!A.on || !A.dirty) return;
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    const uint64_t n = A.n + A.lng.n;
    c->wide.release(p);
    keys_reserve(c, n + 1);
    KeysBuf &k = c->keys;
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, sizeof(unsigned long long), s));
    if (A.T.cap) mrg_acc_launch_emit(A.T, is_idx(c), k.ks, A.n, &c->d_cnt[CNT_KEYS], s);
    HIPCHK(hipGetLastError());
    if (A.lng.n) {  // the long rows behind the short keys; their heap offsets stay valid in a copy of the heap
        const KeySet &l = A.lng.ks;
        const uint64_t m = A.lng.n;
        HIPCHK(hipMemcpyAsync(k.ks.k0 + A.n, l.k0, 8 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.k1 + A.n, l.k1, 8 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.cnt + A.n, l.cnt, 8 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.hoff + A.n, l.hoff, 8 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.doc + A.n, l.doc, 4 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.len + A.n, l.len, 4 * m, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(k.ks.part + A.n, l.part, 4 * m, hipMemcpyDeviceToDevice, s));
        k.heap = pget<uint8_t>(p, A.lng.heap_bytes + 16);
        if (A.lng.heap_bytes)
            HIPCHK(hipMemcpyAsync(k.heap, A.lng.heap, A.lng.heap_bytes, hipMemcpyDeviceToDevice, s));
        k.heap_bytes = A.lng.heap_bytes;
        k.any_long = true;
    }
    read_counters(c);
    if (c->h_cnt[CNT_KEYS] != A.n)
        raise(MRG_EHIP, "internal: accumulator holds %llu keys, %llu expected", (unsigned long long)c->h_cnt[CNT_KEYS],
              (unsigned long long)A.n);
    k.n = n;
    k.sorted = false;
    c->st.distinct_keys = n;
    A.dirty = false;
}

// mrg_job_map_add: map the input like mrg_job_map, then ADD the batch's keys to the job's.
void job_map_add(mrg_ctx *c) {
    need_job(c);
    if (c->doc_off.empty()) raise(MRG_EINVAL, "no input: call mrg_job_set_input first");
    Acc &A = c->acc;
    flush_stage(c);  // (nothing is pending between calls: every map launch flushes first)
    sync(c);
    c->stage_used = c->pend_lo = 0;  // the previous batch's staged copies are done: the staging region is free
    if (!A.on) {  // the keys the job holds already (mrg_job_map / mrg_job_import) come first
        if (c->keyed) {
            wide_densify(c, 0);
            A.on = A.seeded = true;
            A.in_bytes = c->st.input_bytes;
            A.tokens = c->st.tokens;
            A.long_tokens = c->st.long_tokens;
            KeysBuf b = c->keys;
            c->keys = KeysBuf{};
            c->keyed = false;
            try {
                acc_fold(c, b);
            } catch (...) {  // (out of memory with the keys already moved: the job is left without keys)
                acc_release(c);
                keysbuf_release(c->pool, c->keys);  // (a long-key set the fold had begun)
                c->mapped = false;
                throw;
            }
        }
        A.on = true;
    }
    // the job's keys are in the accumulator; c->keys is a view of it, which the map below rebuilds for
    // the batch alone -- so a batch that fails leaves the job with exactly the keys it had
    const mrg_stats st0 = c->st;
    const bool had = A.seeded || A.batches;
    try {
        job_map(c);
        wide_densify(c, 0);
        KeysBuf b = c->keys;
        c->keys = KeysBuf{};
        c->keyed = false;
        acc_fold(c, b);
        ev_rec(c, c->ev, 7);
        A.ms_fold = ev_ms(c, c->ev, 3, 7);
    } catch (...) {
        keysbuf_release(c->pool, c->keys);
        c->wide.release(c->pool);
        c->keyed = false;
        c->st = st0;
        c->mapped = had;
        c->reduced = false;
        A.dirty = true;
        throw;
    }
    A.in_bytes += c->st.input_bytes;
    A.tokens += c->st.tokens;
    A.long_tokens += c->st.long_tokens;
    ++A.batches;
    c->st.input_bytes = A.in_bytes;
    c->st.tokens = A.tokens;
    c->st.long_tokens = A.long_tokens;
    c->st.map_batches = A.batches;
    c->st.distinct_keys = A.n + A.lng.n;
    c->mapped = true;
    c->reduced = false;
    // the device has read the last of the batch's buffer (acc_fold waited for the stream): the caller
    // may overwrite or free it; the next batch needs its own mrg_job_set_input
    c->d_in = nullptr;
    c->doc_off.clear();
    c->doc_ids.clear();
}

}  // namespace mrg_host
