// mrg_map.cpp -- the map stage of a job: the staged small writes of a job's setup
// (stage_h2d, stage_fill, flush_stage, StageDrop) and the counter read-back; the sizing of a launch (MapSteal, the
// tail and long-token regions), its rerun when a capacity was exceeded, and the two maps -- job_map, the LDS-combine
// map, which hands its output to an aggregation, and job_map_wide, which writes every key to its L1 bucket and
// goes on with the leaves of the wide aggregation.
// Calls: mrg_agg.cpp -- agg_ocap and agg_launch (the aggregation queued right behind the map), bucket_aggregate,
// wide_aggregate, wide_finish with WideL1 and PhaseClock (the wide map is an L1 of its own), part_key_plan.
// Called by: mrgpu.cpp (job_begin, mrg_job_map), mrg_agg.cpp (job_map_add), mrg_plugin.cpp, mrg_run.cpp; the
// staging beyond flush_stage and read_counters is the map's alone, so it is not declared in mrg_host.h.
#include <exception>

#include "mrg_host.h"

using namespace mrg_host;

namespace {

// MRG_WIDE=<non-zero>: force the wide (sort-based) aggregation; MRG_WIDE=0 pins the bucket path
bool wide_forced() {
    const char *v = getenv("MRG_WIDE");
    return v && *v && atoi(v) != 0;
}
// MRG_WIDE=0 pins the bucket path, so it also rules out the wide map
bool wide_forced_off() {
    const char *v = getenv("MRG_WIDE");
    return v && *v && atoi(v) == 0;
}

// Host -> device copy of a small table through the pinned staging region (falls back to a pageable
// copy when the region is used up).  Valid only between job_begin and the job's next host wait.
void h2d(mrg_ctx *c, void *dst, const void *src, size_t n) {
    if (!n) return;
    if (c->h_stage && c->stage_used + n <= MRG_STAGE_BYTES) {
        uint8_t *p = c->h_stage + c->stage_used;
        memcpy(p, src, n);
        c->stage_used += (n + 63) & ~(size_t)63;
        HIPCHK(hipMemcpyAsync(dst, p, n, hipMemcpyHostToDevice, c->stream));
    } else {
        HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream));
    }
}

// Batched small writes of a job's setup (r06): data staged in the pinned buffer like h2d's, the writes
// recorded, and issued together by flush_stage -- one copy of the staged range (ops table included)
// and one k_stage_scatter launch instead of a copy or memset each (C3 map setup: 12 -> 2 stream ops).
// Every kernel that reads a staged destination must be launched after a flush_stage.
constexpr size_t MRG_STAGE_OPS = 256;   // ops per batch
constexpr uint32_t MRG_STAGE_MAX = 16384;  // larger writes go through their own copy / memset

bool stage_room(mrg_ctx *c, size_t n) {
    if (!c->h_stage || !c->d_stage || n > MRG_STAGE_MAX) return false;
    if (c->pend.size() >= MRG_STAGE_OPS ||
        c->stage_used + n + 64 + sizeof(StageOp) * (MRG_STAGE_OPS + 1) > MRG_STAGE_BYTES) {
        flush_stage(c);
        if (c->stage_used + n + 64 + sizeof(StageOp) * (MRG_STAGE_OPS + 1) > MRG_STAGE_BYTES) return false;
    }
    return true;
}
void stage_h2d(mrg_ctx *c, void *dst, const void *src, size_t n) {
    if (!n) return;
    if (!stage_room(c, n)) {
        flush_stage(c);  // (issue order kept)
        h2d(c, dst, src, n);
        return;
    }
    if (c->pend.empty()) c->pend_lo = c->stage_used;
    memcpy(c->h_stage + c->stage_used, src, n);
    c->pend.push_back(StageOp{(uint64_t)(uintptr_t)dst, (uint32_t)c->stage_used, (uint32_t)n, 0u, 0u});
    c->stage_used += (n + 63) & ~(size_t)63;
}
void stage_fill(mrg_ctx *c, void *dst, int byte, size_t n) {
    if (!n) return;
    if (!stage_room(c, 0) || n > MRG_STAGE_MAX) {
        flush_stage(c);
        HIPCHK(hipMemsetAsync(dst, byte, n, c->stream));
        return;
    }
    if (c->pend.empty()) c->pend_lo = c->stage_used;
    c->pend.push_back(StageOp{(uint64_t)(uintptr_t)dst, 0xFFFFFFFFu, (uint32_t)n, (uint32_t)(byte & 0xFF), 0u});
}

// Drops the staged writes (stage_h2d / stage_fill) that are still pending when its scope ends by an
// exception: their destinations are scratch blocks the same exit returns to the pool, and the next
// flush_stage -- the next job's, at the latest -- would write them into memory that another call owns
// by then.  The staging bytes they used had no copy issued, so the bump pointer goes back over them.
struct StageDrop {
    mrg_ctx *c;
    int live = std::uncaught_exceptions();
    explicit StageDrop(mrg_ctx *ctx) : c(ctx) {}
    StageDrop(const StageDrop &) = delete;
    StageDrop &operator=(const StageDrop &) = delete;
    ~StageDrop() {
        if (std::uncaught_exceptions() == live || c->pend.empty()) return;
        c->pend.clear();
        c->stage_used = c->pend_lo;
    }
};

// ---- the wide map (near-unique keys, wc): the splitters first, from a sample of the input text, then
// a map that writes every short key to its L1 bucket (R partitions x B1r key ranges) -- the L1 count
// and scatter passes over the map's records (wide_aggregate) disappear; L2 reads the regions.
struct WideMapPlan {
    bool on = false, forced = false, w12 = false;
    bool repeats = false;     // a cold context's sample found repeats: the bucket path is the likely one
    uint64_t n16 = 0, S = 0;  // sampled keys of 13..16 bytes, samples
    uint32_t B1 = 0, B1r = 0;
    uint64_t *spl1 = nullptr;
    uint8_t *ix1 = nullptr;
};

// Sampled (k_wsample_text + k_wsample_dups, ~0.1 ms and one host wait) on every wc job of >= 64 MiB
// whose context has no measured path yet -- the first job of a fresh context, so every mrg_run_job and
// every one-shot worker call -- and when the context's last such job went the wide way (or
// MRG_WIDE_MAP=1).  Taken when the sample is near-unique: fewer than 1 in 16 sampled tokens repeat a
// sampled neighbour in key order.  (Until r05 only the hint sampled: a cold near-unique job ran the
// LDS-combine map, overflowed its tail regions, reran it and took the L1 count + scatter passes.)
// The splitters (and their index) of a plan that is on are blocks of `keep`.
WideMapPlan wide_map_plan(mrg_ctx *c, Scratch &keep, const uint64_t *d_doc_off, uint32_t nd, uint64_t total, int grid) {
    WideMapPlan P;
    const char *env = getenv("MRG_WIDE_MAP");
    P.forced = env && atoi(env) != 0;
    if (is_idx(c) || (env && atoi(env) == 0) || total == 0 || wide_forced_off()) return P;
    if (!P.forced && (total < (64ull << 20) || (c->wc_sized && !c->wide_hint))) return P;
    const uint32_t R = c->R;
    if (R > MRG_WMAP_MAXB1 || grid > 512) return P;
    uint32_t B1r = std::min<uint32_t>(64, std::max<uint32_t>(1, MRG_WMAP_MAXB1 / R));
    if (const uint64_t t = env_u64("MRG_TEST_WMAP_B1R", 0)) B1r = (uint32_t)std::min<uint64_t>(B1r, t);
    const uint32_t B1 = R * B1r;
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint32_t S = (uint32_t)std::min<uint64_t>(64ull * B1, 1u << 20);
    flush_stage(c);  // the document tables, read by the sampling kernels
    if (!P.forced && !c->wide_hint) {  // no hint (a cold context): the one-launch test on 8192 samples first
        Scratch t(c->pool);
        const uint32_t S0 = std::min<uint32_t>(S, 8192);
        SortRec *s0 = t.get<SortRec>(S0);
        unsigned long long *d0 = t.get<unsigned long long>(2);
        mrg_wide_launch_sample_text(c->d_in, d_doc_off, nd, total, S0, R, s0, s);
        mrg_wide_launch_sample_uniq(s0, S0, d0, s);
        unsigned long long *h0 = &c->h_cnt[CNT_N];  // pinned scratch
        HIPCHK(hipMemcpyAsync(h0, d0, 16, hipMemcpyDeviceToHost, s));
        sync(c);
        if (h0[0] * 16 >= S0) {  // repeats: the LDS combine pays
            P.repeats = true;
            return P;
        }
    }
    SortRec *sa = sc.get<SortRec>(S), *sb = sc.get<SortRec>(S);
    void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(S));
    unsigned long long *dups = sc.get<unsigned long long>(2);
    HIPCHK(hipMemsetAsync(dups, 0, 16, s));
    mrg_wide_launch_sample_text(c->d_in, d_doc_off, nd, total, S, R, sa, s);
    int passes = 0;
    SortRec *srt = mrg_radix_sort(sa, sb, S, part_key_plan(R), stmp, s, &passes);
    mrg_wide_launch_sample_dups(srt, S, dups, s);
    uint64_t *spl1 = sc.get<uint64_t>(2ull * R * B1r + 2);
    uint8_t *ix1 = nullptr;
    if (B1r > 1) {
        mrg_wide_launch_split1(srt, S, R, B1r, spl1, s);
        if (B1r >= 5 && R <= MRG_WMAP_IXR) {
            ix1 = sc.get<uint8_t>((uint64_t)MRG_WIDE_IX1 * R);
            mrg_wide_launch_l1ix(spl1, R, B1r, ix1, s);
        }
    }
    unsigned long long dh[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(dh, dups, 16, hipMemcpyDeviceToHost, s));
    sync(c);
    if (!P.forced && dh[0] * 16 >= S) {  // repeats: the LDS combine pays
        c->wide_hint = false;
        return P;
    }
    P.on = true;
    // 12-byte regions when keys of 13..16 bytes are rare (under 1 in 256 sampled tokens): those go to
    // per-bucket lists of 16-byte records (MRG_TEST_WMAP_W12=0/1 overrides)
    P.n16 = dh[1];
    P.S = S;
    P.w12 = !c->w12_off && dh[1] * 256 < S;
    if (const char *e = getenv("MRG_TEST_WMAP_W12")) P.w12 = atoi(e) != 0;
    P.B1 = B1;
    P.B1r = B1r;
    P.spl1 = keep.adopt(sc.release(spl1));
    P.ix1 = keep.adopt(sc.release(ix1));
    return P;
}

// Load balance of a map launch: the last 1/16 of the blocks form a pool that a
// workgroup's waves take from once its equal share of the rest is done, at most steal_max blocks per
// workgroup -- so a workgroup maps at most per_wg_blocks blocks, and its per-workgroup capacities (tail
// and long-token regions, wide-map regions, the non-ASCII tile list) are sized for that (wg_scale x an
// equal share).  MRG_MAP_STEAL=0, or a small input: equal shares of every block, as before r06.
struct MapSteal {
    uint64_t n_static = 0;     // blocks in equal shares
    uint32_t steal_max = 0;    // pool blocks one workgroup may take
    uint32_t run = 1;          // blocks of its share a wave claims at a time (MRG_MAP_RUN)
    uint64_t per_wg_blocks = 0;
    double wg_scale = 1.0;
};
MapSteal map_steal(uint64_t n_chunks, int grid) {
    MapSteal m;
    const uint64_t g = (uint64_t)std::max(grid, 1);
    // runs of MRG_MAP_RUN blocks where every wave of a workgroup still gets four of them; a smaller share in
    // shorter runs, down to single blocks (a 4 MB job has 8 blocks per workgroup: runs of 4 would leave 14 of
    // its 16 waves idle).  MRG_MAP_RUN in the environment is taken as it stands.
    const uint64_t share = n_chunks / g;
    m.run = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(MRG_MAP_RUN, share / (4 * MRG_MAP_WAVES)), 1);
    if (getenv("MRG_MAP_RUN")) m.run = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(env_u64("MRG_MAP_RUN", 1), 1), 64);
    const uint64_t div = env_u64("MRG_MAP_STEAL", 16);  // the pool is 1/div of the blocks (0: no pool)
    const uint64_t pool = div ? n_chunks / div : 0;
    if (pool == 0 || pool < env_u64("MRG_TEST_STEAL_MIN", 64 * g)) {  // nothing worth balancing (tests: any pool)
        m.n_static = n_chunks;
        m.per_wg_blocks = (n_chunks + g - 1) / g + 1;
        return m;
    }
    m.n_static = n_chunks - pool;
    m.steal_max = (uint32_t)(2 * pool / g + 1024);
    // share + budget + one claim (the kernel refuses a claim that would pass the budget: the last term is slack)
    m.per_wg_blocks = (m.n_static + g - 1) / g + 1 + m.steal_max + std::max<uint64_t>(m.run, MRG_MAP_STEAL_K);
    m.wg_scale = (double)m.per_wg_blocks / ((double)n_chunks / (double)g);
    return m;
}

// The packed tail cursors (k_map.hip TailRegions: record index and region end in one 64-bit word) are
// valid while no index can carry into its end.  A region's index starts below rtot and grows by one
// per append, past a full region too; a workgroup appends at most one record per token it maps, and a
// block holds at most BLK / 2 token starts.  So every index of the launch stays below the left side.
inline bool map_tail_packed(uint64_t rtot, uint64_t rtot16, const MapSteal &ms) {
    const uint64_t appends = ms.per_wg_blocks * (uint64_t)(MRG_MAP_NSUB * MRG_MAP_TILE) / 2 + 1;
    return rtot + appends < (1ull << 32) && rtot16 + appends < (1ull << 32);
}

// ---- what the LDS-combine map (job_map) and the wide map (job_map_wide) share.  The device blocks of
// one launch belong to a Scratch of the attempt (`att`), which a rerun returns before it takes its own.

// The input of a map: the document, block and id tables on the device, the grid, the documents' ids.
struct MapIn {
    const uint64_t *doc_off = nullptr, *chunk_base = nullptr;
    const uint32_t *doc_id = nullptr;
    uint32_t nd = 0;
    uint64_t n_chunks = 0, total = 0;
    int grid = 0;
    std::vector<uint32_t> ids;
};

// the steal plan into a launch's arguments, with its pool counters (zeroed by a staged write)
void set_steal(mrg_ctx *c, Scratch &att, MapArgs &A, const MapSteal &ms, uint64_t n_chunks) {
    if (n_chunks * MRG_MAP_NSUB >= 0xFFFFFFFFull) raise(MRG_ENOMEM, "input too large for one map launch");
    A.n_static = ms.n_static;
    A.steal_max = ms.steal_max;
    A.run = ms.run;
    A.pool_ctr = nullptr;
    if (ms.n_static < n_chunks) {
        A.pool_ctr = att.get<unsigned long long>(8 * 16);
        stage_fill(c, A.pool_ctr, 0, 8ull * 8 * 16);
    }
}

// The arguments both maps' launches have: the input, the counters, the long-token regions (one of lper
// records per workgroup + a shared list of lovf), the non-ASCII tile lists (one entry per tile of a
// workgroup's share and steal budget at most) and the steal plan.  Returns the long-token slots.
// knobs: MRG_TEST_LONG_PER / MRG_TEST_LONG_LIST apply (the LDS-combine map's first launch only: a
// rerun grows the regions from the measured demand).  attempt: the launches of this map so far; a tile
// list is sized for every tile its workgroup can map, and a rerun (whatever overflowed) lengthens it
// (MRG_TEST_KWORDS: the first launch's list capacity, to reach that path).
uint64_t map_args_shared(mrg_ctx *c, Scratch &att, MapArgs &A, const MapIn &in, const MapSteal &ms, uint64_t lcap,
                         bool knobs, uint32_t attempt) {
    A.in = c->d_in;
    A.doc_off = in.doc_off;
    A.chunk_base = in.chunk_base;
    A.doc_id = in.doc_id;
    A.n_docs = in.nd;
    A.n_chunks = in.n_chunks;
    A.counters = c->d_cnt;
    A.hash_bits = hash_bits(c);
    uint64_t lper = std::max<uint64_t>(c->lper_hint, (uint64_t)(ms.wg_scale * (double)((lcap + in.grid - 1) / in.grid)) + 16);
    uint64_t lovf = lcap / 4 + 1024;
    if (knobs) {
        if (const uint64_t t = env_u64("MRG_TEST_LONG_PER", 0)) lper = t;
        if (const uint64_t t = env_u64("MRG_TEST_LONG_LIST", 0)) lovf = t;
    }
    if (lper > 0xFFFFFFF0ull) raise(MRG_ENOMEM, "input too large for one map launch");
    const uint64_t lslots = (uint64_t)in.grid * lper + lovf;
    A.lstart = att.get<uint64_t>(lslots);
    A.llen = att.get<uint32_t>(lslots);
    A.ldoc = att.get<uint32_t>(lslots);
    A.lcount = att.get<uint32_t>((uint64_t)in.grid);
    A.lper = (uint32_t)lper;
    A.lovf = lovf;
    uint64_t kwords = MRG_MAP_NSUB * ms.per_wg_blocks * (1 + (uint64_t)std::min(attempt, 7u));
    if (attempt == 0) kwords = env_u64("MRG_TEST_KWORDS", kwords);
    if (kwords > 0xFFFFFFF0ull) raise(MRG_ENOMEM, "input too large for one map launch");
    A.kwords = (uint32_t)kwords;
    A.gbits = att.get<uint32_t>((uint64_t)in.grid * A.kwords);
    set_steal(c, att, A, ms, in.n_chunks);
    return lslots;
}

// A workgroup's long tokens overflowed its region and the shared list: grow both (remembered).
void grow_long_regions(mrg_ctx *c, const MapArgs &A, int grid, uint64_t &lcap) {
    std::vector<uint32_t> lc((uint64_t)grid);
    HIPCHK(hipMemcpyAsync(lc.data(), A.lcount, 4ull * grid, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    const uint64_t mx = *std::max_element(lc.begin(), lc.end());
    const uint64_t nl = c->h_cnt[CNT_LONG];
    c->lper_hint = mx + mx / 4 + 64;
    lcap = c->long_hint = std::max<uint64_t>(lcap, nl + nl / 8 + 1024);
}

// mrg_stats of a finished map, from its counters
void map_stats(mrg_ctx *c, uint32_t launches, uint64_t total) {
    c->st.ms_map = ev_ms(c, c->ev, 0, 1);
    c->st.map_launches = launches;
    c->st.input_bytes = total;
    c->st.tokens = c->h_cnt[CNT_TOKENS];
    c->st.long_tokens = c->h_cnt[CNT_LONG];
    c->st.map_records = c->h_cnt[CNT_REC];
    c->st.nonascii_tiles = c->h_cnt[CNT_NONASCII];
}

// The map found invalid UTF-8 (the reference's read_to_string panic): raise it with the document.
void check_map_utf8(mrg_ctx *c, const std::vector<uint32_t> &ids) {
    const uint64_t errpos = c->h_cnt[CNT_ERRPOS];
    if (errpos == ~0ull) return;
    const uint32_t nd = (uint32_t)ids.size();
    uint32_t d = 0;
    while (d + 1 < nd && c->doc_off[d + 1] <= errpos) ++d;
    const char *nm = ids[d] < c->names.size() ? c->names[ids[d]].c_str() : "";
    raise(MRG_EUTF8, "stream did not contain valid UTF-8: document %u (id %u%s%s), byte offset %llu", d, ids[d],
          *nm ? ", " : "", nm, (unsigned long long)(errpos - c->doc_off[d]));
}

// The map's long tokens: the workgroups' regions and the shared list packed densely (blocks of sc).
LongItems long_items(mrg_ctx *c, Scratch &sc, const MapArgs &A, int grid) {
    LongItems li{};
    li.base = c->d_in;
    li.cnt = nullptr;
    li.n = c->h_cnt[CNT_LONG];
    if (li.n) {
        uint64_t *dstart = sc.get<uint64_t>(li.n);
        uint32_t *dlen = sc.get<uint32_t>(li.n), *ddoc = sc.get<uint32_t>(li.n);
        mrg_launch_long_compact(A, grid, dstart, dlen, ddoc, c->stream);
        li.start = dstart; li.rawlen = dlen; li.doc = ddoc;
    }
    return li;
}

// (sc: the blocks of the whole call, with the input tables and the plan's splitters)
void job_map_wide(mrg_ctx *c, Scratch &sc, const WideMapPlan &wp, const MapIn &in) {
    hipStream_t s = c->stream;
    const uint32_t B1 = wp.B1;
    const int grid = in.grid;
    const uint64_t total = in.total, n_chunks = in.n_chunks;
    // records per (bucket, workgroup) region: the splitters make the buckets about equal; a token per
    // ~10 input bytes, +30 %, or the last run's demand
    const MapSteal ms = map_steal(n_chunks, grid);
    uint64_t wcap = std::max<uint64_t>(c->wcap_hint,
                                       (uint64_t)(1.3 * ms.wg_scale * (double)total / 10.0 / (double)grid / (double)B1) + 64);
    if (const uint64_t t = env_u64("MRG_TEST_WMAP_CAP", 0)) wcap = t;
    uint64_t lcap = std::max<uint64_t>(c->long_hint, total / 1024 + 1024);
    MapArgs A{};
    Scratch att(c->pool);
    uint32_t launches = 0;
    bool w12 = wp.w12;
    // the 16-byte lists of 12-byte regions: four times the sampled share of such keys, at least 2 K each
    uint64_t wl16cap = std::max<uint64_t>(2048, (uint64_t)(4.0 * (double)total / 10.0 / (double)B1 *
                                                            (double)(wp.n16 + 1) / (double)std::max<uint64_t>(wp.S, 1)));
    if (const uint64_t t = env_u64("MRG_TEST_WMAP_L16", 0)) wl16cap = t;
    for (;;) {
        if (wcap > 0xFFFFFFF0ull) raise(MRG_ENOMEM, "input too large for one map launch");
        MapArgs *dargs = att.get<MapArgs>(1);
        A = MapArgs{};
        map_args_shared(c, att, A, in, ms, lcap, false, launches);
        const uint64_t nslots = (uint64_t)B1 * grid * wcap;
        A.wrec = att.get<uint64_t>(w12 ? (12 * nslots + 16 + 7) / 8 : 2 * nslots + 2);
        A.wcnt = att.get<uint32_t>((uint64_t)B1 * grid);
        if (w12) {
            if (wl16cap > 0xFFFFFFF0ull) raise(MRG_ENOMEM, "input too large for one map launch");
            A.wl16 = att.get<uint64_t>(2ull * B1 * wl16cap + 2);
            A.wl16n = att.get<uint32_t>(B1);
            HIPCHK(hipMemsetAsync(A.wl16n, 0, 4ull * B1, s));
        }
        A.wspl = wp.spl1; A.wix = wp.ix1;
        A.wR = c->R; A.wB1r = wp.B1r; A.wcap = (uint32_t)wcap;
        A.w12 = w12 ? 1u : 0u; A.wl16cap = (uint32_t)wl16cap;
        // the kernel's LDS cursors, splitters and index rows are sized by these bounds (k_map.hip)
        if (A.wB1r == 0 || (uint64_t)A.wR * A.wB1r > MRG_WMAP_MAXB1 || (A.wix && A.wR > MRG_WMAP_IXR))
            raise(MRG_EINVAL, "wide map plan exceeds the kernel's LDS bounds");
        HIPCHK(hipMemsetAsync(c->d_cnt, 0, sizeof(unsigned long long) * CNT_N, s));
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_ERRPOS], 0xFF, sizeof(unsigned long long), s));
        flush_stage(c);  // (set_steal's pool counters)
        ev_rec(c, c->ev, 0);
        h2d(c, dargs, &A, sizeof(MapArgs));
        mrg_launch_map(nullptr, dargs, c->app, grid, c->lds_cap, s, true);
        ev_rec(c, c->ev, 1);
        HIPCHK(hipGetLastError());
        ++launches;
        read_counters(c);
        const bool long_full = c->h_cnt[CNT_LONGX] > A.lovf;
        const bool l16_full = c->h_cnt[CNT_W16] != 0;
        if (c->h_cnt[CNT_OVF] == 0 && !long_full && !l16_full) break;
        if (l16_full) {  // too many keys of 13..16 bytes for the lists: 16-byte regions from now on
            w12 = false;
            c->w12_off = true;
        }
        if (c->h_cnt[CNT_OVF]) {  // a region overflowed: every region sized to the largest demand
            std::vector<uint32_t> wc((uint64_t)B1 * grid);
            HIPCHK(hipMemcpyAsync(wc.data(), A.wcnt, 4ull * wc.size(), hipMemcpyDeviceToHost, s));
            sync(c);
            const uint64_t mx = *std::max_element(wc.begin(), wc.end());
            wcap = c->wcap_hint = std::max<uint64_t>(wcap, mx + mx / 4 + 64);
        }
        if (long_full) grow_long_regions(c, A, grid, lcap);
        if (getenv("MRG_DEBUG"))
            fprintf(stderr, "[mrgpu] wide map rerun: region overflow %llu (cap now %llu), long %llu\n",
                    (unsigned long long)c->h_cnt[CNT_OVF], (unsigned long long)wcap,
                    (unsigned long long)c->h_cnt[CNT_LONG]);
        att.put_all();
    }
    map_stats(c, launches, total);
    c->st.tail_records_16 = 0;
    c->st.map_spill = 0;
    check_map_utf8(c, in.ids);
    ev_rec(c, c->ev, 2);
    const LongItems li = long_items(c, att, A, grid);
    // ---- the regions as L1 buckets: per-bucket segment starts, bucket offsets, then L2 and the leaves
    PhaseClock clock(s);
    clock.mark("start");
    Scratch fin(c->pool);  // what wide_finish takes over
    uint32_t *soff = att.get<uint32_t>((uint64_t)B1 * (grid + 2));
    uint64_t *nbk = att.get<uint64_t>((uint64_t)B1 + 1);
    uint64_t *bstart = fin.get<uint64_t>((uint64_t)B1 + 1);
    uint64_t *tmp = att.get<uint64_t>(mrg_scan_tmp_elems((uint64_t)B1 + 1));
    HIPCHK(hipMemsetAsync(nbk + B1, 0, 8, s));
    mrg_wmap_launch_seg(A.wcnt, B1, (uint32_t)grid, (uint32_t)wcap, A.wl16n, (uint32_t)wl16cap, soff, nbk, s);
    mrg_scan_u64(nbk, bstart, (uint64_t)B1 + 1, tmp, s);  // bstart[B1] = records
    uint64_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, bstart + B1, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    if (n >= 0xFFFFFFF0ull) raise(MRG_ENOMEM, "wide aggregation: %llu records exceed one GPU's 32-bit record index",
                                  (unsigned long long)n);
    WideL1 l1;
    l1.n = n; l1.B1 = B1; l1.B1r = wp.B1r;
    l1.bstart = bstart;
    l1.K1 = fin.get<uint64_t>(2 * n + 2);  // the leaves' output keys
    l1.bid = fin.get<uint16_t>(std::max<uint64_t>(n, 1));
    l1.wk0 = fin.get<uint64_t>(1); l1.wk1 = fin.get<uint64_t>(1); l1.wcnt = fin.get<uint64_t>(1);  // (no weighted keys)
    l1.wpart = fin.get<uint32_t>(1);
    l1.spl1 = fin.adopt(sc.release(wp.spl1));
    c->st.agg_path = 2;
    c->spec_agg = false;
    WmapIn &wm = l1.wm;
    wm.rin = A.wrec; wm.soff = soff; wm.grid = (uint32_t)grid; wm.wcap = (uint32_t)wcap;
    wm.w12 = w12 ? 1u : 0u; wm.wl16cap = (uint32_t)wl16cap; wm.wl16 = A.wl16;
    clock.mark("segments");
    wide_finish(c, fin, l1, li, clock);
    c->st.map_kind = 1;
    ev_rec(c, c->ev, 3);
    c->st.ms_aggregate = ev_ms(c, c->ev, 2, 3);
    // the hint holds while the input stays near-unique
    c->wide_hint = 2 * c->st.distinct_keys > c->st.tokens;
    c->wc_sized = true;
    c->mapped = c->keyed = true;
}

// MRG_PROF: the map kernel's phase clocks, and (builds with -DMRG_MAP_PROF) the workgroups' wall clocks
void map_prof_report(const MapArgs &A, int grid) {
    unsigned long long pr[8];
    HIPCHK(hipMemcpy(pr, A.prof, sizeof pr, hipMemcpyDeviceToHost));
    double tot = 0;
    for (int i = 0; i < 7; ++i) tot += (double)pr[i];
    static const char *nm[7] = {"load-wait", "classify", "stage+scan+queue", "token rounds", "slow tokens",
                                "non-ascii", "flush"};
    fprintf(stderr, "[mrgpu] map phase clocks (sum over waves %.3e):", tot);
    for (int i = 0; i < 7; ++i) fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * (double)pr[i] / (tot > 0 ? tot : 1));
    fprintf(stderr, "\n");
    // workgroup start/end wall clocks (100 MHz; written by -DMRG_MAP_PROF builds only)
    std::vector<unsigned long long> wt(8ull * grid);
    HIPCHK(hipMemcpy(wt.data(), A.prof + 8, 8ull * wt.size(), hipMemcpyDeviceToHost));
    if (wt[1]) {
        unsigned long long t0 = ~0ull, t1 = 0, ls = 0;
        std::vector<double> dur(grid), end(grid), lend(grid);
        std::vector<std::vector<double>> fst(5, std::vector<double>(grid, 0.0));
        for (int g = 0; g < grid; ++g) t0 = std::min(t0, wt[8 * g]);
        for (int g = 0; g < grid; ++g) {
            const unsigned long long *w = &wt[8ull * g];
            t1 = std::max(t1, w[1]);
            ls = std::max(ls, w[0]);
            dur[g] = (double)(w[1] - w[0]) * 1e-5;
            end[g] = (double)(w[1] - t0) * 1e-5;
            lend[g] = w[2] ? (double)(w[2] - t0) * 1e-5 : 0.0;
            unsigned long long prev = w[2];
            for (int k = 0; k < 5; ++k)
                if (w[3 + k] && prev) {
                    fst[k][g] = (double)(w[3 + k] - prev) * 1e-5;
                    prev = w[3 + k];
                }
        }
        std::sort(dur.begin(), dur.end());
        std::sort(end.begin(), end.end());
        std::sort(lend.begin(), lend.end());
        fprintf(stderr, "[mrgpu] map workgroups (ms): span %.3f, end min %.3f med %.3f max %.3f, "
                "main loop end min %.3f med %.3f max %.3f, duration min %.3f med %.3f max %.3f, "
                "last start %.3f\n", (double)(t1 - t0) * 1e-5, end[0], end[grid / 2], end[grid - 1],
                lend[0], lend[grid / 2], lend[grid - 1], dur[0], dur[grid / 2], dur[grid - 1],
                (double)(ls - t0) * 1e-5);
        fprintf(stderr, "[mrgpu] map flush steps (ms, median / max over workgroups):");
        static const char *fn[5] = {"counts", "histogram", "scan", "entries", "totals"};
        for (int k = 0; k < 5; ++k) {
            std::sort(fst[k].begin(), fst[k].end());
            fprintf(stderr, " %s %.4f / %.4f", fn[k], fst[k][grid / 2], fst[k][grid - 1]);
        }
        fprintf(stderr, "\n");
    }
}

}  // namespace

namespace mrg_host __attribute__((visibility("hidden"))) {

// issues the batch of staged writes (stage_h2d / stage_fill above): one copy and one k_stage_scatter launch
void flush_stage(mrg_ctx *c) {
    if (c->pend.empty()) return;
    const size_t t = (c->stage_used + 63) & ~(size_t)63;  // the ops table after the staged data
    const size_t tb = sizeof(StageOp) * c->pend.size();
    memcpy(c->h_stage + t, c->pend.data(), tb);
    HIPCHK(hipMemcpyAsync(c->d_stage + c->pend_lo, c->h_stage + c->pend_lo, t + tb - c->pend_lo, hipMemcpyHostToDevice,
                          c->stream));
    mrg_launch_stage_scatter(c->d_stage, (uint32_t)t, (uint32_t)c->pend.size(), c->stream);
    HIPCHK(hipGetLastError());
    c->stage_used = c->pend_lo = (t + tb + 63) & ~(size_t)63;
    c->pend.clear();
}

void read_counters(mrg_ctx *c) {
    HIPCHK(hipMemcpyAsync(c->h_cnt, c->d_cnt, sizeof(unsigned long long) * CNT_N, hipMemcpyDeviceToHost, c->stream));
    sync(c);
}

void job_map(mrg_ctx *c) {
    need_job(c);
    if (c->doc_off.empty()) raise(MRG_EINVAL, "no input: call mrg_job_set_input first");
    c->wide.release(c->pool);  // a second map of the same job replaces the first one's keys
    c->mapped = c->reduced = c->keyed = false;
    c->st.spec_agg = c->st.agg_path = c->st.map_kind = 0;
    Scratch sc(c->pool);  // the blocks of the whole call
    StageDrop undo(c);    // (an error exit returns blocks that staged writes still point at)
    hipStream_t s = c->stream;
    const uint32_t nd = (uint32_t)c->doc_off.size() - 1;
    const uint64_t total = c->doc_off[nd] - c->doc_off[0];
    std::vector<uint64_t> cb(nd + 1, 0);
    for (uint32_t d = 0; d < nd; ++d) cb[d + 1] = cb[d] + mrg_map_tiles(c->doc_off[d], c->doc_off[d + 1]);
    const uint64_t n_chunks = cb[nd];
    MapIn in;
    in.ids = c->doc_ids;
    if (in.ids.empty()) for (uint32_t d = 0; d < nd; ++d) in.ids.push_back(d);

    uint64_t *d_doc_off = sc.get<uint64_t>(nd + 1), *d_cb = sc.get<uint64_t>(nd + 1);
    uint32_t *d_ids = sc.get<uint32_t>(nd);
    stage_h2d(c, d_doc_off, c->doc_off.data(), 8ull * (nd + 1));
    stage_h2d(c, d_cb, cb.data(), 8ull * (nd + 1));
    stage_h2d(c, d_ids, in.ids.data(), 4ull * nd);

    if (!c->map_grid) c->map_grid = mrg_map_max_grid(c->app, c->lds_cap, c->device);
    // (MRG_TEST_MAP_GRID: more workgroups than fit at once, run in waves: an A/B knob for load balance)
    const uint64_t grid_want = env_u64("MRG_TEST_MAP_GRID", (uint64_t)c->map_grid);
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(grid_want, n_chunks));
    in.doc_off = d_doc_off; in.chunk_base = d_cb; in.doc_id = d_ids;
    in.nd = nd; in.n_chunks = n_chunks; in.total = total; in.grid = grid;
    bool cold_repeats = false;  // a cold context whose sample found repeats: queue the aggregation too
    {  // near-unique input: the wide map (every key straight to its L1 bucket)
        const WideMapPlan wp = wide_map_plan(c, sc, d_doc_off, nd, total, grid);
        if (wp.on) {
            job_map_wide(c, sc, wp, in);
            return;
        }
        cold_repeats = wp.repeats;
    }
    const uint32_t cap = (uint32_t)mrg_map_cap(c->app, c->lds_cap);
    const bool idx = is_idx(c);
    const uint32_t RW = idx ? 3u : 2u;
    uint64_t lcap = std::max<uint64_t>(c->long_hint, total / 1024 + 1024);
    // records per (bucket, workgroup) tail region: ~1 in 20 input bytes is a tail record (combine
    // misses), spread evenly over the buckets; grown per bucket to the measured demand on a rerun
    const MapSteal ms = map_steal(n_chunks, grid);
    const double per_wg = (double)std::max<uint64_t>(total, 1) / grid * ms.wg_scale;
    // wc keys of 13..16 bytes (rare in text) get regions of 16-byte records a sixteenth that size
    std::vector<uint64_t> bcap(MRG_NBUCKET), bcap16(MRG_NBUCKET, 0);
    for (int b = 0; b < MRG_NBUCKET; ++b) {
        double est = per_wg / 20.0 / MRG_NBUCKET;
        if (c->bcap_rate.size() == MRG_NBUCKET) est = std::max(est, c->bcap_rate[b] * per_wg);
        bcap[b] = (uint64_t)(est * 1.25) + 32;
        if (!idx) {
            double est16 = per_wg / 20.0 / MRG_NBUCKET / 16.0;
            if (c->bcap16_rate.size() == MRG_NBUCKET) est16 = std::max(est16, c->bcap16_rate[b] * per_wg);
            bcap16[b] = (uint64_t)(est16 * 1.25) + 16;
        }
    }
    // per-bucket overflow lists absorb the run-to-run variation of the regions' demand (the LDS
    // table's contents depend on wave timing: a frequent key that finds its set full in one
    // workgroup sends all its tokens to one region), so a launch is repeated only when one fills
    // up.  Sized at a quarter of the default region total per bucket (C3: 2 GiB, only touched as
    // far as used); at 1/16 about one step in ten reran the whole map.
    uint64_t ocap = std::max<uint64_t>(c->ocap_hint, std::max<uint64_t>(1024, total / 20 / MRG_NBUCKET / 4));
    if (const uint64_t t = env_u64("MRG_TEST_TAIL_CAP", 0)) {  // test knobs
        bcap.assign(MRG_NBUCKET, t);
        if (!idx) bcap16.assign(MRG_NBUCKET, t);
    }
    if (const uint64_t t = env_u64("MRG_TEST_OVF_CAP", 0)) ocap = t;
    MapArgs A{};
    Scratch att(c->pool);
    AggLaunch spec(c->pool);  // the aggregation launched right behind the map (wc, the last job took the bucket path)
    uint32_t launches = 0;
    for (;;) {
        std::vector<uint64_t> rbase(MRG_NBUCKET, 0), rbase16(MRG_NBUCKET, 0);
        std::vector<uint32_t> bcap32(MRG_NBUCKET), bcap16_32(MRG_NBUCKET);
        uint64_t rtot = 0, rtot16 = 0;
        for (int b = 0; b < MRG_NBUCKET; ++b) {
            if (bcap[b] > 0xFFFFFFF0ull || bcap16[b] > 0xFFFFFFF0ull)
                raise(MRG_ENOMEM, "input too large for one map launch");
            bcap32[b] = (uint32_t)bcap[b];
            rbase[b] = rtot;
            rtot += (uint64_t)grid * bcap[b];
            bcap16_32[b] = (uint32_t)bcap16[b];
            rbase16[b] = rtot16;
            rtot16 += (uint64_t)grid * bcap16[b];
        }
        uint64_t *d_rbase = att.get<uint64_t>(MRG_NBUCKET);
        uint32_t *d_bcap = att.get<uint32_t>(MRG_NBUCKET);
        A.bcount = att.get<uint32_t>((uint64_t)grid * MRG_NBUCKET);
        uint64_t *d_rbase16 = att.get<uint64_t>(MRG_NBUCKET);
        uint32_t *d_bcap16 = att.get<uint32_t>(MRG_NBUCKET);
        A.bcount16 = att.get<uint32_t>((uint64_t)grid * MRG_NBUCKET);
        MapArgs *dargs = att.get<MapArgs>(1);
        if (ocap > 0xFFFFFFF0ull) raise(MRG_ENOMEM, "input too large for one map launch");
        A.ovf = att.get<uint64_t>((uint64_t)MRG_NBUCKET * ocap * RW);
        A.onext = att.get<uint32_t>(MRG_NBUCKET);
        A.ocap = (uint32_t)ocap;
        stage_fill(c, A.onext, 0, 4ull * MRG_NBUCKET);
        stage_h2d(c, d_rbase, rbase.data(), 8ull * MRG_NBUCKET);
        stage_h2d(c, d_bcap, bcap32.data(), 4ull * MRG_NBUCKET);
        stage_h2d(c, d_rbase16, rbase16.data(), 8ull * MRG_NBUCKET);
        stage_h2d(c, d_bcap16, bcap16_32.data(), 4ull * MRG_NBUCKET);
        A.rbase = d_rbase; A.bcap = d_bcap; A.rbase16 = d_rbase16; A.bcap16 = d_bcap16;
        // 12-byte (wc) / 24-byte (indexer) records, + 16 bytes: readers may load a 12-byte record as 16
        A.pool = att.get<uint64_t>((rtot * MRG_TAIL_BYTES(idx) + 16 + 7) / 8);
        A.pool16 = att.get<uint64_t>(2 * rtot16 + 2);
        A.fk0 = att.get<uint64_t>((uint64_t)grid * cap);
        A.fk1 = att.get<uint64_t>((uint64_t)grid * cap);
        A.fcnt = att.get<uint32_t>((uint64_t)grid * cap);
        A.fdoc = idx ? att.get<uint32_t>((uint64_t)grid * cap) : nullptr;
        A.foff = att.get<uint32_t>((uint64_t)grid * (MRG_NBUCKET + 1));
        const uint64_t lslots = map_args_shared(c, att, A, in, ms, lcap, launches == 0, launches);
        A.prof = nullptr;
        if (getenv("MRG_PROF")) {
            A.prof = att.get<unsigned long long>(8 + 8ull * grid);
            HIPCHK(hipMemsetAsync(A.prof, 0, 8ull * (8 + 8ull * grid), s));
        }
        stage_fill(c, c->d_cnt, 0, sizeof(unsigned long long) * CNT_N);
        stage_fill(c, &c->d_cnt[CNT_ERRPOS], 0xFF, sizeof(unsigned long long));
        stage_h2d(c, dargs, &A, sizeof(MapArgs));
        flush_stage(c);
        ev_rec(c, c->ev, 0);
        // (MRG_TEST_TAIL64=1: the 64-bit cursors whatever the sizes, for the tests.  The forced-collision hash
        // mask, a test knob too, exists in that general variant only: the packed one hashes in full)
        const bool tail64 = !map_tail_packed(rtot, rtot16, ms) || A.hash_bits != 0 || env_u64("MRG_TEST_TAIL64", 0) != 0;
        // also with no tiles: writes empty flush regions
        mrg_launch_map(nullptr, dargs, c->app, grid, c->lds_cap, s, false, tail64);
        ev_rec(c, c->ev, 1);
        HIPCHK(hipGetLastError());
        ++launches;
        // the aggregation queued behind the map before the host sees the map's counters (one host
        // round trip less per job); checked against them below and by bucket_aggregate, and dropped
        // when the map reruns, goes wide or the 32-bit-count guess was wrong
        // (MRG_WIDE=1 forces the wide path, so nothing is queued; MRG_WIDE=0 and MRG_TEST_AGG_NSUB still
        // queue it: their tests run through this path)
        // (r06: also on a cold context's first job when its sample found repeats; the 32-bit-count guess
        // is then "fewer than 2^32 tokens" -- true unless the input holds billions of one-letter words --
        // and bucket_aggregate checks it like every guess: a wrong one only drops the queued launch)
        if (launches == 1 && !idx && (c->spec_agg || cold_repeats) && !A.prof && !wide_forced() &&
            !getenv("MRG_NO_SPEC_AGG") && grid <= 2048) {
            ev_rec(c, c->ev, 2);
            uint32_t nsub = c->agg_nsub;
            if (const uint64_t t = env_u64("MRG_TEST_AGG_NSUB", 0)) nsub = (uint32_t)t;
            const bool c32 = c->spec_agg ? c->spec_c32 : true;
            spec = agg_launch(c, A, (uint32_t)grid, cap, agg_ocap(c), nsub, lslots, c32 && grid <= 512, false);
        }
        // overflow-list fill into pinned scratch, then the counters: one host wait for both
        uint32_t *onext = (uint32_t *)&c->h_cnt[CNT_N + 8];
        HIPCHK(hipMemcpyAsync(onext, A.onext, 4ull * MRG_NBUCKET, hipMemcpyDeviceToHost, s));
        read_counters(c);
        c->st.map_spill = 0;
        for (int b = 0; b < MRG_NBUCKET; ++b) c->st.map_spill += std::min<uint64_t>(onext[b], ocap);
        if (A.prof) map_prof_report(A, grid);
        const bool long_full = c->h_cnt[CNT_LONGX] > A.lovf;
        if (c->h_cnt[CNT_OVF] == 0 && !long_full) break;
        if (spec.live()) c->st.spec_agg = 2;  // the rerun invalidates the queued aggregation
        spec.drop();
        // capacity exceeded: grow each bucket's regions to its demand (remembered), run again
        if (c->h_cnt[CNT_OVF]) {
            std::vector<uint32_t> cnt((uint64_t)grid * MRG_NBUCKET), cnt16((uint64_t)grid * MRG_NBUCKET, 0);
            HIPCHK(hipMemcpyAsync(cnt.data(), A.bcount, 4ull * cnt.size(), hipMemcpyDeviceToHost, s));
            if (!idx) HIPCHK(hipMemcpyAsync(cnt16.data(), A.bcount16, 4ull * cnt16.size(), hipMemcpyDeviceToHost, s));
            sync(c);
            c->bcap_rate.assign(MRG_NBUCKET, 0.0);
            c->bcap16_rate.assign(MRG_NBUCKET, 0.0);
            for (int b = 0; b < MRG_NBUCKET; ++b) {
                uint64_t mx = 0, mx16 = 0;
                for (int g = 0; g < grid; ++g) {
                    mx = std::max<uint64_t>(mx, cnt[(uint64_t)g * MRG_NBUCKET + b]);
                    mx16 = std::max<uint64_t>(mx16, cnt16[(uint64_t)g * MRG_NBUCKET + b]);
                }
                bcap[b] = std::max<uint64_t>(bcap[b], mx + mx / 4 + 64);
                c->bcap_rate[b] = (double)mx / per_wg;
                if (!idx) {
                    bcap16[b] = std::max<uint64_t>(bcap16[b], mx16 + mx16 / 4 + 16);
                    c->bcap16_rate[b] = (double)mx16 / per_wg;
                }
            }
            ocap = c->ocap_hint = 4 * ocap;
        }
        if (long_full) grow_long_regions(c, A, grid, lcap);
        if (getenv("MRG_DEBUG"))
            fprintf(stderr, "[mrgpu] map rerun: tail overflow %llu, long %llu (list %llu of %llu)\n",
                    (unsigned long long)c->h_cnt[CNT_OVF], (unsigned long long)c->h_cnt[CNT_LONG],
                    (unsigned long long)c->h_cnt[CNT_LONGX], (unsigned long long)A.lovf);
        att.put_all();
    }
    if (getenv("MRG_DEBUG"))
        fprintf(stderr, "[mrgpu] map: %llu tokens, %llu tail records, %llu long, %u launches, grid %d\n",
                (unsigned long long)c->h_cnt[CNT_TOKENS], (unsigned long long)c->h_cnt[CNT_REC],
                (unsigned long long)c->h_cnt[CNT_LONG], launches, grid);
    map_stats(c, launches, total);
    c->st.tail_records_16 = is_idx(c) ? 0 : c->h_cnt[CNT_REC16];  // the indexer's are all 24-byte records
    check_map_utf8(c, in.ids);
    if (!spec.live()) ev_rec(c, c->ev, 2);
    const LongItems li = long_items(c, att, A, grid);
    // high cardinality (most tokens missed the map-side combine): sort-based aggregation
    bool wide = !idx && c->h_cnt[CNT_REC] > (32ull << 20) && 2 * c->h_cnt[CNT_REC] > c->h_cnt[CNT_TOKENS];
    if (const char *v = getenv("MRG_WIDE")) wide = !idx && atoi(v) != 0;  // test / tuning override
    if (wide && spec.live()) {  // the queued aggregation was not needed: its counters back to the map's zeros
        c->st.spec_agg = 2;
        spec.drop();
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_KEYS], 0, 8, s));
        HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_OVF2], 0, 8, s));
    }
    if (wide) c->spec_agg = false;
    if (wide || !bucket_aggregate(c, A, (uint32_t)grid, cap, li, &spec)) {
        c->spec_agg = false;
        c->st.agg_path = 2;
        c->wide_hint = !idx;
        wide_aggregate(c, A, (uint32_t)grid, cap, li);
    }
    ev_rec(c, c->ev, 3);
    c->st.ms_aggregate = ev_ms(c, c->ev, 2, 3);
    if (!idx && total >= (64ull << 20)) c->wc_sized = true;
    c->mapped = c->keyed = true;
}

}  // namespace mrg_host
