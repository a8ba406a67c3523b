// mrg_reduce.cpp -- from the job's keys to text: mr-{r}.txt (job_reduce: the key sort and the
// line writer, or the wide result straight from its leaves), final.txt (job_final), the K most frequent lines
// (job_topk).  Owns c->d_out, c->d_final, c->d_top and the indexer's document ranks.
// Calls: mrg_agg.cpp (acc_emit, wide_densify: the consumers' dense key set).
// Called by: mrgpu.cpp, mrg_plugin.cpp, mrg_run.cpp, mrg_vocab.cpp (job_topk).
#include <stddef.h>

#include "mrg_host.h"

using namespace mrg_host;

namespace {

// Indexer document order = bytewise order of the names (the indexer reduce sorts its values):
// rank of each global document id, and the names concatenated in rank order, on the device (blocks of
// the caller's Scratch).
struct DocRank {
    uint32_t *rank = nullptr;
    uint8_t *names = nullptr;
    uint64_t *name_off = nullptr;
};

DocRank doc_ranks(mrg_ctx *c, Scratch &sc) {
    DocRank d;
    if (!is_idx(c)) return d;
    hipStream_t s = c->stream;
    const uint32_t nn = (uint32_t)c->names.size();
    if (nn == 0) raise(MRG_EINVAL, "indexer needs document names (mrg_job_set_doc_names)");
    std::vector<uint32_t> order(nn);
    for (uint32_t i = 0; i < nn; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return c->names[a] < c->names[b]; });
    std::vector<uint32_t> rank(nn);
    std::vector<uint64_t> noff(nn + 1, 0);
    std::string cat;
    for (uint32_t r = 0; r < nn; ++r) {
        rank[order[r]] = r;
        cat += c->names[order[r]];
        noff[r + 1] = cat.size();
    }
    d.rank = sc.get<uint32_t>(nn);
    d.names = sc.get<uint8_t>(cat.size() + 1);
    d.name_off = sc.get<uint64_t>(nn + 1);
    HIPCHK(hipMemcpyAsync(d.rank, rank.data(), 4ull * nn, hipMemcpyHostToDevice, s));
    if (!cat.empty()) HIPCHK(hipMemcpyAsync(d.names, cat.data(), cat.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.name_off, noff.data(), 8ull * (nn + 1), hipMemcpyHostToDevice, s));
    // every key's document id must have a name: rank[id] and name_off[rank + 1] are read without a bound.
    // Covers ids from mrg_job_set_input, mrg_map, mrg_job_import and the accumulator; read back with the
    // sync below.
    uint32_t *d_max = sc.get<uint32_t>(1);
    uint32_t max_id = 0;
    HIPCHK(hipMemsetAsync(d_max, 0, 4, s));
    mrg_launch_max_doc(c->keys.ks, c->keys.n, d_max, s);
    HIPCHK(hipMemcpyAsync(&max_id, d_max, 4, hipMemcpyDeviceToHost, s));
    sync(c);  // host vectors go out of scope
    if (c->keys.n && max_id >= nn)
        raise(MRG_EINVAL, "indexer: document id %u has no name (%u names; mrg_job_set_doc_names)", max_id, nn);
    return d;
}

// Sort records of the keys `ks` by (partition < R, key bytes[, doc rank]) (worker.rs:162-164).
// Returns a or b.  With `defer`, only the MSD passes are enqueued and b is returned: the caller
// checks the oversized-bucket count (c->h_cnt[CNT_N], pinned) after its next stream sync and calls
// mrg_msd_sort_finish if it is not 0 (saves a host round trip per reduce).
SortPlan sort_plan(mrg_ctx *c, uint32_t R) {
    const bool idx = is_idx(c);
    SortPlan plan{};
    plan.use_part = R > 1;
    plan.part_bytes = bytes_for(R - 1);
    plan.use_k0 = plan.use_k1 = true;
    plan.use_doc = idx;
    plan.doc_bytes = idx ? bytes_for(c->names.size() - 1) : 0;
    return plan;
}

SortRec *sort_keys(mrg_ctx *c, KeySet ks, uint32_t R, const uint32_t *d_rank, SortRec *a, SortRec *b, void *stmp,
                   bool defer = false, bool carry = false) {
    const uint64_t n = c->keys.n;
    mrg_launch_make_sortrec(ks, n, d_rank, a, c->stream, carry);
    check_sort_n(n, "key sort");
    const uint32_t pbits = R > 1 ? 32u - (uint32_t)__builtin_clz(R - 1u) : 0u;
    uint32_t *h_nbig = (uint32_t *)&c->h_cnt[CNT_N];
    if (defer) {
        mrg_msd_sort_launch(a, b, n, pbits, stmp, c->stream, h_nbig);
        return n <= 1 ? a : b;
    }
    uint32_t n_big = 0;
    return mrg_msd_sort(a, b, n, pbits, sort_plan(c, R), stmp, c->stream, &n_big, h_nbig);
}

FormatArgs format_args(mrg_ctx *c, const SortRec *recs, KeySet ks, uint32_t R, int drop_last, const DocRank &dr,
                       bool carried = false) {
    FormatArgs f{};
    f.carried = carried ? 1 : 0;
    f.recs = recs;
    f.n = c->keys.n;
    f.ks = ks;
    f.heap = c->keys.heap;
    f.heap_bytes = c->keys.heap_bytes;
    f.n_reduce = R;
    f.drop_last = drop_last;
    f.indexer = is_idx(c);
    f.any_long = c->keys.any_long;
    f.names = dr.names;
    f.name_off = dr.name_off;
    return f;
}

int compat_drop_last(const mrg_ctx *c) { return (c->flags & MRG_FLAG_NO_COMPAT_DROP_LAST) ? 0 : 1; }

// mr-{r}.txt of a wide result straight from its leaves (k_wide.hip): last-group drop on the last
// non-empty leaf of every partition, a scan of the leaf byte totals, the line writer.
void wide_reduce(mrg_ctx *c) {
    WideRes &w = c->wide;
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint64_t NL = (uint64_t)w.B1 * MRG_WIDE_MAXB2;
    ev_rec(c, c->ev, 4);
    uint32_t *drop = sc.get<uint32_t>(NL);
    HIPCHK(hipMemsetAsync(drop, 0, 4 * NL, s));
    uint64_t *bytes = sc.get<uint64_t>(NL + 1), *off = sc.get<uint64_t>(NL + 1);
    uint64_t *tmp = sc.get<uint64_t>(mrg_scan_tmp_elems(NL + 1));
    HIPCHK(hipMemcpyAsync(bytes, w.leaf_bytes, 8 * (NL + 1), hipMemcpyDeviceToDevice, s));
    if (compat_drop_last(c)) mrg_wide_launch_drop(w.nleaf, w.B1r, c->R, w.leaf_nd, bytes, w.leaf_last, drop, s);
    mrg_scan_u64(bytes, off, NL + 1, tmp, s);  // off[NL] = total (bytes[NL] == 0)
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, off + NL, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    ev_rec(c, c->ev, 5);
    if (total + 16 > c->out_cap) {  // (on a failure the context holds no buffer, never a returned one)
        uint8_t *old = c->d_out;
        c->d_out = nullptr;
        c->out_cap = 0;
        c->pool.put(old);
        c->d_out = pget<uint8_t>(c->pool, total + 16);
        c->out_cap = total + 16;
    }
    if (getenv("MRG_DEBUG_FILL_OUT")) HIPCHK(hipMemsetAsync(c->d_out, 0xEE, total, s));  // diagnostics: unwritten bytes show
    mrg_wide_launch_write(w.kout, w.ocnt, w.leaf_pk, w.nleaf, w.leaf_out, w.leaf_nd, drop, off, w.B1, c->d_out, s);
    uint64_t *poff = sc.get<uint64_t>(c->R + 1);
    mrg_wide_launch_part_off(off, w.B1r, c->R, total, poff, s);
    c->part_off.assign(c->R + 1, 0);
    HIPCHK(hipMemcpyAsync(c->part_off.data(), poff, 8ull * (c->R + 1), hipMemcpyDeviceToHost, s));
    ev_rec(c, c->ev, 6);
    sync(c);
    HIPCHK(hipGetLastError());
    c->out_bytes = total;
    c->st.ms_sort = ev_ms(c, c->ev, 4, 5);
    c->st.ms_format = ev_ms(c, c->ev, 5, 6);
    c->st.output_bytes = total;
    c->reduced = true;
}

}  // namespace

namespace mrg_host __attribute__((visibility("hidden"))) {

void job_reduce(mrg_ctx *c) {
    need_job(c);
    if (!c->mapped) raise(MRG_EINVAL, "nothing to reduce: call mrg_job_map or mrg_job_import first");
    acc_emit(c);
    if (c->wide.ready) {
        wide_reduce(c);
        return;
    }
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint64_t n = c->keys.n;
    const DocRank dr = doc_ranks(c, sc);
    ev_rec(c, c->ev, 4);
    SortRec *a = sc.get<SortRec>(n), *b = sc.get<SortRec>(n);
    void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(n));
    SortRec *sorted = a;
    const bool presorted = c->keys.sorted && !c->keys.any_long && !is_idx(c);
    // the oversized-bucket check of the key sort waits for format's own sync (add_first below is
    // not idempotent: that path checks at once)
    const bool defer = !presorted && !(c->extra_first && n);
    // wc: counts and lengths carried in the sort records, unless the text reduce's empty-key quirk
    // adds to the first key's count after the sort
    const bool carry = !is_idx(c) && !c->extra_first;
    if (presorted) mrg_launch_make_sortrec(c->keys.ks, n, nullptr, a, s, carry);
    else sorted = sort_keys(c, c->keys.ks, c->R, dr.rank, a, b, stmp, defer, carry);
    // text reduce (worker.rs:169-173): lines with an empty key sort first and, since `prev` is still
    // empty when the first real key arrives, their values join that key's group
    if (c->extra_first && n) {
        if (c->keys.any_long) mrg_launch_fix_runs(sorted, n, c->keys.ks, c->keys.heap, s);
        mrg_launch_add_first(sorted, c->keys.ks, c->extra_first, s);
    }
    ev_rec(c, c->ev, 5);
    const FormatArgs f = format_args(c, sorted, c->keys.ks, c->R, compat_drop_last(c), dr, carry);
    c->part_off.assign(c->R + 1, 0);
    c->out_bytes = mrg_format(f, c->pool, &c->d_out, &c->out_cap, c->part_off.data(), s);
    const uint32_t n_big = *(const uint32_t *)&c->h_cnt[CNT_N];  // written by the sort's async copy
    if (defer && n > 1 && n_big) {  // oversized MSD buckets: sort them, format again
        sorted = mrg_msd_sort_finish(a, b, n, sort_plan(c, c->R), stmp, s, n_big);
        const FormatArgs f2 = format_args(c, sorted, c->keys.ks, c->R, compat_drop_last(c), dr, carry);
        c->out_bytes = mrg_format(f2, c->pool, &c->d_out, &c->out_cap, c->part_off.data(), s);
    }
    ev_rec(c, c->ev, 6);
    HIPCHK(hipGetLastError());
    c->st.ms_sort = ev_ms(c, c->ev, 4, 5);
    c->st.ms_format = ev_ms(c, c->ev, 5, 6);
    c->st.output_bytes = c->out_bytes;
    c->reduced = true;
}

// final.txt (src/run.sh:16-20 with LC_ALL=C): the lines of every partition this context holds,
// sorted bytewise, written on the device.  The keys the per-partition pass drops (drop-last) are
// found in the partition order, moved to a second "partition" and the rest re-sorted by key alone.
void job_final(mrg_ctx *c) {
    need_job(c);
    if (!c->mapped) raise(MRG_EINVAL, "no keys: call mrg_job_map or mrg_job_import first");
    acc_emit(c);
    wide_densify(c, 0);
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint64_t n = c->keys.n;
    const DocRank dr = doc_ranks(c, sc);
    SortRec *a = sc.get<SortRec>(n), *b = sc.get<SortRec>(n);
    void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(n));
    const int drop = compat_drop_last(c);
    uint32_t *part2 = sc.get<uint32_t>(std::max<uint64_t>(n, 1));
    KeySet ks2 = c->keys.ks;
    ks2.part = part2;
    if (drop) {
        SortRec *s1 = sort_keys(c, c->keys.ks, c->R, dr.rank, a, b, stmp);
        if (c->keys.any_long) mrg_launch_fix_runs(s1, n, c->keys.ks, c->keys.heap, s);
        mrg_launch_final_part(s1, n, c->keys.ks, c->keys.heap, drop, part2, s);
    } else {
        mrg_launch_fill_u32(part2, 0u, n, s);
    }
    const uint32_t R2 = drop ? 2u : 1u;
    SortRec *s2 = sort_keys(c, ks2, R2, dr.rank, a, b, stmp);
    const FormatArgs f = format_args(c, s2, ks2, R2, 0, dr);
    uint64_t po[3] = {0, 0, 0};
    mrg_format(f, c->pool, &c->d_final, &c->final_cap, po, s);
    HIPCHK(hipGetLastError());
    c->final_bytes = po[1];
    c->finalized = true;
}

// The first k lines of final.txt re-ordered by (count descending, key bytes ascending), without
// sorting the keys (k_topk.hip): at most R keys are dropped, so these lines lie
// within the k + R best keys; a radix select finds those, and only they are sorted and formatted.
// Reads the key set only: reduce, final and export afterwards give what they give without it.
// keep: the ranked records of the lines written (idx = key index in c->keys) become a block of *keep and
// are returned; null when no line was written (mrg_job_vocab).
SortRec *job_topk(mrg_ctx *c, uint64_t k, Scratch *keep) {
    need_job(c);
    if (is_idx(c)) raise(MRG_EINVAL, "mrg_job_topk: word count only (the indexer has no counts to rank)");
    if (!c->mapped) raise(MRG_EINVAL, "no keys: call mrg_job_map or mrg_job_import first");
    acc_emit(c);
    wide_densify(c, 0);
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    const uint64_t n = c->keys.n;
    const KeySet ks = c->keys.ks;
    memset(c->top_info, 0, sizeof c->top_info);
    memset(c->top_pass_bytes, 0, sizeof c->top_pass_bytes);
    c->top_info[0] = n;
    c->top_bytes = c->top_lines = 0;
    c->topped = true;  // (an empty answer is an answer; a failure below clears it again)
    if (k == 0 || n == 0) return nullptr;
    c->topped = false;
    check_sort_n(n, "top-k");
    const uint64_t want = std::min<uint64_t>(n, k > n ? n : k + c->R);  // (k > n: no overflow of k + R)
    TopkState *st = sc.get<TopkState>(1);
    HIPCHK(hipMemsetAsync(st, 0, sizeof(TopkState), s));
    TopkState h{};
    uint64_t m = n;  // candidates
    if (want < n) {
        mrg_topk_select(ks, n, want, st, s);
        HIPCHK(hipMemcpyAsync(&h, st, offsetof(TopkState, hist), hipMemcpyDeviceToHost, s));
        sync(c);  // the one host wait of the select: the candidate count sizes what follows
        m = h.better + h.tied;
        if (m < want || m > n) raise(MRG_EHIP, "top-k select: %llu candidates for %llu wanted of %llu keys",
                                     (unsigned long long)m, (unsigned long long)want, (unsigned long long)n);
        for (uint32_t d = 0; d < MRG_TOPK_DIGITS; ++d)
            if (h.parts[d]) c->top_pass_bytes[d] = 8 * n + (d >= 8 ? 8 * h.parts[8] : 0) + (d >= 16 ? 8 * h.parts[16] : 0);
    }
    SortRec *a = sc.get<SortRec>(m), *b = sc.get<SortRec>(m);
    void *stmp = sc.get<uint8_t>(mrg_sort_tmp_bytes(m));
    mrg_topk_compact(ks, n, st, a, m, s);
    // key order of the candidates (part unused), full-string order where long keys share a prefix
    uint32_t n_big = 0;
    SortRec *sorted = mrg_msd_sort(a, b, m, 0, sort_plan(c, 1), stmp, s, &n_big, (uint32_t *)&c->h_cnt[CNT_N]);
    if (c->keys.any_long) mrg_launch_fix_runs(sorted, m, ks, c->keys.heap, s);
    // drop-last: the byte-largest candidate of a partition is dropped iff no key of the partition exceeds it
    uint32_t *cand_last = nullptr, *exceeded = nullptr;
    if (compat_drop_last(c)) {
        cand_last = sc.get<uint32_t>(2ull * c->R);
        exceeded = cand_last + c->R;
        HIPCHK(hipMemsetAsync(cand_last, 0, 8ull * c->R, s));
        mrg_topk_cand_last(sorted, m, ks, c->R, cand_last, s);
        if (m < n) mrg_topk_exceed(ks, c->keys.heap, n, sorted, c->R, cand_last, exceeded, s);  // (m == n: none can)
    }
    // then a stable sort by ~count: count descending, key order kept among equal counts
    uint64_t *ckeys = sc.get<uint64_t>(m), *kvtmp = sc.get<uint64_t>(4 * m);
    uint32_t *vals = sc.get<uint32_t>(m);
    mrg_topk_count_keys(sorted, m, ks, c->R, cand_last, exceeded, ckeys, vals, st, s);
    mrg_radix_sort_u64(ckeys, vals, kvtmp, m, stmp, s);
    SortRec *top = sorted == a ? b : a;
    mrg_topk_gather(sorted, vals, m, top, s);
    HIPCHK(hipMemcpyAsync(&h, st, offsetof(TopkState, hist), hipMemcpyDeviceToHost, s));
    sync(c);
    const uint64_t lines = std::min<uint64_t>(k, m - std::min<uint64_t>(m, h.ndrop));
    // the wc line writer over the first `lines` records, as one partition; not any_long: the records
    // are no longer in key order, and their long-key runs are already in full-string order
    FormatArgs f{};
    f.recs = top;
    f.n = lines;
    f.ks = ks;
    f.heap = c->keys.heap;
    f.heap_bytes = c->keys.heap_bytes;
    f.n_reduce = 1;
    uint64_t po[2] = {0, 0};
    mrg_format(f, c->pool, &c->d_top, &c->top_cap, po, s);
    HIPCHK(hipGetLastError());
    c->top_bytes = po[1];
    c->top_lines = lines;
    c->topped = true;
    c->top_info[1] = m;
    c->top_info[2] = h.passes;
    c->top_info[3] = h.ndrop;
    return keep ? keep->adopt(sc.release(top)) : nullptr;
}

}  // namespace mrg_host
