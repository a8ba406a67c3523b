// mrg_plugin.cpp -- the host-buffer surfaces of libmrgpu.so (include/mrgpu.h): the reference's text
// intermediates mr-{m}-{r}.txt, byte for byte (mrg_map_text, mrg_reduce_text), and the plugin
// calls (mrg_map with its mrg_parts, mrg_reduce).  Each is a whole job on the caller's context: input from host
// memory, output into a malloc'd buffer the caller frees with mrg_free.  Also check_names, the rule for document
// names that every surface applies.
// Calls: mrgpu.cpp (job_begin), mrg_map.cpp (job_map, read_counters), mrg_exchange.cpp (export_sizes,
// export_pack, import_recs, job_import), mrg_reduce.cpp (job_reduce).
// text_map and text_reduce stand outside any namespace, as they always have, and so remain among the library's
// dynamic symbols: the split of the host layer into units changed no symbol.
#include <stdlib.h>

#include <memory>

#include "mrg_host.h"

using namespace mrg_host;

struct mrg_parts {
    uint32_t R = 0;
    std::vector<uint64_t> rec_off, heap_off;  // [R + 1]
    std::vector<uint8_t> recs, heap;
};

namespace mrg_host __attribute__((visibility("hidden"))) {

void check_names(const char *const *names, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        if (!names[i]) raise(MRG_EINVAL, "null document name %u", i);
        for (const char *q = names[i]; *q; ++q)
            if (*q == ' ' || *q == ',' || *q == '\n')
                raise(MRG_EINVAL, "document name '%s' contains ' ', ',' or newline", names[i]);
    }
}

}  // namespace mrg_host

// ---- text intermediates: the reference's mr-{m}-{r}.txt, byte for byte

// One map task's intermediates: "key 1\n" per token in input order, partition by SipHash % R
// (worker.rs:117-140).  out = the R files' bytes concatenated, off[R + 1] their offsets.
void text_map(mrg_ctx *c, const uint8_t *h, uint64_t n, uint32_t R, std::vector<uint8_t> &out,
              std::vector<uint64_t> &off) {
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    uint8_t *d = sc.get<uint8_t>(n + 64);
    if (n) HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s));
    const uint64_t nseg = mrg_text_segments(n);
    uint64_t *cnt = sc.get<uint64_t>(nseg + 1), *base = sc.get<uint64_t>(nseg + 1);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(nseg + 1));
    HIPCHK(hipMemsetAsync(cnt, 0, 8 * (nseg + 1), s));
    HIPCHK(hipMemsetAsync(&c->d_cnt[CNT_ERRPOS], 0xFF, 8, s));
    mrg_launch_text_tok(d, n, R, nullptr, cnt, nullptr, &c->d_cnt[CNT_ERRPOS], s);
    mrg_scan_u64(cnt, base, nseg + 1, stmp, s);
    uint64_t T = 0;
    HIPCHK(hipMemcpyAsync(&T, base + nseg, 8, hipMemcpyDeviceToHost, s));
    read_counters(c);
    if (c->h_cnt[CNT_ERRPOS] != ~0ull)
        raise(MRG_EUTF8, "stream did not contain valid UTF-8: byte offset %llu", (unsigned long long)c->h_cnt[CNT_ERRPOS]);
    off.assign(R + 1, 0);
    out.clear();
    if (T) {
        TextTok *tok = sc.get<TextTok>(T);
        mrg_launch_text_tok(d, n, R, base, cnt, tok, &c->d_cnt[CNT_ERRPOS], s);
        uint64_t *part = sc.get<uint64_t>(T), *kv = sc.get<uint64_t>(4 * T);
        uint32_t *idx = sc.get<uint32_t>(T);
        void *stmp2 = sc.get<uint8_t>(mrg_sort_tmp_bytes(T));
        mrg_launch_text_keys(tok, T, part, idx, s);
        check_sort_n(T, "text partition sort");
        mrg_radix_sort_u64(part, idx, kv, T, stmp2, s);  // stable: input order inside a partition
        uint64_t *L = sc.get<uint64_t>(T + 1), *O = sc.get<uint64_t>(T + 1);
        uint64_t *stmp3 = sc.get<uint64_t>(mrg_scan_tmp_elems(T + 1));
        mrg_launch_text_len(tok, idx, T, L, s);
        mrg_scan_u64(L, O, T, stmp3, s);
        uint64_t last[2];
        HIPCHK(hipMemcpyAsync(&last[0], O + (T - 1), 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&last[1], L + (T - 1), 8, hipMemcpyDeviceToHost, s));
        sync(c);
        const uint64_t total = last[0] + last[1];
        uint8_t *ob = sc.get<uint8_t>(total + 16);
        uint64_t *doff = sc.get<uint64_t>(R + 1);
        mrg_launch_text_write(d, tok, idx, T, O, ob, s);
        mrg_launch_text_part_off(part, O, T, R, total, doff, s);
        out.resize(total);
        HIPCHK(hipMemcpyAsync(out.data(), ob, total, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(off.data(), doff, 8ull * (R + 1), hipMemcpyDeviceToHost, s));
        sync(c);
    }
}

// One reduce task from text intermediates (worker.rs:79-109, 157-193): returns mr-{r}.txt.
void text_reduce(mrg_ctx *c, const uint8_t *const *files, const uint64_t *sizes, size_t k, uint32_t flags,
                 std::vector<uint8_t> &out) {
    job_begin(c, MRG_APP_WC, 1, flags);  // every key read goes to the one output file
    Scratch sc(c->pool);
    hipStream_t s = c->stream;
    std::vector<uint64_t> fo(k + 1, 0), fe(k);
    for (size_t i = 0; i < k; ++i) {
        fe[i] = fo[i] + sizes[i];
        fo[i + 1] = (fe[i] + 63) & ~63ull;  // files on 64-byte boundaries (one file per segment)
    }
    const uint64_t total = fo[k];
    uint8_t *d = sc.get<uint8_t>(total + 64);
    HIPCHK(hipMemsetAsync(d, 0, total + 64, s));
    for (size_t i = 0; i < k; ++i)
        if (sizes[i]) HIPCHK(hipMemcpyAsync(d + fo[i], files[i], sizes[i], hipMemcpyHostToDevice, s));
    const uint32_t nf = (uint32_t)std::max<size_t>(k, 1);
    uint64_t *dfo = sc.get<uint64_t>(nf + 1), *dfe = sc.get<uint64_t>(nf);
    if (k) {
        HIPCHK(hipMemcpyAsync(dfo, fo.data(), 8 * k, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dfe, fe.data(), 8 * k, hipMemcpyHostToDevice, s));
    }
    unsigned long long *err = sc.get<unsigned long long>(3);  // [utf8 pos, format pos, empty-key lines]
    HIPCHK(hipMemsetAsync(err, 0xFF, 16, s));
    HIPCHK(hipMemsetAsync(err + 2, 0, 8, s));
    mrg_launch_utf8_check(d, total, err, s);  // read_to_string (worker.rs:93); zero padding is valid
    const uint64_t nseg = total / 64;
    uint64_t *cnt = sc.get<uint64_t>(nseg + 1), *base = sc.get<uint64_t>(nseg + 1);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(nseg + 1));
    HIPCHK(hipMemsetAsync(cnt, 0, 8 * (nseg + 1), s));
    if (k) mrg_launch_text_lines(d, dfo, dfe, nf, nseg, nullptr, cnt, nullptr, err, err + 2, s);
    mrg_scan_u64(cnt, base, nseg + 1, stmp, s);
    std::vector<uint64_t> fb(k + 1, 0);  // records before file i = base[fo[i] / 64]
    for (size_t i = 0; i <= k; ++i) HIPCHK(hipMemcpyAsync(&fb[i], base + fo[i] / 64, 8, hipMemcpyDeviceToHost, s));
    unsigned long long herr[3];
    HIPCHK(hipMemcpyAsync(herr, err, sizeof herr, hipMemcpyDeviceToHost, s));
    sync(c);
    auto where = [&](uint64_t pos, uint64_t &f) {
        f = 0;
        while (f + 1 < k && fo[f + 1] <= pos) ++f;
        return pos - fo[f];
    };
    if (herr[0] != ~0ull) {
        uint64_t f;
        const uint64_t at = where(herr[0], f);
        raise(MRG_EUTF8, "intermediate file %llu is not valid UTF-8 (byte offset %llu)", (unsigned long long)f,
              (unsigned long long)at);
    }
    if (herr[1] != ~0ull) {
        uint64_t f;
        const uint64_t at = where(herr[1], f);
        raise(MRG_EINVAL, "intermediate file %llu: the line at byte %llu does not split into `key value` "
              "(worker.rs:100 asserts two space-separated fields; keys hold no NUL)", (unsigned long long)f,
              (unsigned long long)at);
    }
    const uint64_t N = fb[k];
    LRec *x = sc.get<LRec>(std::max<uint64_t>(N, 1));
    if (k) mrg_launch_text_lines(d, dfo, dfe, nf, nseg, base, cnt, x, err, err + 2, s);  // also counts empty keys
    HIPCHK(hipMemcpyAsync(&herr[2], err + 2, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    std::vector<uint64_t> seg_rec(nf, 0), seg_heap(nf, 0);
    for (size_t i = 0; i < k; ++i) {
        seg_rec[i] = fb[i + 1] - fb[i];
        seg_heap[i] = fo[i + 1] - fo[i];  // heap segment of file i = its slot in the buffer
    }
    import_recs(c, nullptr, x, N, d, k ? total : 0, seg_rec.data(), seg_heap.data(), nf);
    c->extra_first = herr[2];
    job_reduce(c);
    out.resize(c->out_bytes);
    if (c->out_bytes) HIPCHK(hipMemcpyAsync(out.data(), c->d_out, c->out_bytes, hipMemcpyDeviceToHost, s));
    sync(c);
    if (c->keys.n == 0 && herr[2] && (flags & MRG_FLAG_NO_COMPAT_DROP_LAST)) {  // only empty keys, group kept
        const std::string line = " " + std::to_string(herr[2]) + "\n";
        out.assign(line.begin(), line.end());
    }
}

extern "C" {

// ---- text intermediates
int mrg_map_text(mrg_ctx *c, const uint8_t *h_bytes, size_t n, uint32_t n_reduce, uint8_t **h_out,
                 uint64_t *h_part_off) {
    return guard([&] {
        if (!c || !h_out || !h_part_off || (n && !h_bytes)) raise(MRG_EINVAL, "null argument");
        if (n_reduce == 0) raise(MRG_EINVAL, "n_reduce must be > 0");
        HIPCHK(hipSetDevice(c->device));
        std::vector<uint8_t> out;
        std::vector<uint64_t> off;
        text_map(c, h_bytes, n, n_reduce, out, off);
        uint8_t *o = (uint8_t *)malloc(out.size() + 1);
        if (!o) raise(MRG_ENOMEM, "host allocation failed");
        if (!out.empty()) memcpy(o, out.data(), out.size());
        memcpy(h_part_off, off.data(), 8ull * (n_reduce + 1));
        *h_out = o;
    });
}

int mrg_reduce_text(mrg_ctx *c, const uint8_t *const *h_files, const uint64_t *h_sizes, size_t k, uint32_t flags,
                    uint8_t **h_out, size_t *h_out_len) {
    return guard([&] {
        if (!c || !h_out || !h_out_len || (k && (!h_files || !h_sizes))) raise(MRG_EINVAL, "null argument");
        for (size_t i = 0; i < k; ++i)
            if (h_sizes[i] && !h_files[i]) raise(MRG_EINVAL, "null file %zu", i);
        HIPCHK(hipSetDevice(c->device));
        std::vector<uint8_t> out;
        text_reduce(c, h_files, h_sizes, k, flags, out);
        uint8_t *o = (uint8_t *)malloc(out.size() + 1);
        if (!o) raise(MRG_ENOMEM, "host allocation failed");
        if (!out.empty()) memcpy(o, out.data(), out.size());
        *h_out = o;
        *h_out_len = out.size();
    });
}

// ---- plugin surface (host buffers)

int mrg_map(mrg_ctx *c, int app, const uint8_t *h_bytes, size_t n, const char *doc, uint32_t doc_id,
            uint32_t n_reduce, uint32_t flags, mrg_parts **out) {
    return guard([&] {
        if (!c || !out || (n && !h_bytes)) raise(MRG_EINVAL, "null argument");
        (void)doc;
        HIPCHK(hipSetDevice(c->device));
        job_begin(c, app, n_reduce, flags);
        Scratch sc(c->pool);
        uint8_t *d = sc.get<uint8_t>(n + 64);
        if (n) HIPCHK(hipMemcpyAsync(d, h_bytes, n, hipMemcpyHostToDevice, c->stream));
        const uint64_t off[2] = {0, n};
        c->d_in = d;
        c->doc_off.assign(off, off + 2);
        c->doc_ids.assign(1, doc_id);
        job_map(c);
        export_sizes(c, n_reduce, nullptr, nullptr);
        std::unique_ptr<mrg_parts> P(new mrg_parts());
        P->R = n_reduce;
        P->rec_off.assign(n_reduce + 1, 0);
        P->heap_off.assign(n_reduce + 1, 0);
        for (uint32_t r = 0; r < n_reduce; ++r) {
            P->rec_off[r + 1] = P->rec_off[r] + c->exp_rec[r];
            P->heap_off[r + 1] = P->heap_off[r] + c->exp_heap[r];
        }
        XRec *dx = sc.get<XRec>(P->rec_off[n_reduce]);
        uint8_t *dh = sc.get<uint8_t>(P->heap_off[n_reduce] + 1);
        export_pack(c, dx, dh);
        P->recs.resize(P->rec_off[n_reduce] * sizeof(XRec));
        P->heap.resize(P->heap_off[n_reduce]);
        if (!P->recs.empty())
            HIPCHK(hipMemcpyAsync(P->recs.data(), dx, P->recs.size(), hipMemcpyDeviceToHost, c->stream));
        if (!P->heap.empty())
            HIPCHK(hipMemcpyAsync(P->heap.data(), dh, P->heap.size(), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        *out = P.release();
    });
}

int mrg_parts_get(const mrg_parts *P, uint32_t r, const uint8_t **h_rec, uint64_t *n_rec, const uint8_t **h_heap,
                  uint64_t *heap_bytes) {
    return guard([&] {
        if (!P || r >= P->R) raise(MRG_EINVAL, "bad parts / partition");
        if (h_rec) *h_rec = P->recs.data() + P->rec_off[r] * sizeof(XRec);
        if (n_rec) *n_rec = P->rec_off[r + 1] - P->rec_off[r];
        if (h_heap) *h_heap = P->heap.data() + P->heap_off[r];
        if (heap_bytes) *heap_bytes = P->heap_off[r + 1] - P->heap_off[r];
    });
}

void mrg_parts_free(mrg_parts *P) { delete P; }

int mrg_reduce(mrg_ctx *c, int app, uint32_t r, const mrg_parts *const *in, size_t k, uint32_t n_reduce,
               uint32_t flags, const char *const *doc_names, uint32_t n_docs, uint8_t **h_out, size_t *h_out_len) {
    return guard([&] {
        if (!c || !h_out || !h_out_len || (k && !in)) raise(MRG_EINVAL, "null argument");
        if (r >= n_reduce) raise(MRG_EINVAL, "partition %u >= n_reduce %u", r, n_reduce);
        HIPCHK(hipSetDevice(c->device));
        job_begin(c, app, n_reduce, flags);
        if (app == MRG_APP_INDEXER) {
            check_names(doc_names, n_docs);
            c->names.assign(doc_names, doc_names + n_docs);
        }
        std::vector<uint64_t> seg_rec, seg_heap;
        std::vector<uint8_t> recs, heap;
        for (size_t i = 0; i < k; ++i) {
            const mrg_parts *P = in[i];
            if (!P || P->R != n_reduce) raise(MRG_EINVAL, "map output %zu has a different n_reduce", i);
            const uint64_t a = P->rec_off[r], b = P->rec_off[r + 1];
            const uint64_t ha = P->heap_off[r], hb = P->heap_off[r + 1];
            recs.insert(recs.end(), P->recs.begin() + a * sizeof(XRec), P->recs.begin() + b * sizeof(XRec));
            heap.insert(heap.end(), P->heap.begin() + ha, P->heap.begin() + hb);
            seg_rec.push_back(b - a);
            seg_heap.push_back(hb - ha);
        }
        const uint64_t nrec = recs.size() / sizeof(XRec);
        Scratch sc(c->pool);
        uint8_t *dr = sc.get<uint8_t>(recs.size() + 16);
        uint8_t *dh = sc.get<uint8_t>(heap.size() + 16);
        if (!recs.empty()) HIPCHK(hipMemcpyAsync(dr, recs.data(), recs.size(), hipMemcpyHostToDevice, c->stream));
        if (!heap.empty()) HIPCHK(hipMemcpyAsync(dh, heap.data(), heap.size(), hipMemcpyHostToDevice, c->stream));
        job_import(c, dr, nrec, dh, heap.size(), seg_rec.data(), seg_heap.data(), (uint32_t)seg_rec.size());
        job_reduce(c);
        const uint64_t a = c->part_off[r], b = c->part_off[r + 1];
        std::unique_ptr<uint8_t, decltype(&free)> o((uint8_t *)malloc(b - a + 1), free);  // (freed if the copy fails)
        if (!o) raise(MRG_ENOMEM, "host allocation failed");
        if (b > a) HIPCHK(hipMemcpyAsync(o.get(), c->d_out + a, b - a, hipMemcpyDeviceToHost, c->stream));
        sync(c);
        *h_out_len = b - a;
        *h_out = o.release();
    });
}

}  // extern "C"
