// mrg_vocab.cpp -- the vocabulary calls of libmrgpu.so (include/mrgpu.h): a vocabulary from a job's ranked keys
// or from text, text -> ids, ids -> text, per-document term counts, the inverted index, BM25 search over it -- in
// one piece, or in shards with the collection's statistics and a merge of the shards' rows; and their diagnostics.
// Apart from mrg_job_vocab, which ranks the job's keys through job_topk, no call touches job state: each uses the
// context's device, stream, timing switch and pool, whose scratch goes back on every exit, and its own VocDiag.
#include <math.h>

#include <memory>

#include "mrg_host.h"

using namespace mrg_host;

namespace {

void vocab_destroy(mrg_vocab *v) {
    if (!v) return;
    if (v->block) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(v->device);
        (void)hipFree(v->block);
        if (cur >= 0 && cur != v->device) (void)hipSetDevice(cur);
    }
    delete v;
}

struct VocDel {
    void operator()(mrg_vocab *v) const { vocab_destroy(v); }
};
using VocPtr = std::unique_ptr<mrg_vocab, VocDel>;

// The block of a vocabulary of n words over text_bytes of text, laid out and allocated; nothing in it is
// written yet except line_off[0] of the empty vocabulary.  Layout: text | line_off | table k0, k1, id |
// wlen | packed words (the last two are the decoder's: the encoder's part is as it was).
VocPtr vocab_alloc(mrg_ctx *c, uint64_t n, uint64_t text_bytes, uint32_t hbits) {
    if (n > 0xFFFFFFFEull) raise(MRG_EINVAL, "vocabulary of %llu words: ids are 32 bits", (unsigned long long)n);
    VocPtr v(new mrg_vocab());
    v->device = c->device;
    v->n = n;
    v->text_bytes = text_bytes;
    const uint64_t cap = pow2_at_least(2 * n);
    auto up = [](uint64_t x) { return (x + 255) & ~255ull; };
    const uint64_t o_text = 0, o_loff = o_text + up(text_bytes + 16), o_k0 = o_loff + up(8 * (n + 1)),
                   o_k1 = o_k0 + 8 * cap, o_id = o_k1 + 8 * cap, o_wlen = o_id + 4 * cap, o_pk = o_wlen + up(4 * n),
                   total = o_pk + up(16 * n);
    if (hipMalloc(&v->block, total) != hipSuccess) {
        (void)hipGetLastError();
        v->block = nullptr;
        raise(MRG_ENOMEM, "vocabulary: device allocation of %llu bytes failed", (unsigned long long)total);
    }
    uint8_t *blk = (uint8_t *)v->block;
    VocTable &T = v->T;
    T.k0 = (uint64_t *)(blk + o_k0);
    T.k1 = (uint64_t *)(blk + o_k1);
    T.id = (uint32_t *)(blk + o_id);
    T.cap = cap;
    T.hash_bits = hbits;
    T.text = blk + o_text;
    T.line_off = (const uint64_t *)(blk + o_loff);
    T.n = n;
    v->W.wlen = (uint32_t *)(blk + o_wlen);
    v->W.pk = (uint64_t *)(blk + o_pk);
    if (!n) HIPCHK(hipMemsetAsync(blk + o_loff, 0, 8, c->stream));
    return v;
}

// The table and the packed words over the block's text, line offsets and word lengths (enqueued before);
// waits for the build.
void vocab_build(mrg_ctx *c, mrg_vocab *v, Scratch &sc) {
    hipStream_t s = c->stream;
    unsigned long long *fail = sc.get<unsigned long long>(1);
    HIPCHK(hipMemsetAsync(fail, 0, 8, s));
    mrg_voc_launch_build(v->T, v->W.wlen, fail, s);
    mrg_voc_launch_words(v->T, v->W, s);
    HIPCHK(hipGetLastError());
    unsigned long long hfail = 0;
    HIPCHK(hipMemcpyAsync(&hfail, fail, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    if (hfail) raise(MRG_EHIP, "vocabulary: %llu words found no table slot", hfail);
}

// The vocabulary of the job's keys: mrg_job_topk's ranked lines, cut at
// min_count, copied with their line offsets into one allocation of the vocabulary's own, and the
// word -> id table over that copy.
mrg_vocab *job_vocab(mrg_ctx *c, uint64_t max_words, uint64_t min_count) {
    need_job(c);
    if (is_idx(c)) raise(MRG_EINVAL, "mrg_job_vocab: word count only (the indexer has no counts to rank)");
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    Scratch sc(p);
    c->enc.make(c);
    c->enc.rec(c, 4);
    SortRec *top = job_topk(c, max_words ? max_words : ~0ull, &sc);
    const uint64_t m = top ? c->top_lines : 0;
    uint64_t n = 0, text_bytes = 0;
    uint64_t *loff = nullptr;
    uint32_t *wlen = nullptr;
    if (m) {
        loff = sc.get<uint64_t>(m + 1);
        wlen = sc.get<uint32_t>(m);
        uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(m + 1));
        unsigned long long *nk = sc.get<unsigned long long>(1);
        HIPCHK(hipMemsetAsync(nk, 0, 8, s));
        mrg_voc_launch_lines(top, m, c->keys.ks, min_count, loff, wlen, nk, s);
        mrg_scan_u64(loff, loff, m + 1, stmp, s);
        HIPCHK(hipMemcpyAsync(&n, nk, 8, hipMemcpyDeviceToHost, s));
        sync(c);
        if (n > m) raise(MRG_EHIP, "vocabulary: %llu of %llu lines kept", (unsigned long long)n, (unsigned long long)m);
        HIPCHK(hipMemcpyAsync(&text_bytes, loff + n, 8, hipMemcpyDeviceToHost, s));
        sync(c);
        if (text_bytes > c->top_bytes) raise(MRG_EHIP, "vocabulary: line offsets exceed the ranked text");
    }
    VocPtr v = vocab_alloc(c, n, text_bytes, hash_bits(c));
    uint8_t *blk = (uint8_t *)v->block;
    if (text_bytes) HIPCHK(hipMemcpyAsync(blk, c->d_top, text_bytes, hipMemcpyDeviceToDevice, s));
    if (n) HIPCHK(hipMemcpyAsync((void *)v->T.line_off, loff, 8 * (n + 1), hipMemcpyDeviceToDevice, s));
    if (n) HIPCHK(hipMemcpyAsync(v->W.wlen, wlen, 4 * n, hipMemcpyDeviceToDevice, s));
    vocab_build(c, v.get(), sc);
    c->enc.rec(c, 5);
    sync(c);
    c->enc.ms[3] = c->enc.elapsed(c, 4, 5);
    return v.release();
}

// What every call over a vocabulary checks first: a context, a vocabulary of its device, a document count with
// room for its n_docs + 1 offsets (any_n_docs: mrg_vocab_postings bounds doc_base + n_docs instead).  voc_enter,
// after the call's own checks: the host offsets do not decrease (fmt may name the row); the device is made current.
void voc_args(const mrg_ctx *c, const mrg_vocab *v, uint32_t n_docs, bool any_n_docs = false) {
    if (!c) raise(MRG_EINVAL, "null context");
    if (!v) raise(MRG_EINVAL, "null vocabulary");
    if (v->device != c->device) raise(MRG_EINVAL, "the vocabulary lives on device %d, the context on device %d", v->device,
                                      c->device);
    if (n_docs == 0xFFFFFFFFu && !any_n_docs) raise(MRG_EINVAL, "n_docs out of range");
}
void voc_enter(const mrg_ctx *c, const uint64_t *off, uint32_t n_docs, const char *fmt) {
    for (uint32_t i = 0; i < n_docs; ++i)
        if (off[i + 1] < off[i]) raise(MRG_EINVAL, fmt, i);
    HIPCHK(hipSetDevice(c->device));
}

// no input in [off[0], off[n_docs]): the call's output offsets are all 0
bool voc_empty(const uint64_t *off, uint32_t n_docs, uint64_t *h_out_off) {
    if (off[n_docs] != off[0]) return false;
    std::fill(h_out_off, h_out_off + n_docs + 1, 0);
    return true;
}

// Text -> ids (k_encode.hip): boundary bitmap, count pass, scan, per-document offsets, emit pass.
void vocab_encode(mrg_ctx *c, const mrg_vocab *v, const uint8_t *d_bytes, const uint64_t *h_doc_off, uint32_t n_docs,
                  uint32_t *d_ids, uint64_t cap_ids, uint64_t *h_tok_off) {
    voc_args(c, v, n_docs);
    if (!h_doc_off || !h_tok_off) raise(MRG_EINVAL, "null offsets (h_doc_off and h_tok_off need n_docs + 1 entries)");
    if ((uintptr_t)d_bytes & 15u) raise(MRG_EINVAL, "input buffer must be 16-byte aligned");
    voc_enter(c, h_doc_off, n_docs, "document offsets must be non-decreasing");
    c->enc.clear(3);
    if (voc_empty(h_doc_off, n_docs, h_tok_off)) return;  // no bytes: no tokens
    const uint64_t lo0 = h_doc_off[0], hi0 = h_doc_off[n_docs];
    if (!d_bytes) raise(MRG_EINVAL, "null input");
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    Scratch sc(p);
    c->enc.make(c);
    // positions relative to the 1 KiB boundary at or below the first document
    const uint64_t shift = lo0 & ~1023ull;
    std::vector<uint64_t> rel(h_doc_off, h_doc_off + n_docs + 1);
    for (auto &x : rel) x -= shift;
    EncPlan P{};
    P.in = d_bytes + shift;
    P.lo = lo0 - shift;
    P.hi = hi0 - shift;
    P.ntiles = (P.hi + 1023) >> 10;
    P.n_docs = n_docs;
    const uint64_t bw = mrg_enc_bitmap_words(P.ntiles);
    P.bnd = sc.get<uint32_t>(bw);
    uint64_t *d_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    P.doc_off = d_off;
    P.cnt = sc.get<uint64_t>(P.ntiles + 1);
    P.tok_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(P.ntiles + 1));
    unsigned long long *small = sc.get<unsigned long long>(9);  // err, info[8]
    P.err = small;
    P.info = small + 1;
    c->enc.info[5] = hi0 - lo0;
    c->enc.info[6] = 4 * bw + 8 * (P.ntiles + 1) + 16 * ((uint64_t)n_docs + 1) + 8 * mrg_scan_tmp_elems(P.ntiles + 1) + 72;
    HIPCHK(hipMemcpyAsync(d_off, rel.data(), 8 * ((uint64_t)n_docs + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.bnd, 0, 4 * bw, s));
    HIPCHK(hipMemsetAsync(P.cnt, 0, 8 * (P.ntiles + 1), s));
    HIPCHK(hipMemsetAsync(P.err, 0xFF, 8, s));
    HIPCHK(hipMemsetAsync(P.info, 0, 64, s));
    mrg_enc_launch_bounds(P, s);
    c->enc.rec(c, 0);
    mrg_enc_launch_count(P, v->T, s);
    c->enc.rec(c, 1);
    mrg_scan_u64(P.cnt, P.cnt, P.ntiles + 1, stmp, s);
    mrg_enc_launch_offsets(P, v->T, s);
    c->enc.rec(c, 2);
    HIPCHK(hipGetLastError());
    unsigned long long herr = 0;
    HIPCHK(hipMemcpyAsync(h_tok_off, P.tok_off, 8 * ((uint64_t)n_docs + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&herr, P.err, 8, hipMemcpyDeviceToHost, s));
    sync(c);  // (also: the pageable `rel` has been read)
    c->enc.ms[0] = c->enc.elapsed(c, 0, 1);
    c->enc.ms[1] = c->enc.elapsed(c, 1, 2);
    if (herr != ~0ull) {
        uint32_t d = 0;
        while (d + 1 < n_docs && rel[d + 1] <= herr) ++d;
        raise(MRG_EUTF8, "stream did not contain valid UTF-8: document %u, byte offset %llu", d,
              (unsigned long long)(herr - rel[d]));
    }
    const uint64_t total = h_tok_off[n_docs];
    if (d_ids) {
        if (cap_ids < total) raise(MRG_EINVAL, "destination too small (%llu ids < %llu tokens)", (unsigned long long)cap_ids,
                                   (unsigned long long)total);
        P.out = d_ids;
        P.out_n = total;
        c->enc.rec(c, 2);
        if (total) mrg_enc_launch_emit(P, v->T, s);
        c->enc.rec(c, 3);
        HIPCHK(hipGetLastError());
    }
    unsigned long long hinfo[8] = {};
    HIPCHK(hipMemcpyAsync(hinfo, P.info, 64, hipMemcpyDeviceToHost, s));
    sync(c);
    if (d_ids) c->enc.ms[2] = c->enc.elapsed(c, 2, 3);
    for (int i = 0; i < 5; ++i) c->enc.info[i] = hinfo[i];
    if (!d_ids) c->enc.info[0] = total;
}

// A vocabulary from its text: the host cuts the lines, the device checks every
// line's UTF-8, its form and its word's codepoints (k_voc_check), builds the table as mrg_job_vocab does, and looks
// every word up again to find a word that stands on two lines (k_voc_verify).  No job state is touched.
mrg_vocab *vocab_from_text(mrg_ctx *c, const uint8_t *h_text, uint64_t bytes, uint32_t flags) {
    if (!c) raise(MRG_EINVAL, "null context");
    if (bytes && !h_text) raise(MRG_EINVAL, "mrg_vocab_from_text: null text");
    if (flags & ~MRG_FLAG_DEBUG_HASH_BITS(0xFFu))
        raise(MRG_EINVAL, "mrg_vocab_from_text: flags 0x%x: only MRG_FLAG_DEBUG_HASH_BITS is accepted", flags);
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint64_t> loff(1, 0);
    for (const uint8_t *p = h_text, *e = h_text + bytes; p < e;) {
        const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(e - p));
        if (!q) raise(MRG_EINVAL, "mrg_vocab_from_text: line %llu: the text does not end in a newline",
                      (unsigned long long)(loff.size() - 1));
        p = q + 1;
        loff.push_back((uint64_t)(p - h_text));
        if (loff.size() - 1 > 0xFFFFFFFEull)
            raise(MRG_EINVAL, "mrg_vocab_from_text: more than %llu lines: ids are 32 bits", 0xFFFFFFFEull);
    }
    const uint64_t n = loff.size() - 1;
    hipStream_t s = c->stream;
    Scratch sc(c->pool);
    c->dec.make(c);
    c->dec.rec(c, 4);
    VocPtr v = vocab_alloc(c, n, bytes, (flags >> 8) & 0xFFu);
    if (n) {
        HIPCHK(hipMemcpyAsync((void *)v->T.text, h_text, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync((void *)v->T.line_off, loff.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
        unsigned long long *err = sc.get<unsigned long long>(2);  // first bad line, first duplicate
        HIPCHK(hipMemsetAsync(err, 0xFF, 16, s));
        mrg_voc_launch_check(v->T, v->W.wlen, err, s);
        HIPCHK(hipGetLastError());
        unsigned long long herr = 0;
        HIPCHK(hipMemcpyAsync(&herr, err, 8, hipMemcpyDeviceToHost, s));
        sync(c);  // (also: the pageable text and offsets have been read)
        if (herr != ~0ull) {
            const unsigned long long line = herr >> 2;
            switch ((uint32_t)(herr & 3u)) {
                case MRG_VOC_BAD_UTF8:
                    raise(MRG_EUTF8, "mrg_vocab_from_text: line %llu: not valid UTF-8", line);
                case MRG_VOC_BAD_CLASS:
                    raise(MRG_EINVAL, "mrg_vocab_from_text: line %llu: the word holds a codepoint that is not \\w", line);
                default:
                    raise(MRG_EINVAL, "mrg_vocab_from_text: line %llu: not `word`, one space, 1 to 20 digits", line);
            }
        }
        vocab_build(c, v.get(), sc);
        mrg_voc_launch_verify(v->T, v->W.wlen, err + 1, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&herr, err + 1, 8, hipMemcpyDeviceToHost, s));
        c->dec.rec(c, 5);
        sync(c);
        if (herr != ~0ull) raise(MRG_EINVAL, "mrg_vocab_from_text: line %llu: duplicate word", herr);
    } else {
        c->dec.rec(c, 5);
        sync(c);
    }
    c->dec.ms[3] = c->dec.elapsed(c, 4, 5);
    return v.release();
}

// Ids -> text (k_decode.hip): boundary bitmap, count pass, scan, per-document offsets, emit pass.
void vocab_decode(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off, uint32_t n_docs,
                  const uint8_t *h_unk, uint32_t unk_len, uint8_t *d_out, uint64_t cap, uint64_t *h_out_off) {
    voc_args(c, v, n_docs);
    if (!h_tok_off || !h_out_off) raise(MRG_EINVAL, "null offsets (h_tok_off and h_out_off need n_docs + 1 entries)");
    if ((uintptr_t)d_ids & 3u) raise(MRG_EINVAL, "the ids must be 4-byte aligned");
    if (unk_len > 255u) raise(MRG_EINVAL, "unk_len %u: at most 255 bytes", unk_len);
    if (unk_len && !h_unk) raise(MRG_EINVAL, "null h_unk with unk_len %u", unk_len);
    voc_enter(c, h_tok_off, n_docs, "token offsets must be non-decreasing");
    c->dec.clear(3);
    if (voc_empty(h_tok_off, n_docs, h_out_off)) return;  // no ids: no bytes
    const uint64_t lo0 = h_tok_off[0], hi0 = h_tok_off[n_docs];
    if (!d_ids) raise(MRG_EINVAL, "null ids");
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    Scratch sc(p);
    c->dec.make(c);
    // positions relative to the 16-byte boundary at or below the first id
    const uint64_t shift = (uint64_t)(((uintptr_t)(d_ids + lo0) & 15u) >> 2);
    std::vector<uint64_t> rel(h_tok_off, h_tok_off + n_docs + 1);
    for (auto &x : rel) x = x - lo0 + shift;
    DecPlan P{};
    P.in = d_ids + lo0 - shift;
    P.lo = shift;
    P.hi = shift + (hi0 - lo0);
    P.nchunks = (P.hi + MRG_DEC_CHUNK - 1) / MRG_DEC_CHUNK;
    P.n_docs = n_docs;
    const uint64_t bw = mrg_dec_bitmap_words(P.nchunks);
    P.bnd = sc.get<uint32_t>(bw);
    uint64_t *d_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    P.tok_off = d_off;
    P.cnt = sc.get<uint64_t>(P.nchunks + 1);
    P.out_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(P.nchunks + 1));
    unsigned long long *small = sc.get<unsigned long long>(1 + 32);  // err, the UNK bytes
    P.err = small;
    P.unk_len = unk_len;
    P.unk = (const uint8_t *)(small + 1);
    for (uint32_t i = 0; i < unk_len && i < 16u; ++i)
        (i < 8u ? P.unk_k0 : P.unk_k1) |= (uint64_t)h_unk[i] << (56u - 8u * (i & 7u));
    c->dec.info[0] = hi0 - lo0;
    c->dec.info[2] = P.nchunks;
    c->dec.info[3] = 4 * bw + 8 * (P.nchunks + 1) + 16 * ((uint64_t)n_docs + 1) + 8 * mrg_scan_tmp_elems(P.nchunks + 1) + 264;
    HIPCHK(hipMemcpyAsync(d_off, rel.data(), 8 * ((uint64_t)n_docs + 1), hipMemcpyHostToDevice, s));
    if (unk_len) HIPCHK(hipMemcpyAsync(small + 1, h_unk, unk_len, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.bnd, 0, 4 * bw, s));
    HIPCHK(hipMemsetAsync(P.cnt, 0, 8 * (P.nchunks + 1), s));
    HIPCHK(hipMemsetAsync(P.err, 0xFF, 8, s));
    mrg_dec_launch_bounds(P, s);
    c->dec.rec(c, 0);
    mrg_dec_launch_count(P, v->T, v->W, s);
    c->dec.rec(c, 1);
    mrg_scan_u64(P.cnt, P.cnt, P.nchunks + 1, stmp, s);
    mrg_dec_launch_offsets(P, v->T, v->W, s);
    c->dec.rec(c, 2);
    HIPCHK(hipGetLastError());
    unsigned long long herr = 0;
    HIPCHK(hipMemcpyAsync(h_out_off, P.out_off, 8 * ((uint64_t)n_docs + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&herr, P.err, 8, hipMemcpyDeviceToHost, s));
    sync(c);  // (also: the pageable `rel` and h_unk have been read)
    c->dec.ms[0] = c->dec.elapsed(c, 0, 1);
    c->dec.ms[1] = c->dec.elapsed(c, 1, 2);
    if (herr != ~0ull)
        raise(MRG_EINVAL, "mrg_vocab_decode: the id at index %llu is not in the vocabulary (%llu words%s)",
              (unsigned long long)(herr - shift + lo0), (unsigned long long)v->n,
              unk_len ? "" : "; MRG_ID_UNK needs unk_len > 0");
    const uint64_t total = h_out_off[n_docs];
    c->dec.info[1] = total;
    if (!d_out) return;
    if (cap < total) raise(MRG_EINVAL, "destination too small (%llu bytes < %llu bytes of text)", (unsigned long long)cap,
                           (unsigned long long)total);
    P.out = d_out;
    P.out_n = total;
    c->dec.rec(c, 2);
    if (total) mrg_dec_launch_emit(P, v->T, v->W, s);
    c->dec.rec(c, 3);
    HIPCHK(hipGetLastError());
    sync(c);
    c->dec.ms[2] = c->dec.elapsed(c, 2, 3);
}

// Ids -> per-document term counts in CSR form (k_terms.hip): the documents are
// listed by path on the host; a count pass (LDS sort per document, radix sort per large slice) gives every
// row's length and UNK count, the scan the row offsets, an emit pass the rows.
void vocab_term_counts(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off, uint32_t n_docs,
                       uint32_t *d_terms, uint32_t *d_counts, uint64_t cap, uint64_t *h_row_off, uint64_t *h_unk) {
    voc_args(c, v, n_docs);
    if (!h_tok_off || !h_row_off) raise(MRG_EINVAL, "null offsets (h_tok_off and h_row_off need n_docs + 1 entries)");
    if ((uintptr_t)d_ids & 3u) raise(MRG_EINVAL, "the ids must be 4-byte aligned");
    if (!d_terms != !d_counts) raise(MRG_EINVAL, "d_terms and d_counts must both be given, or both be NULL (sizes only)");
    if (((uintptr_t)d_terms | (uintptr_t)d_counts) & 3u) raise(MRG_EINVAL, "d_terms and d_counts must be 4-byte aligned");
    voc_enter(c, h_tok_off, n_docs, "token offsets must be non-decreasing");
    // the documents by path (an empty document takes none: its row length stays 0)
    std::vector<uint32_t> list[3];
    for (uint32_t i = 0; i < n_docs; ++i) {
        const uint64_t T = h_tok_off[i + 1] - h_tok_off[i];
        if (T > 0xFFFFFFFFull)
            raise(MRG_EINVAL, "mrg_vocab_term_counts: document %u has %llu ids: at most 4294967295 (counts are 32 bits)", i,
                  (unsigned long long)T);
        if (T) list[T <= MRG_TERMS_WAVE_MAX ? 0 : T <= MRG_TERMS_WG_MAX ? 1 : 2].push_back(i);
    }
    c->terms.clear(5);
    const uint64_t n_ids = h_tok_off[n_docs] - h_tok_off[0];
    if (voc_empty(h_tok_off, n_docs, h_row_off)) {  // no ids: empty rows
        if (h_unk) std::fill(h_unk, h_unk + n_docs, 0);
        return;
    }
    if (!d_ids) raise(MRG_EINVAL, "null ids");
    // the large documents in slices: maximal runs of at most `budget` ids together, a longer document alone
    uint64_t budget = 1ull << 25;
    if (const char *e = getenv("MRG_TEST_TERMS_SLICE_IDS")) budget = std::max<long long>(1, atoll(e));
    struct Slice {
        uint32_t first, nd;  // list[2][first, first + nd)
        uint64_t m, soff_at; // ids; its nd + 1 offsets in `soff`
    };
    std::vector<Slice> slices;
    std::vector<uint64_t> soff;
    for (uint32_t x = 0; x < list[2].size(); ++x) {
        const uint64_t T = h_tok_off[list[2][x] + 1] - h_tok_off[list[2][x]];
        if (slices.empty() || slices.back().m + T > budget) {
            if (!slices.empty()) soff.push_back(slices.back().m);
            slices.push_back(Slice{x, 0, 0, soff.size()});
        }
        soff.push_back(slices.back().m);
        slices.back().m += T;
        slices.back().nd += 1;
    }
    if (!slices.empty()) soff.push_back(slices.back().m);
    for (const Slice &S : slices)
        if (S.m > 0xFFFFFFFFull) raise(MRG_EINVAL, "MRG_TEST_TERMS_SLICE_IDS: a slice of %llu ids", (unsigned long long)S.m);

    Pool &p = c->pool;
    hipStream_t s = c->stream;
    Scratch sc(p);
    c->terms.make(c);
    const uint64_t nl[3] = {list[0].size(), list[1].size(), list[2].size()};
    TermsPlan P{};
    P.in = d_ids;
    P.n_words = v->n;
    uint64_t *d_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    P.tok_off = d_off;
    P.len = sc.get<uint64_t>((uint64_t)n_docs + 1);
    P.unk = sc.get<uint64_t>(n_docs);
    uint32_t *d_list = sc.get<uint32_t>(nl[0] + nl[1] + nl[2]);
    const uint32_t *d_lp[3] = {d_list, d_list + nl[0], d_list + nl[0] + nl[1]};
    uint64_t *d_soff = sc.get<uint64_t>(soff.size());
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems((uint64_t)n_docs + 1));
    P.err = sc.get<unsigned long long>(1);
    uint64_t scratch = 8 * (3 * (uint64_t)n_docs + 2) + 4 * (nl[0] + nl[1] + nl[2]) + 8 * soff.size() +
                       8 * mrg_scan_tmp_elems((uint64_t)n_docs + 1) + 8, slice_max = 0;
    for (const Slice &S : slices)
        slice_max = std::max(slice_max, 16 * (S.m + 1) + mrg_sort_u64_keys_tmp_bytes(S.m) + 4 * mrg_scan_tmp_elems(S.m + 1));
    c->terms.info[0] = n_ids;
    for (int k = 0; k < 3; ++k) c->terms.info[3 + k] = nl[k];
    c->terms.info[6] = slices.size();
    c->terms.info[7] = scratch + slice_max;
    HIPCHK(hipMemcpyAsync(d_off, h_tok_off, 8 * ((uint64_t)n_docs + 1), hipMemcpyHostToDevice, s));
    for (int k = 0; k < 3; ++k)
        if (nl[k]) HIPCHK(hipMemcpyAsync((void *)d_lp[k], list[k].data(), 4 * nl[k], hipMemcpyHostToDevice, s));
    if (!soff.empty()) HIPCHK(hipMemcpyAsync(d_soff, soff.data(), 8 * soff.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.len, 0, 8 * ((uint64_t)n_docs + 1), s));
    HIPCHK(hipMemsetAsync(P.unk, 0, 8 * (uint64_t)n_docs, s));
    HIPCHK(hipMemsetAsync(P.err, 0xFF, 8, s));

    // One slice, sorted and run-flagged: K = the sorted keys, E = the scanned run starts, pos = room for
    // the run positions (E and pos lie in the key buffer the sort left free).
    struct Sorted {
        TermsSlice sl;
        const uint64_t *K;
        uint32_t *E, *pos;
    };
    auto sort_slice = [&](const Slice &S, Scratch &ss) {
        Sorted r{};
        r.sl = TermsSlice{d_lp[2] + S.first, d_soff + S.soff_at, S.nd, S.m};
        uint64_t *a = ss.get<uint64_t>(S.m + 1), *b = ss.get<uint64_t>(S.m + 1);
        void *sort_tmp = ss.get<uint8_t>(mrg_sort_u64_keys_tmp_bytes(S.m));
        uint32_t *scan_tmp = ss.get<uint32_t>(mrg_scan_tmp_elems(S.m + 1));
        mrg_terms_launch_keys(P, r.sl, a, s);
        // the key bytes that can differ: those of an id <= n_words, and of a rank < nd
        const uint32_t mask = ((1u << bytes_for(v->n)) - 1u) | (((1u << bytes_for((uint64_t)S.nd - 1u)) - 1u) << 4);
        uint64_t *K = mrg_radix_sort_u64_keys(a, b, S.m, mask, sort_tmp, s, nullptr);
        r.K = K;
        r.E = (uint32_t *)(K == a ? b : a);
        r.pos = r.E + S.m + 1;
        mrg_terms_launch_flags(K, S.m, v->n, r.E, s);
        mrg_scan_u32(r.E, r.E, S.m + 1, scan_tmp, s);
        HIPCHK(hipGetLastError());
        return r;
    };

    // ---- count: row lengths and UNKs of every document, then the row offsets
    c->terms.rec(c, 0);
    mrg_terms_launch_lds(P, d_lp[0], (uint32_t)nl[0], false, false, s);
    mrg_terms_launch_lds(P, d_lp[1], (uint32_t)nl[1], true, false, s);
    c->terms.rec(c, 1);
    Scratch kept(p);  // a single slice stays sorted for the emit pass
    Sorted one{};
    for (const Slice &S : slices) {
        Scratch ss(p);
        const Sorted r = sort_slice(S, ss);
        mrg_terms_launch_rows(P, r.sl, r.K, r.E, s);
        if (slices.size() == 1 && d_terms) {
            one = r;
            kept = std::move(ss);
        }
    }
    mrg_scan_u64(P.len, P.len, (uint64_t)n_docs + 1, stmp, s);
    c->terms.rec(c, 2);
    HIPCHK(hipGetLastError());
    unsigned long long herr = 0;
    std::vector<uint64_t> hu(n_docs);
    HIPCHK(hipMemcpyAsync(h_row_off, P.len, 8 * ((uint64_t)n_docs + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hu.data(), P.unk, 8 * (uint64_t)n_docs, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&herr, P.err, 8, hipMemcpyDeviceToHost, s));
    sync(c);  // (also: the pageable offsets and lists have been read)
    c->terms.ms[0] = c->terms.elapsed(c, 0, 1);
    c->terms.ms[1] = c->terms.elapsed(c, 1, 2);
    if (herr != ~0ull)
        raise(MRG_EINVAL, "mrg_vocab_term_counts: the id at index %llu is not in the vocabulary (%llu words)", herr,
              (unsigned long long)v->n);
    uint64_t n_unk = 0;
    for (uint32_t i = 0; i < n_docs; ++i) n_unk += hu[i];
    if (h_unk) memcpy(h_unk, hu.data(), 8 * (uint64_t)n_docs);
    const uint64_t total = h_row_off[n_docs];
    c->terms.info[1] = total;
    c->terms.info[2] = n_unk;
    if (!d_terms) return;
    if (cap < total) raise(MRG_EINVAL, "destination too small (%llu entries < %llu row entries)", (unsigned long long)cap,
                           (unsigned long long)total);
    // ---- emit
    P.terms = d_terms;
    P.counts = d_counts;
    c->terms.rec(c, 3);
    mrg_terms_launch_lds(P, d_lp[0], (uint32_t)nl[0], false, true, s);
    mrg_terms_launch_lds(P, d_lp[1], (uint32_t)nl[1], true, true, s);
    c->terms.rec(c, 4);
    for (const Slice &S : slices) {
        Scratch ss(p);
        const Sorted r = slices.size() == 1 ? one : sort_slice(S, ss);
        mrg_terms_launch_write(P, r.sl, r.K, r.E, r.pos, s);
    }
    c->terms.rec(c, 5);
    HIPCHK(hipGetLastError());
    sync(c);
    c->terms.ms[2] = c->terms.elapsed(c, 3, 4);
    c->terms.ms[3] = c->terms.elapsed(c, 4, 5);
}

// The CSR of mrg_vocab_term_counts -> the inverted index over ids (k_postings.hip):
// one pass over the terms checks them and counts the document frequencies into d_post_off, a scan turns
// them into the offsets; then (term, doc, tf) records are packed, sorted by the term's bytes with the
// stable LSD radix sort and unpacked.
void vocab_postings(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_terms, const uint32_t *d_counts,
                    const uint64_t *h_row_off, uint32_t n_docs, uint32_t doc_base, uint64_t *d_post_off, uint32_t *d_docs,
                    uint32_t *d_tf, uint64_t cap, uint64_t *h_entries) {
    voc_args(c, v, n_docs, true);
    if (!h_row_off) raise(MRG_EINVAL, "null offsets (h_row_off needs n_docs + 1 entries)");
    voc_enter(c, h_row_off, n_docs, "row offsets must be non-decreasing (row %u)");
    if ((uint64_t)doc_base + n_docs > (1ull << 32))
        raise(MRG_EINVAL, "doc_base + n_docs = %llu: documents are 32 bits", (unsigned long long)doc_base + n_docs);
    const uint64_t lo = h_row_off[0], E = h_row_off[n_docs] - lo;
    if (E > 0xFFFFFFFFull) raise(MRG_EINVAL, "mrg_vocab_postings: %llu entries: at most 4294967295", (unsigned long long)E);
    if (!d_post_off) raise(MRG_EINVAL, "null d_post_off (it receives the vocabulary's words + 1 offsets)");
    if (d_tf && !d_docs) raise(MRG_EINVAL, "d_tf without d_docs");
    if (d_tf && !d_counts) raise(MRG_EINVAL, "d_tf without d_counts");
    if (((uintptr_t)d_terms | (uintptr_t)d_counts | (uintptr_t)d_docs | (uintptr_t)d_tf) & 3u)
        raise(MRG_EINVAL, "d_terms, d_counts, d_docs and d_tf must be 4-byte aligned");
    if ((uintptr_t)d_post_off & 7u) raise(MRG_EINVAL, "d_post_off must be 8-byte aligned");
    if (d_docs && cap < E) raise(MRG_EINVAL, "destination too small (%llu entries < %llu postings)", (unsigned long long)cap,
                                 (unsigned long long)E);
    if (E && !d_terms) raise(MRG_EINVAL, "null terms");
    c->post.clear(5);
    const uint64_t n_words = v->n;
    c->post.info[0] = E;
    c->post.info[1] = n_words;
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(d_post_off, 0, 8 * (n_words + 1), s));
    if (E == 0) {  // no entries: all-zero offsets
        sync(c);
        if (h_entries) *h_entries = 0;
        return;
    }
    Pool &p = c->pool;
    Scratch sc(p);
    c->post.make(c);
    PostPlan P{};
    P.terms = d_terms;
    P.counts = d_tf ? d_counts : nullptr;
    P.n_docs = n_docs;
    P.doc_base = doc_base;
    P.lo = lo;
    P.hi = lo + E;
    P.n_words = n_words;
    P.df = (unsigned long long *)d_post_off;
    P.stat = sc.get<unsigned long long>(4);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(n_words + 1));
    uint64_t scratch = 32 + 8 * mrg_scan_tmp_elems(n_words + 1);
    HIPCHK(hipMemsetAsync(P.stat, 0xFF, 8, s));
    HIPCHK(hipMemsetAsync(P.stat + 1, 0, 24, s));
    // ---- count and validate, then the offsets
    c->post.rec(c, 0);
    mrg_post_launch_count(P, s);
    c->post.rec(c, 1);
    mrg_post_launch_max(P, s);
    mrg_scan_u64(d_post_off, d_post_off, n_words + 1, stmp, s);  // d_post_off[n_words] = E
    c->post.rec(c, 2);
    HIPCHK(hipGetLastError());
    unsigned long long hstat[4] = {};
    HIPCHK(hipMemcpyAsync(hstat, P.stat, sizeof hstat, hipMemcpyDeviceToHost, s));
    sync(c);
    c->post.ms[0] = c->post.elapsed(c, 0, 1);
    c->post.ms[1] = c->post.elapsed(c, 1, 2);
    c->post.info[6] = scratch;
    if (hstat[0] != ~0ull)
        raise(MRG_EINVAL, "mrg_vocab_postings: the term at index %llu is not in the vocabulary (%llu words)", hstat[0],
              (unsigned long long)n_words);
    c->post.info[2] = hstat[3];
    c->post.info[4] = hstat[1];
    c->post.info[5] = hstat[2];
    if (h_entries) *h_entries = E;
    if (!d_docs) return;
    // ---- pack, stable sort by the term's bytes, unpack
    uint64_t *d_off = sc.get<uint64_t>((uint64_t)n_docs + 1);
    PostRec *a = sc.get<PostRec>(E), *b = sc.get<PostRec>(E);
    void *sort_tmp = sc.get<uint8_t>(mrg_sort_post_tmp_bytes(E));
    c->post.info[6] = scratch + 8 * ((uint64_t)n_docs + 1) + 2 * sizeof(PostRec) * E + mrg_sort_post_tmp_bytes(E);
    P.row_off = d_off;
    HIPCHK(hipMemcpyAsync(d_off, h_row_off, 8 * ((uint64_t)n_docs + 1), hipMemcpyHostToDevice, s));
    c->post.rec(c, 2);
    mrg_post_launch_pack(P, a, s);
    c->post.rec(c, 3);
    int passes = 0;  // (the sort's byte mask: the bytes that n_words - 1 can set)
    const PostRec *r = mrg_radix_sort_post(a, b, E, (1u << bytes_for(n_words - 1)) - 1u, sort_tmp, s, &passes);
    c->post.rec(c, 4);
    mrg_post_launch_unpack(r, E, d_docs, d_tf, s);
    c->post.rec(c, 5);
    HIPCHK(hipGetLastError());
    sync(c);  // (also: the pageable offsets have been read)
    c->post.info[3] = (uint64_t)passes;
    c->post.ms[2] = c->post.elapsed(c, 2, 3);
    c->post.ms[3] = c->post.elapsed(c, 3, 4);
    c->post.ms[4] = c->post.elapsed(c, 4, 5);
}

// The inverted index of mrg_vocab_postings + a batch of queries -> the k best documents of every query by BM25
// (k_search.hip).  Plan: the offsets of every query position and the sum of the document
// lengths come back in one stream wait; the host validates, computes the idfs and cuts the segments into tiles.
// Then the queries go in chunks of dense score rows: one accumulate launch per query position, the radix select
// with the ordered compaction, the ordering of the candidates.
// cs (mrg_vocab_search_shard): the index is one shard of a collection; N, avgdl and every df are the collection's.
// roles (mrg_vocab_search_bool, _bool_shard): h_q_role of the call, MRG_Q_* per query id,
// indexed like h_q_off; `boolean` names the entry point.  With a role other than SHOULD in the call, every cell
// has a match state beside its score, the accumulate launches take the role-aware kernel, and the rows of the
// queries that have such a role are filtered before the select.  Without one the call is the plain search.
struct CollStats {
    const uint64_t *d_df;
    uint64_t docs, sum_len;
};
void vocab_search(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs, const uint32_t *d_tf,
                  uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs, uint32_t doc_base, const uint32_t *d_q_ids,
                  const uint64_t *h_q_off, uint32_t n_queries, float k1, float b, uint32_t k, uint32_t *d_top_docs,
                  float *d_top_scores, uint32_t *h_top_n, const CollStats *cs = nullptr, const uint8_t *roles = nullptr,
                  bool boolean = false) {
    const char *fn = boolean ? (cs ? "mrg_vocab_search_bool_shard" : "mrg_vocab_search_bool")
                             : (cs ? "mrg_vocab_search_shard" : "mrg_vocab_search");
    voc_args(c, v, n_queries);
    if (!d_post_off) raise(MRG_EINVAL, "null d_post_off (the vocabulary's words + 1 offsets of mrg_vocab_postings)");
    if (!h_q_off) raise(MRG_EINVAL, "null offsets (h_q_off needs n_queries + 1 entries)");
    if (!d_top_docs || !d_top_scores || !h_top_n)
        raise(MRG_EINVAL, "null output (d_top_docs and d_top_scores need n_queries * k entries, h_top_n n_queries)");
    if (n_entries && (!d_docs || !d_tf || !d_doc_len)) raise(MRG_EINVAL, "null d_docs, d_tf or d_doc_len with %llu entries",
                                                             (unsigned long long)n_entries);
    if (((uintptr_t)d_docs | (uintptr_t)d_tf | (uintptr_t)d_doc_len | (uintptr_t)d_q_ids | (uintptr_t)d_top_docs |
         (uintptr_t)d_top_scores) & 3u)
        raise(MRG_EINVAL, "d_docs, d_tf, d_doc_len, d_q_ids, d_top_docs and d_top_scores must be 4-byte aligned");
    if ((uintptr_t)d_post_off & 7u) raise(MRG_EINVAL, "d_post_off must be 8-byte aligned");
    if ((uint64_t)doc_base + n_docs > (1ull << 32))
        raise(MRG_EINVAL, "doc_base + n_docs = %llu: documents are 32 bits", (unsigned long long)doc_base + n_docs);
    if (n_entries > 0xFFFFFFFFull) raise(MRG_EINVAL, "%s: %llu entries: at most 4294967295", fn,
                                         (unsigned long long)n_entries);
    if (cs) {
        if (v->n && !cs->d_df) raise(MRG_EINVAL, "null d_df (the collection's document frequencies: mrg_vocab_stats_add)");
        if ((uintptr_t)cs->d_df & 7u) raise(MRG_EINVAL, "d_df must be 8-byte aligned");
        if (cs->docs < n_docs) raise(MRG_EINVAL, "coll_docs = %llu: the shard alone has %u documents",
                                     (unsigned long long)cs->docs, n_docs);
        if (cs->docs > (1ull << 32)) raise(MRG_EINVAL, "coll_docs = %llu: documents are 32 bits", (unsigned long long)cs->docs);
    }
    if (k < 1u || k > MRG_SEARCH_MAX_K) raise(MRG_EINVAL, "k = %u: 1 to %u", k, MRG_SEARCH_MAX_K);
    if (!(k1 >= 0.0f && k1 <= 1000.0f)) raise(MRG_EINVAL, "k1 = %g: 0 to 1000", (double)k1);
    if (!(b >= 0.0f && b <= 1.0f)) raise(MRG_EINVAL, "b = %g: 0 to 1", (double)b);
    voc_enter(c, h_q_off, n_queries, "query offsets must be non-decreasing (query %u)");
    const uint64_t qlo = h_q_off[0], n_ids = h_q_off[n_queries] - qlo;
    if (n_ids > (1ull << 20)) raise(MRG_EINVAL, "%s: %llu query ids in one call: at most 1048576", fn,
                                    (unsigned long long)n_ids);
    if (n_ids && !d_q_ids) raise(MRG_EINVAL, "null query ids");
    bool filtered = false;  // a role other than SHOULD in the call
    for (uint64_t i = qlo; roles && i < qlo + n_ids; ++i) {
        if (roles[i] > MRG_Q_MUST_NOT)
            raise(MRG_EINVAL, "%s: role at index %llu: %u is none of MRG_Q_SHOULD, MRG_Q_MUST, MRG_Q_MUST_NOT", fn,
                  (unsigned long long)i, (unsigned)roles[i]);
        filtered |= roles[i] != MRG_Q_SHOULD;
    }
    c->srch.clear(4);
    c->srch.info[0] = n_queries;
    c->srch.info[1] = n_ids;
    if (!n_ids) {  // no query positions: no hits
        std::fill(h_top_n, h_top_n + n_queries, 0u);
        return;
    }
    Pool &p = c->pool;
    hipStream_t s = c->stream;
    Scratch sc(p);
    c->srch.make(c);
    const uint64_t n_words = v->n;

    // ---- plan
    c->srch.rec(c, 4);
    uint64_t *d_po = sc.get<uint64_t>(2 * n_ids);
    unsigned long long *d_small = sc.get<unsigned long long>(2);  // the sum of the lengths, the error position
    HIPCHK(hipMemsetAsync(d_small, 0, 8, s));
    HIPCHK(hipMemsetAsync(d_small + 1, 0xFF, 8, s));
    uint64_t *d_dfo = cs ? sc.get<uint64_t>(n_ids) : nullptr;  // the collection's df of every query position
    mrg_search_launch_gather(d_q_ids + qlo, n_ids, d_post_off, n_words, d_po, s, cs ? cs->d_df : nullptr, d_dfo);
    if (n_entries && !cs) mrg_search_launch_sum(d_doc_len, n_docs, d_small, s);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> ids(n_ids);
    std::vector<uint64_t> po(2 * n_ids), dfc(cs ? n_ids : 0);
    unsigned long long sum_len = 0;
    if (cs) HIPCHK(hipMemcpyAsync(dfc.data(), d_dfo, 8 * n_ids, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ids.data(), d_q_ids + qlo, 4 * n_ids, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(po.data(), d_po, 16 * n_ids, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&sum_len, d_small, 8, hipMemcpyDeviceToHost, s));
    sync(c);
    for (uint64_t i = 0; i < n_ids; ++i)
        if (ids[i] != MRG_ID_UNK && ids[i] >= n_words)
            raise(MRG_EINVAL, "%s: the id at index %llu is not in the vocabulary (%llu words)", fn,
                  (unsigned long long)(qlo + i), (unsigned long long)n_words);
    for (uint64_t i = 0; i < n_ids; ++i)
        if (po[2 * i] > po[2 * i + 1] || po[2 * i + 1] > n_entries)
            raise(MRG_EINVAL, "%s: d_post_off of word %u: [%llu, %llu) is not a range of the %llu entries", fn, ids[i],
                  (unsigned long long)po[2 * i], (unsigned long long)po[2 * i + 1], (unsigned long long)n_entries);
    if (cs) {  // a word with postings here: the collection has at least the shard's documents of it, at most all
        sum_len = cs->sum_len;
        for (uint64_t i = 0; i < n_ids; ++i) {
            const uint64_t df = po[2 * i + 1] - po[2 * i];
            if (df && (dfc[i] < df || dfc[i] > cs->docs))
                raise(MRG_EINVAL, "%s: d_df of word %u: %llu, with %llu documents of it in this shard and %llu in the collection",
                      fn, ids[i], (unsigned long long)dfc[i], (unsigned long long)df, (unsigned long long)cs->docs);
        }
    }
    std::vector<uint32_t> top(n_queries, 0u);
    uint64_t visited = 0;
    for (uint64_t i = 0; i < n_ids; ++i) visited += po[2 * i + 1] - po[2 * i];
    c->srch.info[2] = visited;
    if (!visited || !n_docs) {  // no postings to visit: no hits
        c->srch.rec(c, 5);
        sync(c);
        c->srch.ms[0] = c->srch.elapsed(c, 4, 5);
        std::copy(top.begin(), top.end(), h_top_n);
        return;
    }
    // the chunks: as many queries as have their dense rows in MRG_SEARCH_ACC_BYTES (one at least; the row of a
    // query is a grid coordinate of the select: at most 65535)
    uint64_t acc_bytes = 256ull << 20;
    if (const char *e = getenv("MRG_SEARCH_ACC_BYTES")) acc_bytes = (uint64_t)std::max<long long>(1, atoll(e));
    SearchPlan P{};
    P.docs = d_docs;
    P.tf = d_tf;
    P.doc_len = d_doc_len;
    P.n_docs = n_docs;
    P.doc_base = doc_base;
    P.shift = (uint32_t)(((uintptr_t)d_docs >> 2) & 3u);
    P.tf_vec = (((uintptr_t)d_docs ^ (uintptr_t)d_tf) & 15u) == 0u;
    P.k1 = k1;
    P.k1p1 = k1 + 1.0f;
    P.b = b;
    const double n_coll = cs ? (double)cs->docs : (double)n_docs;  // N
    const double avgdl = (double)sum_len / n_coll;
    P.avgdl = avgdl > 0.0 ? (float)avgdl : 1.0f;  // (every length is 0: dl / avgdl counts as 0)
    P.err = d_small + 1;
    P.k = k;
    P.want = std::min(k, n_docs);
    P.stride = ((uint64_t)n_docs + 3u) & ~3ull;
    P.ntile = (uint32_t)((P.stride + MRG_SEARCH_SEL_TILE - 1u) / MRG_SEARCH_SEL_TILE);
    P.out_docs = d_top_docs;
    P.out_scores = d_top_scores;
    const uint64_t cell_bytes = filtered ? 8u : 4u;  // the score, and the match state of a Boolean search
    const uint32_t rows_max = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(n_queries, 65535u),
                                                           std::max<uint64_t>(1, acc_bytes / (cell_bytes * P.stride)));
    // the tiles, by (chunk, position, query): launch j of a chunk takes position j of its queries
    struct Launch {
        uint64_t first, n;  // tiles
    };
    std::vector<SearchTile> tiles;
    std::vector<Launch> launches;
    std::vector<uint32_t> chunk_launches;  // launches of every chunk
    // a Boolean search: what every position does (SRCH_TILE_* or 0; QUERY_DEAD: a query that cannot have a hit),
    // and by chunk the rows to filter
    constexpr uint32_t QUERY_DEAD = 1u;
    std::vector<uint32_t> mode(filtered ? n_ids : 0, 0u);
    std::vector<SearchFilterRow> frows;
    std::vector<uint32_t> chunk_frows;
    std::vector<std::pair<uint32_t, uint64_t>> must;  // (word, position) of the MUST positions of one query
    for (uint64_t q0 = 0; q0 < n_queries; q0 += rows_max) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(rows_max, n_queries - q0);
        uint32_t nf = 0;
        for (uint32_t r = 0; filtered && r < rows; ++r) {
            const uint64_t a = h_q_off[q0 + r] - qlo, e = h_q_off[q0 + r + 1] - qlo;
            must.clear();
            bool any = false, dead = false;
            for (uint64_t i = a; i < e; ++i) {
                const uint8_t role = roles[qlo + i];
                any |= role != MRG_Q_SHOULD;
                if (role == MRG_Q_MUST_NOT) mode[i] = SRCH_TILE_EXCLUDE;
                if (role != MRG_Q_MUST) continue;
                dead |= po[2 * i] == po[2 * i + 1];  // MRG_ID_UNK, or a word with no postings here
                must.emplace_back(ids[i], i);
            }
            if (dead) {  // no tiles: the row stays zero
                for (uint64_t i = a; i < e; ++i) mode[i] = QUERY_DEAD;
                continue;
            }
            if (!any) continue;
            std::sort(must.begin(), must.end());
            uint32_t need = 0;
            for (size_t m = 0; m < must.size(); ++m)
                if (!m || must[m].first != must[m - 1].first) {  // the first MUST position of the word counts
                    mode[must[m].second] = SRCH_TILE_COUNT;
                    ++need;
                }
            frows.push_back(SearchFilterRow{r, need});
            ++nf;
        }
        chunk_frows.push_back(nf);
        uint64_t longest = 0;
        for (uint32_t r = 0; r < rows; ++r) longest = std::max(longest, h_q_off[q0 + r + 1] - h_q_off[q0 + r]);
        uint32_t nl = 0;
        for (uint64_t j = 0; j < longest; ++j) {
            const uint64_t first = tiles.size();
            for (uint32_t r = 0; r < rows; ++r) {
                const uint64_t at = h_q_off[q0 + r] + j;
                if (at >= h_q_off[q0 + r + 1]) continue;
                const uint64_t a = po[2 * (at - qlo)], e = po[2 * (at - qlo) + 1], df = e - a;
                if (!df) continue;  // MRG_ID_UNK, or a word with no postings
                const uint32_t md = filtered ? mode[at - qlo] : 0u;
                if (md == QUERY_DEAD) continue;
                // (a df above N cannot ascend strictly inside the collection: the kernel reports it)
                double x = df <= n_docs ? ((double)n_docs - (double)df + 0.5) / ((double)df + 0.5) : 0.0;
                if (cs) {  // (checked above: the shard's df <= the collection's <= N)
                    const double dfn = (double)dfc[at - qlo];
                    x = (n_coll - dfn + 0.5) / (dfn + 0.5);
                }
                const float idf = (float)log(1.0 + x);
                for (uint64_t lo = a; lo < e;) {
                    const uint64_t hi = std::min(e, ((lo + P.shift) / MRG_SEARCH_TILE + 1u) * MRG_SEARCH_TILE - P.shift);
                    tiles.push_back(SearchTile{(uint32_t)lo, (uint32_t)hi, (uint32_t)a, r | md, idf});
                    lo = hi;
                }
            }
            if (tiles.size() > first) {
                launches.push_back(Launch{first, tiles.size() - first});
                ++nl;
            }
        }
        chunk_launches.push_back(nl);
    }
    if (filtered) {  // (the tiles of a query with an unsatisfiable MUST were dropped)
        visited = 0;
        for (const SearchTile &t : tiles) visited += t.hi - t.lo;
        c->srch.info[2] = visited;
    }
    SearchTile *d_tiles = sc.get<SearchTile>(tiles.size());
    P.top_n = sc.get<uint32_t>(n_queries);
    if (!tiles.empty())  // (none: every query of a Boolean search has an unsatisfiable MUST)
        HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(SearchTile) * tiles.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.top_n, 0, 4 * (uint64_t)n_queries, s));
    const uint64_t n_acc = (uint64_t)rows_max * P.stride, n_cnt = 2 * (uint64_t)rows_max * P.ntile;
    P.acc = sc.get<float>(n_acc);
    SearchFilterRow *d_frows = nullptr;
    if (filtered) {
        P.match = sc.get<uint32_t>(n_acc);
        if (!frows.empty()) {
            d_frows = sc.get<SearchFilterRow>(frows.size());
            HIPCHK(hipMemcpyAsync(d_frows, frows.data(), sizeof(SearchFilterRow) * frows.size(), hipMemcpyHostToDevice, s));
        }
    }
    P.hist = sc.get<uint32_t>(256 * (uint64_t)rows_max);
    P.sel = sc.get<uint32_t>(4 * (uint64_t)rows_max);
    P.cnt = sc.get<uint32_t>(n_cnt);
    P.cand_doc = sc.get<uint32_t>((uint64_t)rows_max * k);
    P.cand_bits = sc.get<uint32_t>((uint64_t)rows_max * k);
    c->srch.info[3] = chunk_launches.size();
    c->srch.info[4] = launches.size();
    c->srch.info[5] = 16 * n_ids + 16 + sizeof(SearchTile) * tiles.size() + 4 * (uint64_t)n_queries + 4 * n_acc +
                      (1024 + 16 + 8 * (uint64_t)k) * rows_max + 4 * n_cnt +
                      (filtered ? 4 * n_acc + sizeof(SearchFilterRow) * frows.size() : 0);
    HIPCHK(hipMemsetAsync(P.hist, 0, 1024 * (uint64_t)rows_max, s));
    c->srch.rec(c, 5);
    if (c->timing) c->srch.ms[0] = c->srch.elapsed(c, 4, 5);

    // ---- the chunks
    uint64_t li = 0, fi = 0;
    for (uint64_t q0 = 0, ch = 0; q0 < n_queries; q0 += rows_max, ++ch) {
        P.rows = (uint32_t)std::min<uint64_t>(rows_max, n_queries - q0);
        P.q0 = (uint32_t)q0;
        c->srch.rec(c, 0);
        HIPCHK(hipMemsetAsync(P.acc, 0, 4 * (uint64_t)P.rows * P.stride, s));
        if (filtered) HIPCHK(hipMemsetAsync(P.match, 0, 4 * (uint64_t)P.rows * P.stride, s));
        for (uint32_t j = 0; j < chunk_launches[ch]; ++j, ++li)
            (filtered ? mrg_search_launch_acc_bool : mrg_search_launch_acc)(P, d_tiles + launches[li].first, launches[li].n, s);
        c->srch.rec(c, 1);
        if (filtered) {
            mrg_search_launch_filter(P, d_frows + fi, chunk_frows[ch], s);
            fi += chunk_frows[ch];
        }
        mrg_search_launch_select(P, s);
        c->srch.rec(c, 2);
        mrg_search_launch_order(P, s);
        c->srch.rec(c, 3);
        HIPCHK(hipGetLastError());
        if (c->timing) {  // (the events are reused by the next chunk: read them now)
            c->srch.ms[1] += c->srch.elapsed(c, 0, 1);
            c->srch.ms[2] += c->srch.elapsed(c, 1, 2);
            c->srch.ms[3] += c->srch.elapsed(c, 2, 3);
        }
    }
    unsigned long long herr = 0;
    HIPCHK(hipMemcpyAsync(top.data(), P.top_n, 4 * (uint64_t)n_queries, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&herr, P.err, 8, hipMemcpyDeviceToHost, s));
    sync(c);  // (also: the pageable tiles have been read)
    if (herr != ~0ull)
        raise(MRG_EINVAL, "%s: posting %llu: its document is outside [doc_base, doc_base + n_docs), or not "
                          "above the document before it in its word's postings", fn, herr);
    std::copy(top.begin(), top.end(), h_top_n);
}

// One shard's part of the collection statistics (k_merge.hip): its document frequencies are
// added to d_df on the device, its documents and the sum of their lengths to the host totals.
void vocab_stats_add(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_doc_len, uint32_t n_docs,
                     uint64_t *d_df, uint64_t *h_coll) {
    voc_args(c, v, n_docs, true);
    if (!d_post_off) raise(MRG_EINVAL, "null d_post_off (the vocabulary's words + 1 offsets of mrg_vocab_postings)");
    if (!d_df) raise(MRG_EINVAL, "null d_df (the vocabulary's words uint64, zeroed before the first shard)");
    if (!h_coll) raise(MRG_EINVAL, "null h_coll (two uint64: the documents and the sum of their lengths)");
    if (n_docs && !d_doc_len) raise(MRG_EINVAL, "null d_doc_len with %u documents", n_docs);
    if (((uintptr_t)d_post_off | (uintptr_t)d_df) & 7u) raise(MRG_EINVAL, "d_post_off and d_df must be 8-byte aligned");
    if ((uintptr_t)d_doc_len & 3u) raise(MRG_EINVAL, "d_doc_len must be 4-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    if (!v->n && !n_docs) return;
    hipStream_t s = c->stream;
    Scratch sc(c->pool);
    unsigned long long *d_small = sc.get<unsigned long long>(2);  // the sum of the lengths, the error word
    HIPCHK(hipMemsetAsync(d_small, 0, 8, s));
    HIPCHK(hipMemsetAsync(d_small + 1, 0xFF, 8, s));
    if (v->n) mrg_stats_launch_df(d_post_off, v->n, (unsigned long long *)d_df, d_small + 1, s);
    mrg_search_launch_sum(d_doc_len, n_docs, d_small, s);
    HIPCHK(hipGetLastError());
    unsigned long long h[2] = {};
    HIPCHK(hipMemcpyAsync(h, d_small, sizeof h, hipMemcpyDeviceToHost, s));
    sync(c);
    if (h[1] != ~0ull) raise(MRG_EINVAL, "mrg_vocab_stats_add: d_post_off of word %llu: the offsets must be non-decreasing", h[1]);
    h_coll[0] += n_docs;
    h_coll[1] += h[0];
}

// The result rows of the shards of one collection -> the collection's rows (k_merge.hip).
void search_merge(mrg_ctx *c, uint32_t n_shards, uint32_t n_queries, uint32_t k_in, const uint32_t *d_in_docs,
                  const float *d_in_scores, const uint32_t *h_in_top_n, uint32_t k_out, uint32_t *d_top_docs,
                  float *d_top_scores, uint32_t *h_top_n) {
    if (!c) raise(MRG_EINVAL, "null context");
    if (!d_in_docs || !d_in_scores || !h_in_top_n)
        raise(MRG_EINVAL, "null input (d_in_docs and d_in_scores: n_shards * n_queries * k_in entries, h_in_top_n: n_shards * "
                          "n_queries)");
    if (!d_top_docs || !d_top_scores || !h_top_n)
        raise(MRG_EINVAL, "null output (d_top_docs and d_top_scores need n_queries * k_out entries, h_top_n n_queries)");
    if (((uintptr_t)d_in_docs | (uintptr_t)d_in_scores | (uintptr_t)d_top_docs | (uintptr_t)d_top_scores) & 3u)
        raise(MRG_EINVAL, "d_in_docs, d_in_scores, d_top_docs and d_top_scores must be 4-byte aligned");
    if (n_shards < 1u || n_shards > MRG_SEARCH_MAX_SHARDS)
        raise(MRG_EINVAL, "n_shards = %u: 1 to %u (more shards merge in stages)", n_shards, MRG_SEARCH_MAX_SHARDS);
    if (k_in < 1u || k_in > MRG_SEARCH_MAX_K) raise(MRG_EINVAL, "k_in = %u: 1 to %u", k_in, MRG_SEARCH_MAX_K);
    if (k_out < 1u || k_out > MRG_SEARCH_MAX_K) raise(MRG_EINVAL, "k_out = %u: 1 to %u", k_out, MRG_SEARCH_MAX_K);
    const uint64_t n_rows = (uint64_t)n_shards * n_queries;
    if (n_rows * k_in > 0xFFFFFFFFull)
        raise(MRG_EINVAL, "mrg_search_merge: %llu input entries: at most 4294967295", (unsigned long long)(n_rows * k_in));
    for (uint64_t r = 0; r < n_rows; ++r)
        if (h_in_top_n[r] > k_in)
            raise(MRG_EINVAL, "mrg_search_merge: h_in_top_n[%llu] = %u is above k_in = %u", (unsigned long long)r, h_in_top_n[r],
                  k_in);
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint32_t> top(n_queries, 0u);
    bool any = false;
    for (uint32_t q = 0; q < n_queries; ++q) {
        uint64_t sum = 0;
        for (uint32_t sh = 0; sh < n_shards; ++sh) sum += h_in_top_n[(uint64_t)sh * n_queries + q];
        top[q] = (uint32_t)std::min<uint64_t>(sum, k_out);
        any = any || sum;
    }
    if (any) {
        hipStream_t s = c->stream;
        Scratch sc(c->pool);
        MergePlan M{};
        uint32_t *d_n = sc.get<uint32_t>(n_rows);
        M.err = sc.get<unsigned long long>(1);
        HIPCHK(hipMemcpyAsync(d_n, h_in_top_n, 4 * n_rows, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(M.err, 0xFF, 8, s));
        M.in_docs = d_in_docs;
        M.in_bits = (const uint32_t *)d_in_scores;
        M.in_n = d_n;
        M.n_shards = n_shards;
        M.n_queries = n_queries;
        M.k_in = k_in;
        M.k_out = k_out;
        M.out_docs = d_top_docs;
        M.out_bits = (uint32_t *)d_top_scores;
        mrg_merge_launch(M, s);
        HIPCHK(hipGetLastError());
        unsigned long long herr = 0;
        HIPCHK(hipMemcpyAsync(&herr, M.err, 8, hipMemcpyDeviceToHost, s));
        sync(c);  // (also: the pageable counts have been read)
        if (herr != ~0ull)
            raise(MRG_EINVAL, "mrg_search_merge: entry %llu: its score is not positive or a NaN, or it does not stand after the "
                              "entry before it in its row (score descending, then document ascending)", herr);
    }
    std::copy(top.begin(), top.end(), h_top_n);
}

// The indexes of the shards of one collection -> the index of the whole (k_postings_merge.hip, DESIGN.md section
// 31): the shards' offsets are checked and summed per word, a scan gives the merged offsets; then every (shard,
// word) list gets its place in the output, the seams between the shards are checked, and the lists are copied.
void vocab_postings_merge(mrg_ctx *c, const mrg_vocab *v, uint32_t n_shards, const uint64_t *const *h_post_off,
                          const uint32_t *const *h_docs, const uint32_t *const *h_tf, const uint64_t *h_entries,
                          uint64_t *d_post_off, uint32_t *d_docs, uint32_t *d_tf, uint64_t cap, uint64_t *h_total) {
    const char *fn = "mrg_vocab_postings_merge";
    voc_args(c, v, 0);
    if (!h_post_off || !h_entries) raise(MRG_EINVAL, "null h_post_off or h_entries (n_shards entries each)");
    if (!d_post_off) raise(MRG_EINVAL, "null d_post_off (it receives the vocabulary's words + 1 offsets)");
    if (n_shards < 1u || n_shards > MRG_SEARCH_MAX_SHARDS)
        raise(MRG_EINVAL, "n_shards = %u: 1 to %u (more shards merge in stages)", n_shards, MRG_SEARCH_MAX_SHARDS);
    if (d_tf && !d_docs) raise(MRG_EINVAL, "d_tf without d_docs");
    if (d_tf && !h_tf) raise(MRG_EINVAL, "d_tf without h_tf");
    if (d_docs && !h_docs) raise(MRG_EINVAL, "d_docs without h_docs");
    if (((uintptr_t)d_docs | (uintptr_t)d_tf) & 3u) raise(MRG_EINVAL, "d_docs and d_tf must be 4-byte aligned");
    if ((uintptr_t)d_post_off & 7u) raise(MRG_EINVAL, "d_post_off must be 8-byte aligned");
    const uint64_t n_words = v->n;
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_shards; ++s) {
        if (!h_post_off[s]) raise(MRG_EINVAL, "%s: shard %u: null offsets (h_post_off[s]: the vocabulary's words + 1)", fn, s);
        if ((uintptr_t)h_post_off[s] & 7u) raise(MRG_EINVAL, "%s: shard %u: the offsets must be 8-byte aligned", fn, s);
        if (h_entries[s] > 0xFFFFFFFFull || (total += h_entries[s]) > 0xFFFFFFFFull)
            raise(MRG_EINVAL, "%s: more than 4294967295 entries in the shards up to shard %u", fn, s);
        if (!n_words && h_entries[s]) raise(MRG_EINVAL, "%s: shard %u: %llu entries of an empty vocabulary", fn, s,
                                            (unsigned long long)h_entries[s]);
        if (d_docs && h_entries[s] && !h_docs[s]) raise(MRG_EINVAL, "%s: shard %u: null documents with %llu entries", fn, s,
                                                        (unsigned long long)h_entries[s]);
        if (d_tf && h_entries[s] && !h_tf[s]) raise(MRG_EINVAL, "%s: shard %u: null term frequencies with %llu entries", fn,
                                                    s, (unsigned long long)h_entries[s]);
        if (((d_docs ? (uintptr_t)h_docs[s] : 0u) | (d_tf ? (uintptr_t)h_tf[s] : 0u)) & 3u)
            raise(MRG_EINVAL, "%s: shard %u: the documents and term frequencies must be 4-byte aligned", fn, s);
    }
    if (d_docs && cap < total) raise(MRG_EINVAL, "destination too small (%llu entries < %llu postings)", (unsigned long long)cap,
                                     (unsigned long long)total);
    // no output range may overlap an input range (the copy reads while others write)
    struct Range {
        uintptr_t a, e;
        const char *what;
    };
    const Range outs[3] = {{(uintptr_t)d_post_off, (uintptr_t)d_post_off + 8 * (n_words + 1), "d_post_off"},
                           {(uintptr_t)d_docs, (uintptr_t)d_docs + (d_docs ? 4 * total : 0), "d_docs"},
                           {(uintptr_t)d_tf, (uintptr_t)d_tf + (d_tf ? 4 * total : 0), "d_tf"}};
    for (uint32_t s = 0; s < n_shards; ++s) {
        const Range ins[3] = {{(uintptr_t)h_post_off[s], (uintptr_t)h_post_off[s] + 8 * (n_words + 1), "offsets"},
                              {d_docs ? (uintptr_t)h_docs[s] : 0u, (d_docs ? (uintptr_t)h_docs[s] + 4 * h_entries[s] : 0u), "documents"},
                              {d_tf ? (uintptr_t)h_tf[s] : 0u, (d_tf ? (uintptr_t)h_tf[s] + 4 * h_entries[s] : 0u), "term frequencies"}};
        for (const Range &o : outs)
            for (const Range &i : ins)
                if (o.a < o.e && i.a < i.e && o.a < i.e && i.a < o.e)
                    raise(MRG_EINVAL, "%s: %s overlaps the %s of shard %u", fn, o.what, i.what, s);
    }
    HIPCHK(hipSetDevice(c->device));
    c->pmrg.clear(3);
    c->pmrg.info[0] = total;
    c->pmrg.info[1] = n_words;
    c->pmrg.info[2] = n_shards;
    hipStream_t s = c->stream;
    Scratch sc(c->pool);
    c->pmrg.make(c);
    std::vector<PMergeShard> tab(n_shards);
    PMergePlan P{};
    for (uint32_t i = 0; i < n_shards; ++i) {
        tab[i] = PMergeShard{h_post_off[i], d_docs && h_entries[i] ? h_docs[i] : nullptr,
                             d_tf && h_entries[i] ? h_tf[i] : nullptr, h_entries[i], P.n_tiles};
        P.n_tiles += (h_entries[i] + MRG_PMERGE_TILE - 1u) / MRG_PMERGE_TILE;
    }
    PMergeShard *d_tab = sc.get<PMergeShard>(n_shards);
    P.sh = d_tab;
    P.n_shards = n_shards;
    P.n_words = n_words;
    P.post_off = d_post_off;
    P.stat = sc.get<unsigned long long>(2);
    uint64_t *stmp = sc.get<uint64_t>(mrg_scan_tmp_elems(n_words + 1));
    uint64_t scratch = sizeof(PMergeShard) * n_shards + 16 + 8 * mrg_scan_tmp_elems(n_words + 1);
    c->pmrg.info[5] = scratch;
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(PMergeShard) * n_shards, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.stat, 0xFF, 8, s));
    HIPCHK(hipMemsetAsync(P.stat + 1, 0, 8, s));
    // ---- check and sum the offsets, then the merged offsets
    c->pmrg.rec(c, 0);
    mrg_pmerge_launch_sum(P, s);
    mrg_scan_u64(d_post_off, d_post_off, n_words + 1, stmp, s);  // d_post_off[n_words] = total
    c->pmrg.rec(c, 1);
    HIPCHK(hipGetLastError());
    unsigned long long hstat[2] = {};
    HIPCHK(hipMemcpyAsync(hstat, P.stat, 8, hipMemcpyDeviceToHost, s));
    sync(c);  // (also: the pageable table has been read)
    c->pmrg.ms[0] = c->pmrg.elapsed(c, 0, 1);
    if (hstat[0] != ~0ull)
        raise(MRG_EINVAL, "%s: shard %llu word %llu: the offsets of a shard must start at 0, not decrease, and end at its "
                          "h_entries", fn, hstat[0] & 63u, hstat[0] >> 6);
    if (h_total) *h_total = total;
    if (!d_docs || !total) return;
    // ---- the place of every (shard, word) list with the seams, then the copy
    P.docs = d_docs;
    P.tf = d_tf;
    P.dst = sc.get<uint32_t>((uint64_t)n_shards * n_words);
    c->pmrg.info[3] = P.n_tiles;
    c->pmrg.info[5] = scratch + 4 * (uint64_t)n_shards * n_words;
    c->pmrg.rec(c, 2);
    mrg_pmerge_launch_place(P, s);
    c->pmrg.rec(c, 3);
    mrg_pmerge_launch_copy(P, s);
    c->pmrg.rec(c, 4);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hstat, P.stat, sizeof hstat, hipMemcpyDeviceToHost, s));
    sync(c);
    c->pmrg.ms[1] = c->pmrg.elapsed(c, 2, 3);
    c->pmrg.ms[2] = c->pmrg.elapsed(c, 3, 4);
    c->pmrg.info[4] = hstat[1];
    if (hstat[0] != ~0ull)
        raise(MRG_EINVAL, "%s: shard %llu word %llu: the shard's first document of the word is not above the last document "
                          "of the word in the shards before it", fn, hstat[0] & 63u, hstat[0] >> 6);
}

// one of the mrg_*_info entry points: all of the record's info, the first n_ms of its milliseconds
int voc_info(mrg_ctx *c, VocDiag mrg_ctx::*diag, int n_ms, uint64_t *h_info, double *h_ms) {
    return guard([&] {
        if (!c) raise(MRG_EINVAL, "null context");
        const VocDiag &d = c->*diag;
        if (h_info) memcpy(h_info, d.info, sizeof d.info);
        if (h_ms) memcpy(h_ms, d.ms, sizeof(double) * n_ms);
    });
}

}  // namespace

extern "C" {

int mrg_job_vocab(mrg_ctx *c, uint64_t max_words, uint64_t min_count, mrg_vocab **out) {
    if (out) *out = nullptr;
    return guard([&] {
        if (!out) raise(MRG_EINVAL, "null out");
        *out = job_vocab(c, max_words, min_count);
    });
}

int mrg_vocab_size(const mrg_vocab *v, uint64_t *n_words, uint64_t *text_bytes) {
    return guard([&] {
        if (!v) raise(MRG_EINVAL, "null vocabulary");
        if (n_words) *n_words = v->n;
        if (text_bytes) *text_bytes = v->text_bytes;
    });
}

int mrg_vocab_copy_text(const mrg_vocab *v, uint8_t *h_dst, uint64_t cap) {
    return guard([&] {
        if (!v) raise(MRG_EINVAL, "null vocabulary");
        if (cap < v->text_bytes) raise(MRG_EINVAL, "destination too small (%llu < %llu)", (unsigned long long)cap,
                                       (unsigned long long)v->text_bytes);
        if (!v->text_bytes) return;
        if (!h_dst) raise(MRG_EINVAL, "null argument");
        HIPCHK(hipSetDevice(v->device));
        HIPCHK(hipMemcpy(h_dst, v->T.text, v->text_bytes, hipMemcpyDeviceToHost));
    });
}

void mrg_vocab_free(mrg_vocab *v) { vocab_destroy(v); }

int mrg_vocab_encode(mrg_ctx *c, const mrg_vocab *v, const uint8_t *d_bytes, const uint64_t *h_doc_off, uint32_t n_docs,
                     uint32_t *d_ids, uint64_t cap_ids, uint64_t *h_tok_off) {
    return guard([&] { vocab_encode(c, v, d_bytes, h_doc_off, n_docs, d_ids, cap_ids, h_tok_off); });
}

int mrg_vocab_from_text(mrg_ctx *c, const uint8_t *h_text, uint64_t bytes, uint32_t flags, mrg_vocab **out) {
    return guard([&] {
        if (!out) raise(MRG_EINVAL, "null out pointer");
        *out = nullptr;
        *out = vocab_from_text(c, h_text, bytes, flags);
    });
}

int mrg_vocab_decode(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off, uint32_t n_docs,
                     const uint8_t *h_unk, uint32_t unk_len, uint8_t *d_out, uint64_t cap, uint64_t *h_out_off) {
    return guard([&] { vocab_decode(c, v, d_ids, h_tok_off, n_docs, h_unk, unk_len, d_out, cap, h_out_off); });
}

int mrg_vocab_term_counts(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_ids, const uint64_t *h_tok_off,
                          uint32_t n_docs, uint32_t *d_terms, uint32_t *d_counts, uint64_t cap, uint64_t *h_row_off,
                          uint64_t *h_unk) {
    return guard([&] { vocab_term_counts(c, v, d_ids, h_tok_off, n_docs, d_terms, d_counts, cap, h_row_off, h_unk); });
}

// Diagnostics of the last mrg_vocab_term_counts (not in include/mrgpu.h; tools/time_terms.py): h_info[0..8) =
// ids, row entries, UNK ids, documents of the wave, workgroup and large path, large-path slices, scratch
// bytes; h_ms[0..4) = the LDS paths' count pass, the large path's count pass with the row scan, the LDS
// paths' emit pass, the large path's emit pass (HIP events, with mrg_set_timing).
int mrg_terms_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::terms, 4, h_info, h_ms); }

int mrg_vocab_postings(mrg_ctx *c, const mrg_vocab *v, const uint32_t *d_terms, const uint32_t *d_counts,
                       const uint64_t *h_row_off, uint32_t n_docs, uint32_t doc_base, uint64_t *d_post_off, uint32_t *d_docs,
                       uint32_t *d_tf, uint64_t cap, uint64_t *h_entries) {
    return guard([&] {
        vocab_postings(c, v, d_terms, d_counts, h_row_off, n_docs, doc_base, d_post_off, d_docs, d_tf, cap, h_entries);
    });
}

// Diagnostics of the last mrg_vocab_postings (not in include/mrgpu.h; tools/time_postings.py): h_info[0..7) =
// entries, words, the largest document frequency, radix passes run, entries counted in LDS, entries counted
// with global atomics, scratch bytes; h_ms[0..5) = count, scan (with the largest df), pack, sort, unpack
// (HIP events, with mrg_set_timing).
int mrg_postings_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::post, 5, h_info, h_ms); }

int mrg_vocab_search(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs, const uint32_t *d_tf,
                     uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs, uint32_t doc_base,
                     const uint32_t *d_q_ids, const uint64_t *h_q_off, uint32_t n_queries, float k1, float b, uint32_t k,
                     uint32_t *d_top_docs, float *d_top_scores, uint32_t *h_top_n) {
    return guard([&] {
        vocab_search(c, v, d_post_off, d_docs, d_tf, n_entries, d_doc_len, n_docs, doc_base, d_q_ids, h_q_off, n_queries, k1, b,
                     k, d_top_docs, d_top_scores, h_top_n);
    });
}

int mrg_vocab_search_bool(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                          const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                          uint32_t doc_base, const uint32_t *d_q_ids, const uint8_t *h_q_role, const uint64_t *h_q_off,
                          uint32_t n_queries, float k1, float b, uint32_t k, uint32_t *d_top_docs, float *d_top_scores,
                          uint32_t *h_top_n) {
    return guard([&] {
        vocab_search(c, v, d_post_off, d_docs, d_tf, n_entries, d_doc_len, n_docs, doc_base, d_q_ids, h_q_off, n_queries, k1, b,
                     k, d_top_docs, d_top_scores, h_top_n, nullptr, h_q_role, true);
    });
}

int mrg_vocab_stats_add(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_doc_len, uint32_t n_docs,
                        uint64_t *d_df, uint64_t *h_coll) {
    return guard([&] { vocab_stats_add(c, v, d_post_off, d_doc_len, n_docs, d_df, h_coll); });
}

int mrg_vocab_search_shard(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                           const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                           uint32_t doc_base, const uint64_t *d_df, uint64_t coll_docs, uint64_t coll_sum_len,
                           const uint32_t *d_q_ids, const uint64_t *h_q_off, uint32_t n_queries, float k1, float b, uint32_t k,
                           uint32_t *d_top_docs, float *d_top_scores, uint32_t *h_top_n) {
    return guard([&] {
        const CollStats cs{d_df, coll_docs, coll_sum_len};
        vocab_search(c, v, d_post_off, d_docs, d_tf, n_entries, d_doc_len, n_docs, doc_base, d_q_ids, h_q_off, n_queries, k1, b,
                     k, d_top_docs, d_top_scores, h_top_n, &cs);
    });
}

int mrg_vocab_search_bool_shard(mrg_ctx *c, const mrg_vocab *v, const uint64_t *d_post_off, const uint32_t *d_docs,
                                const uint32_t *d_tf, uint64_t n_entries, const uint32_t *d_doc_len, uint32_t n_docs,
                                uint32_t doc_base, const uint64_t *d_df, uint64_t coll_docs, uint64_t coll_sum_len,
                                const uint32_t *d_q_ids, const uint8_t *h_q_role, const uint64_t *h_q_off, uint32_t n_queries,
                                float k1, float b, uint32_t k, uint32_t *d_top_docs, float *d_top_scores, uint32_t *h_top_n) {
    return guard([&] {
        const CollStats cs{d_df, coll_docs, coll_sum_len};
        vocab_search(c, v, d_post_off, d_docs, d_tf, n_entries, d_doc_len, n_docs, doc_base, d_q_ids, h_q_off, n_queries, k1, b,
                     k, d_top_docs, d_top_scores, h_top_n, &cs, h_q_role, true);
    });
}

int mrg_search_merge(mrg_ctx *c, uint32_t n_shards, uint32_t n_queries, uint32_t k_in, const uint32_t *d_in_docs,
                     const float *d_in_scores, const uint32_t *h_in_top_n, uint32_t k_out, uint32_t *d_top_docs,
                     float *d_top_scores, uint32_t *h_top_n) {
    return guard([&] {
        search_merge(c, n_shards, n_queries, k_in, d_in_docs, d_in_scores, h_in_top_n, k_out, d_top_docs, d_top_scores, h_top_n);
    });
}

int mrg_vocab_postings_merge(mrg_ctx *c, const mrg_vocab *v, uint32_t n_shards, const uint64_t *const *h_post_off,
                             const uint32_t *const *h_docs, const uint32_t *const *h_tf, const uint64_t *h_entries,
                             uint64_t *d_post_off, uint32_t *d_docs, uint32_t *d_tf, uint64_t cap, uint64_t *h_total) {
    return guard([&] {
        vocab_postings_merge(c, v, n_shards, h_post_off, h_docs, h_tf, h_entries, d_post_off, d_docs, d_tf, cap, h_total);
    });
}

// Diagnostics of the last mrg_vocab_postings_merge (not in include/mrgpu.h; tools/time_postings_merge.py):
// h_info[0..6) = entries, words, shards, copy tiles, copy tiles inside one word, scratch bytes; h_ms[0..3) = sum
// with the scan, place (with the seams), copy (HIP events, with mrg_set_timing).
int mrg_postings_merge_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::pmrg, 3, h_info, h_ms); }

// Diagnostics of the last mrg_vocab_search, _search_shard, _search_bool or _search_bool_shard (not in include/mrgpu.h;
// tools/time_search.py, tools/time_search_shards.py, tools/time_search_bool.py): h_info[0..6) =
// queries, query positions, postings visited, chunks, accumulate launches, scratch bytes (with the match states of
// a Boolean search); h_ms[0..4) = plan, accumulate, select (with the filter and the compaction), order, summed over
// the chunks (HIP events, with mrg_set_timing).
int mrg_search_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::srch, 4, h_info, h_ms); }

// Diagnostics of the last mrg_vocab_decode (not in include/mrgpu.h; tools/time_decode.py): h_info[0..4) =
// ids, output bytes, chunks, scratch bytes; h_ms[0..4) = count pass, scan + document offsets, emit pass,
// and the last mrg_vocab_from_text (HIP events, with mrg_set_timing).
int mrg_decode_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::dec, 4, h_info, h_ms); }

// Diagnostics of the last mrg_vocab_encode (not in include/mrgpu.h; tools/time_encode.py): h_info[0..7) =
// tokens, UNK tokens, long tokens, non-ASCII 1 KiB chunks, table probes, input bytes, scratch bytes;
// h_ms[0..4) = count pass, scan + document offsets, emit pass, and the last mrg_job_vocab (HIP events,
// with mrg_set_timing).
int mrg_encode_info(mrg_ctx *c, uint64_t *h_info, double *h_ms) { return voc_info(c, &mrg_ctx::enc, 4, h_info, h_ms); }

}  // extern "C"
