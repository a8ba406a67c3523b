// k_search.hip -- BM25 top-k over the inverted index of mrg_vocab_postings, for a batch of queries (gfx950;
// DESIGN.md sections 24 and 34).
//
// mrg_vocab_search: plan -> accumulate -> select -> order, the queries in chunks of dense score rows.
//   plan        k_srch_gather reads post_off[t], post_off[t + 1] of every query position, k_srch_sum adds the
//               document lengths (integers: exact); the host layer validates, computes every idf in double and
//               cuts each (query, position) segment of postings into tiles: the parts of the segment that fall
//               into one window of MRG_SEARCH_TILE postings, the windows laid so that they start 16-byte aligned.
//   accumulate  k_srch_acc, one launch per query position, one workgroup per tile: 16-byte loads of docs and
//               tf, a gather of the document lengths, acc[row][doc - doc_base] += w.  A word's documents ascend
//               strictly, so within one launch a cell receives at most one posting: a plain read-modify-write,
//               every cell summed in query order.  Every posting is checked first -- its document lies in the
//               collection and is above its predecessor's in the segment -- and a posting that fails is
//               reported (atomicMin of its position) and not applied: nothing is written outside the row.
//   select      positive floats order as their bit patterns: a radix select over the score bits of every row,
//               most significant byte first (k_srch_hist + k_srch_pick, 4 passes), gives the bits of the k-th
//               largest score, the number of scores above it and the number of ties wanted.  Then the ordered
//               compaction: k_srch_count (documents above / at the threshold per tile of MRG_SEARCH_SEL_TILE),
//               k_srch_scan (per row), k_srch_take (everything above, the first `need` ties by document).
//   order       k_srch_order, one workgroup per query: the <= 1024 candidates ranked in LDS by (score
//               descending, document ascending) and written to the output rows, top_n entries and no more.
// mrg_vocab_search_bool: a call with a MUST or MUST_NOT position keeps a match state per
// cell beside the score.  Its accumulate launches take k_srch_acc<true>, which also counts the distinct MUST words
// that hold the document and marks the documents of MUST_NOT words; k_srch_filter then zeroes the cells of the
// queries' rows whose state is not the query's number of distinct MUST words.  The select sees rows of hits only.
// Every other call launches k_srch_acc<false>, the kernel without any of this.
// No kernel waits for another workgroup.  The only atomics add integers or take a minimum: no result depends
// on scheduling.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int SRCH_WG = 256;
constexpr int SRCH_ROUNDS = MRG_SEARCH_TILE / (4 * SRCH_WG);
static_assert(MRG_SEARCH_TILE % (4 * SRCH_WG) == 0 && SRCH_ROUNDS >= 1, "whole rounds of 16-byte loads per tile");
static_assert(MRG_SEARCH_SEL_TILE == 4 * SRCH_WG, "one 16-byte load per thread and select tile");
static_assert(MRG_SEARCH_SEL_TILE < (1u << 16), "two tile counts packed in 32 bits");
static_assert(MRG_SEARCH_MAX_K * 8u <= 64u * 1024u, "the candidates of a query fit the LDS of k_srch_order");

int srch_cus() {
    static int cus[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int cu = (dev >= 0 && dev < 64) ? cus[dev] : 0;
    if (cu == 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        if (dev >= 0 && dev < 64) cus[dev] = cu;
    }
    return cu;
}

// ---------------------------------------------------------------- plan

__global__ __launch_bounds__(SRCH_WG) void k_srch_gather(const uint32_t *q_ids, uint64_t n_ids, const uint64_t *post_off,
                                                        uint64_t n_words, uint64_t *po, const uint64_t *df, uint64_t *dfo) {
    const uint64_t i = (uint64_t)blockIdx.x * SRCH_WG + threadIdx.x;
    if (i >= n_ids) return;
    const uint32_t t = q_ids[i];
    const bool ok = (uint64_t)t < n_words;  // (post_off has n_words + 1 entries)
    po[2 * i] = ok ? post_off[t] : 0ull;
    po[2 * i + 1] = ok ? post_off[(uint64_t)t + 1u] : 0ull;
    if (df) dfo[i] = ok ? df[t] : 0ull;  // (a sharded search: the collection's document frequency)
}

__global__ __launch_bounds__(SRCH_WG) void k_srch_sum(const uint32_t *doc_len, uint32_t n_docs, unsigned long long *sum) {
    unsigned long long a = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * SRCH_WG + threadIdx.x; i < n_docs; i += (uint64_t)gridDim.x * SRCH_WG)
        a += doc_len[i];
    a = mrg_wave_sum_lane0(a);
    if (__lane_id() == 0 && a) atomicAdd(sum, a);
}

// ---------------------------------------------------------------- accumulate

// One posting, standing at position p of docs: checked, then added to its cell.  `prev` is the document of
// position p - 1 when that belongs to the same segment (has_prev).  BOOL (a Boolean search, DESIGN.md section
// 34): `mode` is the tile's SRCH_TILE_* bits, uniform in the workgroup; the match state of the cell is updated
// like the score, with a plain read-modify-write or a plain store, and whatever the posting's tf.
template <bool BOOL>
__device__ __forceinline__ void srch_one(const SearchPlan &A, float *row, uint32_t *match, uint32_t mode, float idf,
                                         uint32_t doc, uint32_t tf, uint32_t prev, bool has_prev, uint64_t p) {
    const uint32_t idx = doc - A.doc_base;
    if (idx >= A.n_docs || (has_prev && prev >= doc)) {
        atomicMin(A.err, (unsigned long long)p);
        return;
    }
    if (BOOL) {
        if (mode & SRCH_TILE_EXCLUDE) {  // (a count that is lost under the store belonged to an excluded cell)
            match[idx] = SRCH_EXCLUDED;
            return;
        }
        if (mode & SRCH_TILE_COUNT) match[idx] += 1u;
    }
    if (!tf) return;  // w = 0
    const float tff = (float)tf, dl = (float)A.doc_len[idx];
    const float w = idf * (tff * A.k1p1) / (tff + A.k1 * ((1.0f - A.b) + A.b * (dl / A.avgdl)));
    row[idx] += w;
}

template <bool BOOL>
__global__ __launch_bounds__(SRCH_WG) void k_srch_acc(SearchPlan A, const SearchTile *tiles) {
    const SearchTile T = tiles[blockIdx.x];
    const uint32_t trow = BOOL ? T.row & SRCH_TILE_ROW : T.row, mode = BOOL ? T.row & ~SRCH_TILE_ROW : 0u;
    float *row = A.acc + (uint64_t)trow * A.stride;
    uint32_t *match = BOOL ? A.match + (uint64_t)trow * A.stride : nullptr;
    const bool want_tf = !(mode & SRCH_TILE_EXCLUDE);  // (a MUST_NOT tile reads the documents only)
    const int64_t lo = T.lo, hi = T.hi, seg = T.seg_lo;
    // the window of the tile starts at a 16-byte boundary of docs; it may start below the tile
    const int64_t wbase = (int64_t)(((uint64_t)T.lo + A.shift) / MRG_SEARCH_TILE * MRG_SEARCH_TILE) - (int64_t)A.shift;
    for (int r = 0; r < SRCH_ROUNDS; ++r) {
        const int64_t p0 = wbase + 4 * (int64_t)(r * SRCH_WG + (int)threadIdx.x);
        if (p0 + 4 <= lo || p0 >= hi) continue;
        if (p0 >= lo && p0 + 4 <= hi) {  // four postings of the tile, 16-byte aligned in docs
            const uint4 d = *reinterpret_cast<const uint4 *>(A.docs + p0);
            uint4 f = make_uint4(0u, 0u, 0u, 0u);
            if (want_tf && A.tf_vec) f = *reinterpret_cast<const uint4 *>(A.tf + p0);
            else if (want_tf) f = make_uint4(A.tf[p0], A.tf[p0 + 1], A.tf[p0 + 2], A.tf[p0 + 3]);
            const bool hp = p0 > seg;
            const uint32_t prev = hp ? A.docs[p0 - 1] : 0u;
            srch_one<BOOL>(A, row, match, mode, T.idf, d.x, f.x, prev, hp, (uint64_t)p0);
            srch_one<BOOL>(A, row, match, mode, T.idf, d.y, f.y, d.x, true, (uint64_t)p0 + 1u);
            srch_one<BOOL>(A, row, match, mode, T.idf, d.z, f.z, d.y, true, (uint64_t)p0 + 2u);
            srch_one<BOOL>(A, row, match, mode, T.idf, d.w, f.w, d.z, true, (uint64_t)p0 + 3u);
        } else {  // the tile's first or last few postings, one by one
            for (int e = 0; e < 4; ++e) {
                const int64_t p = p0 + e;
                if (p < lo || p >= hi) continue;
                const bool hp = p > seg;
                srch_one<BOOL>(A, row, match, mode, T.idf, A.docs[p], want_tf ? A.tf[p] : 0u, hp ? A.docs[p - 1] : 0u, hp,
                               (uint64_t)p);
            }
        }
    }
}

// ---------------------------------------------------------------- filter

// A Boolean search, before the select: a cell keeps its score when its match state equals the distinct MUST
// words of its query, and becomes 0 -- no hit -- otherwise.  One row of `rows` per blockIdx.y; 16-byte loads
// of the scores, and of the match states only where one of the four scores is set (most of a row is not).
// The cells of the stride beyond n_docs are never written by the accumulate, and stay 0 here.
__global__ __launch_bounds__(SRCH_WG) void k_srch_filter(SearchPlan A, const SearchFilterRow *rows) {
    const SearchFilterRow R = rows[blockIdx.y];
    uint4 *v = reinterpret_cast<uint4 *>(A.acc + (uint64_t)R.row * A.stride);
    const uint4 *m = reinterpret_cast<const uint4 *>(A.match + (uint64_t)R.row * A.stride);
    const uint64_t nvec = A.stride >> 2;
    for (uint64_t i = (uint64_t)blockIdx.x * SRCH_WG + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * SRCH_WG) {
        uint4 q = v[i];
        if (!(q.x | q.y | q.z | q.w)) continue;
        const uint4 c = m[i];
        const bool drop = (q.x && c.x != R.need) || (q.y && c.y != R.need) || (q.z && c.z != R.need) || (q.w && c.w != R.need);
        if (!drop) continue;
        if (c.x != R.need) q.x = 0u;
        if (c.y != R.need) q.y = 0u;
        if (c.z != R.need) q.z = 0u;
        if (c.w != R.need) q.w = 0u;
        v[i] = q;
    }
}

// ---------------------------------------------------------------- select

// One pass of the radix select: the histogram of byte d (0: the most significant) of the score bits, among the
// scores of the row that match the prefix on the bytes above it.  Zero scores -- most of a row -- are counted in
// a register, not in LDS.
__global__ __launch_bounds__(SRCH_WG) void k_srch_hist(SearchPlan A, uint32_t d) {
    __shared__ uint32_t h[256];
    const uint32_t row = blockIdx.y, tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const uint32_t prefix = d ? A.sel[4u * row] : 0u, mask = d ? ~0u << (32u - 8u * d) : 0u, sh = 24u - 8u * d;
    const bool zero_in = (prefix & mask) == 0u;
    const uint4 *v = reinterpret_cast<const uint4 *>(A.acc + (uint64_t)row * A.stride);
    const uint64_t nvec = A.stride >> 2;
    uint32_t nz = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * SRCH_WG + tid; i < nvec; i += (uint64_t)gridDim.x * SRCH_WG) {
        const uint4 q = v[i];
        const uint32_t x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4u * i + (uint64_t)j >= A.n_docs) continue;
            if (x[j] == 0u) nz += zero_in ? 1u : 0u;
            else if (((x[j] ^ prefix) & mask) == 0u) atomicAdd(&h[(x[j] >> sh) & 0xFFu], 1u);
        }
    }
    nz = mrg_wave_sum_lane0(nz);
    if (__lane_id() == 0 && nz) atomicAdd(&h[0], nz);
    __syncthreads();
    const uint32_t c = h[tid];
    if (c) atomicAdd(&A.hist[256u * row + tid], c);
}

// The bin that holds the wanted rank, counted from the top, becomes the next byte of the prefix.
// sel[4 row ..] = prefix, the rank still wanted among the scores on the prefix, the scores above the prefix,
// and after the last pass top_n = those above + the ties wanted (none at a threshold of 0: not a hit).
__global__ __launch_bounds__(256) void k_srch_pick(SearchPlan A, uint32_t d) {
    __shared__ uint32_t sc[256];
    const uint32_t row = blockIdx.x, t = threadIdx.x;
    uint32_t *sel = A.sel + 4u * row;
    const uint32_t prefix = d ? sel[0] : 0u, want = d ? sel[1] : A.want, gt = d ? sel[2] : 0u;
    const uint32_t mine = A.hist[256u * row + t];
    A.hist[256u * row + t] = 0u;  // for the next pass
    sc[t] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {  // inclusive suffix sums
        const uint32_t a = t + o < 256u ? sc[t + o] : 0u;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    const uint32_t incl = sc[t], above = incl - mine;
    if (above < want && want <= incl) {  // exactly one bin (1 <= want <= the scores on the prefix)
        const uint32_t np = prefix | (t << (24u - 8u * d));
        sel[0] = np;
        sel[1] = want - above;
        sel[2] = gt + above;
        if (d == 3u) {
            const uint32_t top = gt + above + (np ? want - above : 0u);
            sel[3] = top;
            A.top_n[A.q0 + row] = top;
        }
    }
}

// the four scores of the thread in tile `tile` of the row: bits, 0 beyond the row
__device__ __forceinline__ uint4 srch_load4(const SearchPlan &A, uint32_t row, uint32_t tile, uint64_t *first) {
    const uint64_t i = (uint64_t)tile * SRCH_WG + threadIdx.x;
    *first = 4u * i;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (i < (A.stride >> 2)) q = reinterpret_cast<const uint4 *>(A.acc + (uint64_t)row * A.stride)[i];
    if (4u * i + 0u >= A.n_docs) q.x = 0u;
    if (4u * i + 1u >= A.n_docs) q.y = 0u;
    if (4u * i + 2u >= A.n_docs) q.z = 0u;
    if (4u * i + 3u >= A.n_docs) q.w = 0u;
    return q;
}

// documents above (low 16 bits) and at (high 16 bits) the threshold among the thread's four
__device__ __forceinline__ uint32_t srch_flags(const uint4 &q, uint32_t thr) {
    return (uint32_t)(q.x > thr) + (uint32_t)(q.y > thr) + (uint32_t)(q.z > thr) + (uint32_t)(q.w > thr) +
           (((uint32_t)(q.x == thr) + (uint32_t)(q.y == thr) + (uint32_t)(q.z == thr) + (uint32_t)(q.w == thr)) << 16);
}

__global__ __launch_bounds__(SRCH_WG) void k_srch_count(SearchPlan A) {
    __shared__ uint32_t s_w[SRCH_WG / 64];
    const uint32_t row = blockIdx.y, tile = blockIdx.x;
    uint64_t first;
    const uint4 q = srch_load4(A, row, tile, &first);
    uint32_t total;
    (void)mrg_wg_scan_excl<SRCH_WG / 64, false, false>(srch_flags(q, A.sel[4u * row]), s_w, &total);
    if (threadIdx.x == 0) {
        uint32_t *c = A.cnt + 2u * ((uint64_t)row * A.ntile + tile);
        c[0] = total & 0xFFFFu;
        c[1] = total >> 16;
    }
}

// cnt of a row -> its exclusive scans over the tiles, in place
__global__ __launch_bounds__(SRCH_WG) void k_srch_scan(SearchPlan A) {
    __shared__ uint32_t s_w[SRCH_WG / 64];
    uint32_t *c = A.cnt + 2u * ((uint64_t)blockIdx.x * A.ntile);
    uint32_t carry[2] = {0u, 0u};
    for (uint32_t base = 0; base < A.ntile; base += SRCH_WG) {  // (the trip count is the same in every thread)
        const uint32_t i = base + threadIdx.x;
        for (int k = 0; k < 2; ++k) {
            const uint32_t v = i < A.ntile ? c[2u * i + k] : 0u;
            uint32_t total;
            const uint32_t ex = mrg_wg_scan_excl<SRCH_WG / 64, false, false>(v, s_w, &total);
            if (i < A.ntile) c[2u * i + k] = carry[k] + ex;
            carry[k] += total;
            __syncthreads();  // s_w is written again
        }
    }
}

__global__ __launch_bounds__(SRCH_WG) void k_srch_take(SearchPlan A) {
    __shared__ uint32_t s_w[SRCH_WG / 64];
    const uint32_t row = blockIdx.y, tile = blockIdx.x;
    const uint32_t *sel = A.sel + 4u * row;
    const uint32_t thr = sel[0], need = thr ? sel[1] : 0u, n_gt = sel[2];
    uint64_t first;
    const uint4 q = srch_load4(A, row, tile, &first);
    const uint32_t mine = srch_flags(q, thr);
    uint32_t total;
    const uint32_t ex = mrg_wg_scan_excl<SRCH_WG / 64, false, false>(mine, s_w, &total);
    if (!mine) return;
    const uint32_t *c = A.cnt + 2u * ((uint64_t)row * A.ntile + tile);
    uint32_t g = c[0] + (ex & 0xFFFFu), e = c[1] + (ex >> 16);
    const uint32_t x[4] = {q.x, q.y, q.z, q.w};
    uint32_t *cd = A.cand_doc + (uint64_t)row * A.k, *cb = A.cand_bits + (uint64_t)row * A.k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t at = ~0u;
        if (x[j] > thr) at = g++;
        else if (x[j] == thr && e++ < need) at = n_gt + (e - 1u);
        if (at < A.k) {  // (always, for a slot that was given: n_gt + need <= k)
            cd[at] = (uint32_t)(first + (uint64_t)j);
            cb[at] = x[j];
        }
    }
}

// ---------------------------------------------------------------- order

// The candidates of one query, ranked by (score descending, document ascending): the keys (~bits, document)
// are distinct, so the rank of a key is the number of smaller keys.
__global__ __launch_bounds__(SRCH_WG) void k_srch_order(SearchPlan A) {
    __shared__ uint64_t s_k[MRG_SEARCH_MAX_K];
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = min(A.sel[4u * row + 3u], A.k);
    const uint32_t *cd = A.cand_doc + (uint64_t)row * A.k, *cb = A.cand_bits + (uint64_t)row * A.k;
    for (uint32_t i = tid; i < n; i += SRCH_WG) s_k[i] = ((uint64_t)~cb[i] << 32) | cd[i];
    __syncthreads();
    uint32_t *od = A.out_docs + ((uint64_t)A.q0 + row) * A.k;
    float *os = A.out_scores + ((uint64_t)A.q0 + row) * A.k;
    for (uint32_t i = tid; i < n; i += SRCH_WG) {
        const uint64_t key = s_k[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += s_k[j] < key ? 1u : 0u;
        od[rank] = (uint32_t)key + A.doc_base;
        os[rank] = __uint_as_float(~(uint32_t)(key >> 32));
    }
}

}  // namespace

void mrg_search_launch_gather(const uint32_t *q_ids, uint64_t n_ids, const uint64_t *post_off, uint64_t n_words,
                              uint64_t *po, hipStream_t s, const uint64_t *df, uint64_t *dfo) {
    if (n_ids)
        hipLaunchKernelGGL(k_srch_gather, dim3(grid_for(n_ids, SRCH_WG)), dim3(SRCH_WG), 0, s, q_ids, n_ids, post_off, n_words, po, df,
                           dfo);
}

void mrg_search_launch_sum(const uint32_t *doc_len, uint32_t n_docs, unsigned long long *sum, hipStream_t s) {
    if (!n_docs) return;
    const unsigned g = (unsigned)std::min<uint64_t>(grid_for(n_docs, SRCH_WG), (uint64_t)srch_cus() * 4u);
    hipLaunchKernelGGL(k_srch_sum, dim3(g), dim3(SRCH_WG), 0, s, doc_len, n_docs, sum);
}

void mrg_search_launch_acc(const SearchPlan &p, const SearchTile *tiles, uint64_t n, hipStream_t s) {
    for (uint64_t at = 0; at < n; at += 1u << 30) {  // (a grid has fewer than 2^31 workgroups)
        const unsigned g = (unsigned)std::min<uint64_t>(n - at, 1u << 30);
        hipLaunchKernelGGL(k_srch_acc<false>, dim3(g), dim3(SRCH_WG), 0, s, p, tiles + at);
    }
}

void mrg_search_launch_acc_bool(const SearchPlan &p, const SearchTile *tiles, uint64_t n, hipStream_t s) {
    for (uint64_t at = 0; at < n; at += 1u << 30) {
        const unsigned g = (unsigned)std::min<uint64_t>(n - at, 1u << 30);
        hipLaunchKernelGGL(k_srch_acc<true>, dim3(g), dim3(SRCH_WG), 0, s, p, tiles + at);
    }
}

void mrg_search_launch_filter(const SearchPlan &p, const SearchFilterRow *rows, uint32_t n, hipStream_t s) {
    if (!n) return;  // (n <= the chunk's rows <= 65535: a grid coordinate)
    const unsigned gx = (unsigned)std::min<uint64_t>(grid_for(p.stride >> 2, SRCH_WG), std::max(1u, (unsigned)srch_cus() * 8u / n));
    hipLaunchKernelGGL(k_srch_filter, dim3(gx, n), dim3(SRCH_WG), 0, s, p, rows);
}

void mrg_search_launch_select(const SearchPlan &p, hipStream_t s) {
    // the rows of a chunk are independent: grid.y = the row (chunks hold at most 65535 rows)
    const unsigned gx = (unsigned)std::min<uint64_t>(grid_for(p.stride >> 2, SRCH_WG), std::max(1u, (unsigned)srch_cus() * 8u / p.rows));
    for (uint32_t d = 0; d < 4u; ++d) {
        hipLaunchKernelGGL(k_srch_hist, dim3(gx, p.rows), dim3(SRCH_WG), 0, s, p, d);
        hipLaunchKernelGGL(k_srch_pick, dim3(p.rows), dim3(256), 0, s, p, d);
    }
    hipLaunchKernelGGL(k_srch_count, dim3(p.ntile, p.rows), dim3(SRCH_WG), 0, s, p);
    hipLaunchKernelGGL(k_srch_scan, dim3(p.rows), dim3(SRCH_WG), 0, s, p);
    hipLaunchKernelGGL(k_srch_take, dim3(p.ntile, p.rows), dim3(SRCH_WG), 0, s, p);
}

void mrg_search_launch_order(const SearchPlan &p, hipStream_t s) {
    hipLaunchKernelGGL(k_srch_order, dim3(p.rows), dim3(SRCH_WG), 0, s, p);
}
