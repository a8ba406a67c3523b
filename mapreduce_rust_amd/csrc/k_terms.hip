// k_terms.hip -- per-document term counts of id sequences: the document-term matrix in CSR form
// (gfx950).
//
// mrg_vocab_term_counts: row i = the distinct ids of document i other than MRG_ID_UNK, ascending, with
// their occurrences.  The host sorts the documents into three lists by their length T:
//   wave   T <= MRG_TERMS_WAVE_MAX: one wave per document, waves striding over the list.  The ids are
//          padded with MRG_ID_UNK to a power of two, bitonic-sorted in the wave's LDS and run-length
//          encoded: head flags, a wave scan, then one row entry per run.
//   wg     T <= MRG_TERMS_WG_MAX: the same by one 256-thread workgroup per document (block scan).
//   large  keys (rank of the document among the slice's documents) << 32 | id, sorted by the LSD radix
//          sort over the key bytes that can differ; head flags, a scan, the rows.
// Order comes from count -> scan -> emit: a count launch writes every document's row length and UNK
// count, the host layer scans the lengths (mrg_scan_u64), an emit launch sorts again and writes.  No
// kernel waits for another workgroup; the only atomics are the atomicMin of the first bad id.
// Every id is checked where it is loaded; loads are masked to the document's own ids.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int TRM_WG = 256;
constexpr int TRM_NW = TRM_WG / 64;
constexpr uint32_t TRM_UNK = 0xFFFFFFFFu;
static_assert((MRG_TERMS_WAVE_MAX & (MRG_TERMS_WAVE_MAX - 1u)) == 0 && MRG_TERMS_WAVE_MAX >= 64u, "power of two");
static_assert((MRG_TERMS_WG_MAX & (MRG_TERMS_WG_MAX - 1u)) == 0 && MRG_TERMS_WG_MAX >= (uint32_t)TRM_WG, "power of two");
static_assert(MRG_TERMS_WG_MAX < 65536u, "heads and UNKs of a document are scanned as two 16-bit halves");

int trm_cus() {
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

// NT = 64: the caller is one wave with LDS of its own; NT = 256: the whole workgroup
template <int NT>
__device__ __forceinline__ void trm_sync() {
    if (NT == 64) {
        mrg_wave_sync_lds();
    } else {
        __syncthreads();
    }
}

// One document by NT threads (tid = 0 .. NT - 1): s holds the padded length (a power of two >= NT), pos
// (EMIT only) the same.  Every thread of the NT takes every barrier: the trip counts depend on the
// document's length alone.
template <int NT, bool EMIT>
__device__ __forceinline__ void trm_doc(const TermsPlan &A, uint32_t doc, uint32_t *s, uint32_t *pos, uint32_t *s_red,
                                        uint32_t tid) {
    const uint64_t lo = A.tok_off[doc];
    const uint32_t T = (uint32_t)(A.tok_off[doc + 1] - lo);
    uint32_t P = NT;
    while (P < T) P <<= 1;
    for (uint32_t i = tid; i < P; i += NT) {
        uint32_t v = TRM_UNK;
        if (i < T) {
            v = A.in[lo + i];
            if (!EMIT && v != TRM_UNK && (uint64_t)v >= A.n_words) atomicMin(A.err, (unsigned long long)(lo + i));
        }
        s[i] = v;
    }
    trm_sync<NT>();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += NT) {
                const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;
                const uint32_t x = s[i], y = s[l];
                if ((y < x) == ((i & k) == 0)) {
                    s[i] = y;
                    s[l] = x;
                }
            }
            trm_sync<NT>();
        }
    }
    // run starts (heads) and UNKs (the padding included) of this thread's share [b, b + ipt)
    const uint32_t ipt = P / NT, b = tid * ipt;
    uint32_t prev = b ? s[b - 1] : 0u, h = 0, u = 0;
    for (uint32_t i = b; i < b + ipt; ++i) {
        const uint32_t v = s[i];
        h += (v != TRM_UNK && (i == 0 || v != prev)) ? 1u : 0u;
        u += v == TRM_UNK ? 1u : 0u;
        prev = v;
    }
    uint32_t tot;
    const uint32_t pre = mrg_wg_scan_excl<NT / 64>(h | (u << 16), s_red, &tot);
    const uint32_t nd = tot & 0xFFFFu, nu = tot >> 16;  // (nu <= P <= 4096, nd likewise)
    if (!EMIT) {
        if (tid == 0) {
            A.len[doc] = nd;
            A.unk[doc] = nu - (P - T);
        }
    } else {
        uint32_t r = pre & 0xFFFFu;
        prev = b ? s[b - 1] : 0u;
        for (uint32_t i = b; i < b + ipt; ++i) {
            const uint32_t v = s[i];
            if (v != TRM_UNK && (i == 0 || v != prev)) pos[r++] = i;
            prev = v;
        }
        trm_sync<NT>();
        const uint64_t base = A.len[doc];
        const uint32_t valid = P - nu;  // the ids that are not UNK stand first
        for (uint32_t q = tid; q < nd; q += NT) {
            const uint32_t at = pos[q], nx = q + 1 < nd ? pos[q + 1] : valid;
            A.terms[base + q] = s[at];
            A.counts[base + q] = nx - at;
        }
    }
    trm_sync<NT>();  // s and pos are reused by the next document
}

template <bool EMIT>
__global__ __launch_bounds__(TRM_WG) void k_terms_wave(TermsPlan A, const uint32_t *list, uint32_t n) {
    __shared__ uint32_t s_v[TRM_NW][MRG_TERMS_WAVE_MAX];
    __shared__ uint32_t s_p[TRM_NW][EMIT ? MRG_TERMS_WAVE_MAX : 1u];
    const uint32_t wv = threadIdx.x >> 6, lane = __lane_id();
    const uint32_t stride = gridDim.x * TRM_NW;
    for (uint32_t x = blockIdx.x * TRM_NW + wv; x < n; x += stride)
        trm_doc<64, EMIT>(A, list[x], s_v[wv], s_p[wv], nullptr, lane);
}

template <bool EMIT>
__global__ __launch_bounds__(TRM_WG) void k_terms_wg(TermsPlan A, const uint32_t *list, uint32_t n) {
    __shared__ uint32_t s_v[MRG_TERMS_WG_MAX];
    __shared__ uint32_t s_p[EMIT ? MRG_TERMS_WG_MAX : 1u];
    __shared__ uint32_t s_red[TRM_NW];
    for (uint32_t x = blockIdx.x; x < n; x += gridDim.x) trm_doc<TRM_WG, EMIT>(A, list[x], s_v, s_p, s_red, threadIdx.x);
}

// ---- the large path
__global__ __launch_bounds__(TRM_WG) void k_terms_keys(TermsPlan A, TermsSlice S, uint64_t *keys) {
    const uint64_t i = (uint64_t)blockIdx.x * TRM_WG + threadIdx.x;
    if (i >= S.m) return;
    const uint32_t j = mrg_last_le(S.soff, 0u, S.nd, i);  // the slice document that holds position i
    const uint64_t at = A.tok_off[S.ldoc[j]] + (i - S.soff[j]);
    const uint32_t v = A.in[at];
    if (v != TRM_UNK && (uint64_t)v >= A.n_words) atomicMin(A.err, (unsigned long long)at);
    keys[i] = ((uint64_t)j << 32) | min((uint64_t)v, A.n_words);
}

__global__ __launch_bounds__(TRM_WG) void k_terms_flags(const uint64_t *keys, uint64_t m, uint64_t n_words,
                                                        uint32_t *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * TRM_WG + threadIdx.x;
    if (i > m) return;
    uint32_t f = 0;
    if (i < m) {
        const uint64_t k = keys[i];
        f = ((k & 0xFFFFFFFFull) != n_words && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
    }
    flag[i] = f;
}

// one thread per document of the slice: its run starts, and its UNKs (the keys at the end of its segment)
__global__ __launch_bounds__(TRM_WG) void k_terms_rows(TermsPlan A, TermsSlice S, const uint64_t *keys, const uint32_t *E) {
    const uint32_t j = blockIdx.x * TRM_WG + threadIdx.x;
    if (j >= S.nd) return;
    const uint64_t lo = S.soff[j], hi = S.soff[j + 1];
    const uint64_t want = ((uint64_t)j << 32) | A.n_words;
    uint64_t a = lo, b = hi;  // the first position in [lo, hi] whose key is >= want
    while (a < b) {
        const uint64_t m = a + ((b - a) >> 1);
        if (keys[m] < want) a = m + 1;
        else b = m;
    }
    const uint32_t doc = S.ldoc[j];
    A.len[doc] = E[hi] - E[lo];
    A.unk[doc] = hi - a;
}

__global__ __launch_bounds__(TRM_WG) void k_terms_pos(const uint64_t *keys, uint64_t m, uint64_t n_words,
                                                      const uint32_t *E, uint32_t *pos) {
    const uint64_t i = (uint64_t)blockIdx.x * TRM_WG + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = keys[i];
    if ((k & 0xFFFFFFFFull) != n_words && (i == 0 || keys[i - 1] != k)) pos[E[i]] = (uint32_t)i;
}

// one thread per run r of the slice (E[m] of them): the run ends at the next run of its document, or
// where the document's UNKs begin
__global__ __launch_bounds__(TRM_WG) void k_terms_write(TermsPlan A, TermsSlice S, const uint64_t *keys, const uint32_t *E,
                                                        const uint32_t *pos) {
    const uint64_t r = (uint64_t)blockIdx.x * TRM_WG + threadIdx.x;
    const uint64_t H = E[S.m];
    if (r >= H) return;
    const uint32_t at = pos[r];
    const uint64_t k = keys[at];
    const uint32_t j = (uint32_t)(k >> 32);
    const uint32_t doc = S.ldoc[j];
    uint64_t end = S.soff[j + 1] - A.unk[doc];
    if (r + 1 < H) {
        const uint32_t nx = pos[r + 1];
        if ((uint32_t)(keys[nx] >> 32) == j) end = nx;
    }
    const uint64_t dst = A.len[doc] + (r - E[S.soff[j]]);
    A.terms[dst] = (uint32_t)k;
    A.counts[dst] = (uint32_t)(end - at);
}

}  // namespace

void mrg_terms_launch_lds(const TermsPlan &p, const uint32_t *list, uint32_t n, bool wg, bool emit, hipStream_t s) {
    if (!n) return;
    // all workgroups resident (8 per CU), striding over the list
    const uint64_t need = wg ? n : ((uint64_t)n + TRM_NW - 1) / TRM_NW;
    const unsigned g = (unsigned)std::min<uint64_t>(need, (uint64_t)trm_cus() * 8u);
    if (wg) {
        if (emit) hipLaunchKernelGGL(k_terms_wg<true>, dim3(g), dim3(TRM_WG), 0, s, p, list, n);
        else hipLaunchKernelGGL(k_terms_wg<false>, dim3(g), dim3(TRM_WG), 0, s, p, list, n);
    } else {
        if (emit) hipLaunchKernelGGL(k_terms_wave<true>, dim3(g), dim3(TRM_WG), 0, s, p, list, n);
        else hipLaunchKernelGGL(k_terms_wave<false>, dim3(g), dim3(TRM_WG), 0, s, p, list, n);
    }
}

void mrg_terms_launch_keys(const TermsPlan &p, const TermsSlice &sl, uint64_t *keys, hipStream_t s) {
    hipLaunchKernelGGL(k_terms_keys, dim3(grid_for(sl.m, TRM_WG)), dim3(TRM_WG), 0, s, p, sl, keys);
}
void mrg_terms_launch_flags(const uint64_t *keys, uint64_t m, uint64_t n_words, uint32_t *flag, hipStream_t s) {
    hipLaunchKernelGGL(k_terms_flags, dim3(grid_for(m + 1, TRM_WG)), dim3(TRM_WG), 0, s, keys, m, n_words, flag);
}
void mrg_terms_launch_rows(const TermsPlan &p, const TermsSlice &sl, const uint64_t *keys, const uint32_t *E,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_terms_rows, dim3(grid_for(sl.nd, TRM_WG)), dim3(TRM_WG), 0, s, p, sl, keys, E);
}
void mrg_terms_launch_write(const TermsPlan &p, const TermsSlice &sl, const uint64_t *keys, const uint32_t *E,
                            uint32_t *pos, hipStream_t s) {
    hipLaunchKernelGGL(k_terms_pos, dim3(grid_for(sl.m, TRM_WG)), dim3(TRM_WG), 0, s, keys, sl.m, p.n_words, E, pos);
    hipLaunchKernelGGL(k_terms_write, dim3(grid_for(sl.m, TRM_WG)), dim3(TRM_WG), 0, s, p, sl, keys, E, (const uint32_t *)pos);
}
