// k_postings.hip -- the inverted index over ids: the transpose (CSC) of the document-term matrix that
// mrg_vocab_term_counts writes (gfx950).
//
// mrg_vocab_postings: count -> scan -> stable scatter.
//   count   one read of the terms (16-byte loads over the aligned body of the range, the few entries
//           before and after it one by one): every term is checked against the vocabulary (atomicMin of
//           the first bad index) and counted into the document-frequency histogram.  Terms below
//           MRG_POST_LDS_WORDS -- the hot ones of a ranked vocabulary -- go to a histogram in the
//           workgroup's LDS that is flushed with one global atomic per non-zero bin, the others to global
//           atomics.  The host layer scans the histogram in place into d_post_off (mrg_scan_u64).
//   pack    one workgroup per tile of MRG_POST_TILE consecutive entries: the rows of the tile's first and
//           last entry by binary search over all row offsets, the row of every entry by a search between
//           those two that starts at the row of the thread's previous entry; writes (term, doc, tf).
//   sort    the LSD radix sort of k_sort.hip over the term's bytes only (mrg_radix_sort_post); the entries
//           stand in document order, so stability gives every word its documents ascending.
//   unpack  doc and tf of the sorted records, coalesced.
// No kernel waits for another workgroup; no order depends on scheduling (the atomics only add).
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int PST_WG = 256;
constexpr int PST_IPT = MRG_POST_TILE / PST_WG;
static_assert(MRG_POST_TILE % PST_WG == 0 && PST_IPT >= 1, "whole rounds of the workgroup per tile");
// the count kernel keeps at least 4 workgroups per CU resident (160 KiB of LDS per CU)
static_assert(4u * (MRG_POST_LDS_WORDS * 4u + 64u) <= 160u * 1024u, "4 workgroups per CU");

int pst_cus() {
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

// one term, standing at index `at` of the terms
__device__ __forceinline__ void pst_count_one(const PostPlan &A, uint32_t t, uint64_t at, uint32_t *s_h, uint32_t &n_lds,
                                              uint32_t &n_glb) {
    if ((uint64_t)t >= A.n_words) {
        atomicMin(&A.stat[0], (unsigned long long)at);
    } else if (t < MRG_POST_LDS_WORDS) {
        atomicAdd(&s_h[t], 1u);
        ++n_lds;
    } else {
        atomicAdd(&A.df[t], 1ull);
        ++n_glb;
    }
}

__global__ __launch_bounds__(PST_WG) void k_post_count(PostPlan A) {
    __shared__ uint32_t s_h[MRG_POST_LDS_WORDS];
    const uint32_t tid = threadIdx.x;
    const uint32_t nb = (uint32_t)min(A.n_words, (uint64_t)MRG_POST_LDS_WORDS);
    for (uint32_t i = tid; i < nb; i += PST_WG) s_h[i] = 0;
    __syncthreads();
    // [lo, hi) = head (up to the first 16-byte boundary) + nvec vectors of 4 + tail (< 4 entries)
    const uint64_t lo = A.lo, n = A.hi - A.lo;
    const uint64_t head = min((uint64_t)(((16u - ((uintptr_t)(A.terms + lo) & 15u)) & 15u) >> 2), n);
    const uint64_t nvec = (n - head) >> 2;
    const uint64_t body = lo + head, tail = body + 4u * nvec;
    const uint4 *vp = (const uint4 *)(A.terms + body);
    uint32_t n_lds = 0, n_glb = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * PST_WG + tid; i < nvec; i += (uint64_t)gridDim.x * PST_WG) {
        const uint4 v = vp[i];
        const uint64_t at = body + 4u * i;
        pst_count_one(A, v.x, at, s_h, n_lds, n_glb);
        pst_count_one(A, v.y, at + 1u, s_h, n_lds, n_glb);
        pst_count_one(A, v.z, at + 2u, s_h, n_lds, n_glb);
        pst_count_one(A, v.w, at + 3u, s_h, n_lds, n_glb);
    }
    if (blockIdx.x == 0) {  // head: lanes 0..2 of wave 0, tail: lanes 0..2 of wave 1
        if (tid < head) pst_count_one(A, A.terms[lo + tid], lo + tid, s_h, n_lds, n_glb);
        if (tid >= 64u && tail + (tid - 64u) < A.hi)
            pst_count_one(A, A.terms[tail + (tid - 64u)], tail + (tid - 64u), s_h, n_lds, n_glb);
    }
    __syncthreads();
    for (uint32_t i = tid; i < nb; i += PST_WG) {
        const uint32_t x = s_h[i];
        if (x) atomicAdd(&A.df[i], (unsigned long long)x);
    }
    n_lds = mrg_wave_sum_lane0(n_lds);
    n_glb = mrg_wave_sum_lane0(n_glb);
    if (__lane_id() == 0) {
        if (n_lds) atomicAdd(&A.stat[1], (unsigned long long)n_lds);
        if (n_glb) atomicAdd(&A.stat[2], (unsigned long long)n_glb);
    }
}

// stat[3] = the largest document frequency (before the scan turns df into the offsets)
__global__ __launch_bounds__(PST_WG) void k_post_max(const unsigned long long *df, uint64_t n_words,
                                                    unsigned long long *stat) {
    unsigned long long m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * PST_WG + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * PST_WG)
        m = max(m, df[i]);
    // not mrg_wave_max: only lane 0 needs it, and the shifts down take 8 instructions fewer than the butterfly
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned long long)__shfl_down(m, o));
    if (__lane_id() == 0 && m) atomicMax(&stat[3], m);
}

__global__ __launch_bounds__(PST_WG) void k_post_pack(PostPlan A, PostRec *out) {
    __shared__ uint32_t s_r[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = A.hi - A.lo;
    const uint64_t t0 = (uint64_t)blockIdx.x * MRG_POST_TILE, t1 = min(t0 + MRG_POST_TILE, n);  // (t0 < n by the grid)
    if (tid < 2u) s_r[tid] = mrg_last_le(A.row_off, 0u, A.n_docs, A.lo + (tid ? t1 - 1u : t0));
    __syncthreads();
    const uint32_t r1 = s_r[1];
    uint32_t r = s_r[0];  // rows ascend with the entries of a thread
    for (int k = 0; k < PST_IPT; ++k) {
        const uint64_t i = t0 + (uint64_t)k * PST_WG + tid;
        if (i >= t1) break;
        const uint64_t pos = A.lo + i;
        r = mrg_last_le(A.row_off, r, r1 + 1u, pos);  // off[r1 + 1] > lo + t1 - 1 >= pos
        out[i] = PostRec{A.terms[pos], A.doc_base + r, A.counts ? A.counts[pos] : 0u};
    }
}

__global__ __launch_bounds__(PST_WG) void k_post_unpack(const PostRec *in, uint64_t n, uint32_t *docs, uint32_t *tf) {
    const uint64_t i = (uint64_t)blockIdx.x * PST_WG + threadIdx.x;
    if (i >= n) return;
    const PostRec r = in[i];
    docs[i] = r.doc;
    if (tf) tf[i] = r.tf;
}

}  // namespace

void mrg_post_launch_count(const PostPlan &p, hipStream_t s) {
    // all workgroups resident (4 per CU), striding over the 16-byte vectors
    const uint64_t nvec = (p.hi - p.lo) / 4u;
    const unsigned g = (unsigned)std::min<uint64_t>(grid_for(nvec, PST_WG), (uint64_t)pst_cus() * 4u);
    hipLaunchKernelGGL(k_post_count, dim3(g), dim3(PST_WG), 0, s, p);
}

void mrg_post_launch_max(const PostPlan &p, hipStream_t s) {
    const unsigned g = (unsigned)std::min<uint64_t>(grid_for(p.n_words, PST_WG), (uint64_t)pst_cus() * 4u);
    hipLaunchKernelGGL(k_post_max, dim3(g), dim3(PST_WG), 0, s, (const unsigned long long *)p.df, p.n_words, p.stat);
}

void mrg_post_launch_pack(const PostPlan &p, PostRec *out, hipStream_t s) {
    if (p.hi == p.lo) return;
    hipLaunchKernelGGL(k_post_pack, dim3(grid_for(p.hi - p.lo, MRG_POST_TILE)), dim3(PST_WG), 0, s, p, out);
}

void mrg_post_launch_unpack(const PostRec *in, uint64_t n, uint32_t *docs, uint32_t *tf, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_post_unpack, dim3(grid_for(n, PST_WG)), dim3(PST_WG), 0, s, in, n, docs, tf);
}
