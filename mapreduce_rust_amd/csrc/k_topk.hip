// k_topk.hip -- the K most frequent words, selected on the device (gfx950).
//
// The distinct keys and their counts are resident after the map (KeySet).  A word-count user's first
// question -- which words are most frequent -- needs the K best keys by (count descending, key bytes
// ascending), not the sorted listing of all of them, so nothing here sorts the whole key set:
//   select   radix select over the 24-byte composite (~count, k0, k1), most significant byte first.
//            One pass = k_sel_hist (stream the counts, 16-byte loads, grid sized to the device; LDS
//            histogram of the current byte among the keys still tied on the prefix) + k_sel_pick (one
//            workgroup: the bin holding the wanted rank becomes the next prefix byte).  The state is
//            device memory; passes that have nothing to do (above the largest count's first byte, or
//            after the select finished) return at once, so the host enqueues all of them blindly.
//   compact  keys at or below the prefix -> SortRecs (a few more than wanted: ties on the last byte,
//            or long keys sharing count and 16-byte prefix).
//   drop     the reference never writes the byte-largest key of a partition (worker.rs:169-184).  Only
//            the byte-largest candidate of a partition can be that key, and it is iff no key of the
//            partition exceeds it: one streaming pass over (part, k0), no sort.
// The candidates are then ordered by the existing sorts and formatted by the existing line writer
// (mrg_reduce.cpp job_topk).  Every ballot / shuffle below runs in loops whose trip count is uniform per
// workgroup, with out-of-range lanes predicated off, never returned early.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int SEL_WG = 256;

// workgroups of a streaming pass over n items, `per` items per workgroup iteration: sized to the
// device (8 per CU), grid-stride over the rest
unsigned stream_grid(uint64_t n, uint64_t per) {
    static int cus[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int cu = (dev >= 0 && dev < 64) ? cus[dev] : 0;
    if (cu == 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        if (dev >= 0 && dev < 64) cus[dev] = cu;
    }
    const uint64_t need = (n + per - 1) / per;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cu * 8u));
}

__global__ __launch_bounds__(SEL_WG) void k_sel_max(const uint64_t *cnt, uint64_t n, TopkState *st) {
    __shared__ unsigned long long m_s;
    static_assert(sizeof(unsigned long long) <= 64 * 1024, "k_sel_max LDS");
    if (threadIdx.x == 0) m_s = 0ull;
    __syncthreads();
    unsigned long long m = 0ull;
    const uint64_t npair = (n + 1) / 2;
    for (uint64_t t = (uint64_t)blockIdx.x * SEL_WG + threadIdx.x; t < npair; t += (uint64_t)gridDim.x * SEL_WG) {
        const uint64_t i = 2 * t;
        if (i + 1 < n) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(cnt + i);
            m = max(m, max(q.x, q.y));
        } else {
            m = max(m, (unsigned long long)cnt[i]);
        }
    }
    atomicMax(&m_s, m);
    __syncthreads();
    if (threadIdx.x == 0 && m_s) atomicMax(&st->maxcnt, m_s);
}

// the select starts at the first non-zero byte of the largest count (counts are heavily skewed: most
// keys occur once or twice, the high bytes of every count are zero)
__global__ void k_sel_init(TopkState *st, uint64_t want) {
    const unsigned long long m = st->maxcnt;
    st->pre[0] = ~0ull;  // ~count of the skipped bytes
    st->pre[1] = st->pre[2] = 0ull;
    st->want = want;
    st->better = st->tied = 0ull;
    st->digit = m ? (uint32_t)__builtin_clzll(m) >> 3 : 7u;
    st->done = 0u;
}

// One LDS add per distinct bin present in the wave for the first few bins (skewed digits: usually
// one), plain LDS atomics for what is left.  Reached by every lane of the wave.
__device__ __forceinline__ void hist_add(uint32_t *h, uint32_t bin, bool act) {
    uint64_t rem = __ballot(act);
    for (int it = 0; it < 4 && rem; ++it) {  // (rem is wave-uniform)
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t lb = (uint32_t)__shfl((int)bin, leader);
        const bool mine = act && bin == lb;
        const uint64_t m = __ballot(mine);
        if ((int)__lane_id() == leader) atomicAdd(&h[lb], (uint32_t)__popcll(m));
        rem &= ~m;
        act = act && !mine;
    }
    if (act) atomicAdd(&h[bin], 1u);
}

// L = composite word of digit d (0: ~count, 1: k0, 2: k1).  A key takes part when its composite
// matches the prefix on the first d bytes; k0 / k1 are loaded for such keys only.
template <int L>
__device__ __forceinline__ void sel_one(uint32_t *h, uint64_t w0, uint64_t i, bool act, const uint64_t *k0,
                                        const uint64_t *k1, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t mask,
                                        uint32_t sh) {
    uint64_t w = w0;
    if (L >= 1) {
        act = act && w0 == p0;
        w = act ? k0[i] : 0ull;
    }
    if (L >= 2) {
        act = act && w == p1;
        w = act ? k1[i] : 0ull;
    }
    const uint64_t pl = L == 0 ? p0 : (L == 1 ? p1 : p2);
    act = act && ((w ^ pl) & mask) == 0ull;
    hist_add(h, (uint32_t)(w >> sh) & 0xFFu, act);
}

template <int L>
__global__ __launch_bounds__(SEL_WG) void k_sel_hist(const uint64_t *cnt, const uint64_t *k0, const uint64_t *k1,
                                                     uint64_t n, TopkState *st, uint32_t d) {
    __shared__ uint32_t h[256];
    static_assert(sizeof(uint32_t) * 256 <= 64 * 1024, "k_sel_hist LDS");
    if (st->done || st->digit != d) return;  // (the same in every thread of the grid)
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t b = d & 7u;
    const uint64_t mask = b ? ~0ull << (64u - 8u * b) : 0ull;
    const uint32_t sh = 56u - 8u * b;
    const uint64_t p0 = st->pre[0], p1 = st->pre[1], p2 = st->pre[2];
    const uint64_t npair = (n + 1) / 2;
    for (uint64_t base = (uint64_t)blockIdx.x * SEL_WG; base < npair; base += (uint64_t)gridDim.x * SEL_WG) {
        const uint64_t i = 2 * (base + threadIdx.x);
        const bool v0 = i < n, v1 = i + 1 < n;
        uint64_t c0 = 0ull, c1 = 0ull;
        if (v1) {
            const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(cnt + i);
            c0 = q.x;
            c1 = q.y;
        } else if (v0) {
            c0 = cnt[i];
        }
        sel_one<L>(h, ~c0, i, v0, k0, k1, p0, p1, p2, mask, sh);
        sel_one<L>(h, ~c1, i + 1, v1, k0, k1, p0, p1, p2, mask, sh);
    }
    __syncthreads();
    const uint32_t v = h[threadIdx.x];
    if (v) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)v);  // one global add per non-empty bin
}

__global__ __launch_bounds__(256) void k_sel_pick(TopkState *st, uint32_t d) {
    __shared__ uint64_t sc[256];
    static_assert(sizeof(uint64_t) * 256 <= 64 * 1024, "k_sel_pick LDS");
    if (st->done || st->digit != d) return;
    const uint32_t t = threadIdx.x;
    const uint64_t mine = st->hist[t];
    const uint64_t want = st->want;
    sc[t] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {  // inclusive scan
        const uint64_t a = t >= o ? sc[t - o] : 0ull;
        __syncthreads();
        sc[t] += a;
        __syncthreads();
    }
    const uint64_t incl = sc[t], excl = incl - mine, total = sc[255];
    st->hist[t] = 0ull;  // for the next pass
    if (excl < want && want <= incl) {  // exactly one bin (1 <= want <= total)
        const uint32_t L = d >> 3, sh = 56u - 8u * (d & 7u);
        st->pre[L] = (st->pre[L] & ~(0xFFull << sh)) | ((uint64_t)t << sh);
        st->better += excl;
        st->want = want - excl;
        st->tied = mine;
        st->digit = d + 1u;
        // the whole bin is wanted: every key on the new prefix is in, nothing is left to select
        st->done = (mine == want - excl || d + 1u == MRG_TOPK_DIGITS) ? 1u : 0u;
        st->passes += 1u;
        st->parts[d] = total;
    }
}

// composite cut to nd bytes <= prefix cut to nd bytes
__device__ __forceinline__ uint64_t cut_mask(uint32_t nd, uint32_t word) {
    const uint32_t lo = 8u * word;
    const uint32_t nb = nd <= lo ? 0u : (nd - lo >= 8u ? 8u : nd - lo);
    return nb ? ~0ull << (64u - 8u * nb) : 0ull;
}

__global__ __launch_bounds__(SEL_WG) void k_topk_compact(KeySet ks, uint64_t n, TopkState *st, SortRec *out,
                                                         uint64_t cap) {
    const uint32_t nd = st->digit;
    const uint64_t m0 = cut_mask(nd, 0), m1 = cut_mask(nd, 1), m2 = cut_mask(nd, 2);
    const uint64_t p0 = st->pre[0] & m0, p1 = st->pre[1] & m1, p2 = st->pre[2] & m2;
    for (uint64_t base = (uint64_t)blockIdx.x * SEL_WG; base < n; base += (uint64_t)gridDim.x * SEL_WG) {
        const uint64_t i = base + threadIdx.x;
        const bool v = i < n;
        bool cand = false;
        uint64_t a0 = 0ull, a1 = 0ull;
        if (v) {
            const uint64_t w0 = ~ks.cnt[i] & m0;
            if (w0 != p0) {
                cand = w0 < p0;
            } else {  // (the key words are read only for keys tied on the count, and for candidates)
                a0 = ks.k0[i];
                if ((a0 & m1) != p1) cand = (a0 & m1) < p1;
                else cand = !m2 || (ks.k1[i] & m2) <= p2;
            }
            if (cand) {
                a0 = ks.k0[i];
                a1 = ks.k1[i];
            }
        }
        const uint64_t slot = mrg_wave_append(&st->ncand, cand);  // (every lane gets here)
        if (cand && slot < cap) {
            SortRec r;
            r.k0 = a0;
            r.k1 = a1;
            r.part = 0u;
            r.doc = 0u;
            r.idx = (uint32_t)i;
            r.pad = 0u;
            out[slot] = r;
        }
    }
}

__global__ void k_topk_cand_last(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, uint32_t *cand_last) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t p = ks.part[r[j].idx];
    if (p < R && cand_last[p] < (uint32_t)(j + 1)) atomicMax(&cand_last[p], (uint32_t)(j + 1));
}

// key i byte-greater than the candidate c (distinct keys)?  k0 / k1 first; on a 16-byte-prefix tie
// the lengths and, for two long keys, the heap bytes
__device__ bool key_exceeds(const KeySet &ks, const uint8_t *heap, uint64_t i, const SortRec &c) {
    const uint64_t a0 = ks.k0[i];
    if (a0 != c.k0) return a0 > c.k0;
    const uint64_t a1 = ks.k1[i];
    if (a1 != c.k1) return a1 > c.k1;
    if (i == c.idx) return false;
    const uint32_t li = ks.len[i], lc = ks.len[c.idx];
    if (li <= 16u || lc <= 16u) return li > lc;  // the 16-byte key is a prefix of the long one
    const uint8_t *x = heap + ks.hoff[i], *y = heap + ks.hoff[c.idx];
    const uint32_t l = li < lc ? li : lc;
    for (uint32_t b = 16; b < l; ++b)
        if (x[b] != y[b]) return x[b] > y[b];
    return li > lc;
}

__global__ __launch_bounds__(SEL_WG) void k_topk_exceed(KeySet ks, const uint8_t *heap, uint64_t n, const SortRec *r,
                                                        uint32_t R, const uint32_t *cand_last, uint32_t *exceeded) {
    for (uint64_t i = (uint64_t)blockIdx.x * SEL_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SEL_WG) {
        const uint32_t p = ks.part[i];
        if (p >= R) continue;  // (never: a key's partition is its hash % R)
        const uint32_t cl = cand_last[p];
        // (a stale 0 from the unsynchronised read only repeats the store of 1)
        if (cl == 0u || exceeded[p]) continue;
        if (key_exceeds(ks, heap, i, r[cl - 1u])) exceeded[p] = 1u;
    }
}

__global__ void k_topk_count_keys(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, const uint32_t *cand_last,
                                  const uint32_t *exceeded, uint64_t *keys, uint32_t *vals, TopkState *st) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t e = r[j].idx;
    bool dropped = false;
    if (cand_last) {
        const uint32_t p = ks.part[e];
        dropped = p < R && cand_last[p] == (uint32_t)(j + 1) && exceeded[p] == 0u;
    }
    keys[j] = dropped ? ~0ull : ~ks.cnt[e];  // (a count is never 0: dropped candidates sort last)
    vals[j] = (uint32_t)j;
    if (dropped) atomicAdd(&st->ndrop, 1ull);  // at most one per partition
}

__global__ void k_topk_gather(const SortRec *r, const uint32_t *vals, uint64_t m, SortRec *out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = r[vals[j]];
}

}  // namespace

void mrg_topk_select(KeySet ks, uint64_t n, uint64_t want, TopkState *st, hipStream_t s) {
    if (n == 0 || want == 0 || want >= n) return;
    const dim3 g(stream_grid(n, 2 * SEL_WG)), b(SEL_WG);
    hipLaunchKernelGGL(k_sel_max, g, b, 0, s, (const uint64_t *)ks.cnt, n, st);
    hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(1), 0, s, st, want);
    for (uint32_t d = 0; d < MRG_TOPK_DIGITS; ++d) {
        const uint64_t *c = ks.cnt, *k0 = ks.k0, *k1 = ks.k1;
        if (d < 8) hipLaunchKernelGGL(k_sel_hist<0>, g, b, 0, s, c, k0, k1, n, st, d);
        else if (d < 16) hipLaunchKernelGGL(k_sel_hist<1>, g, b, 0, s, c, k0, k1, n, st, d);
        else hipLaunchKernelGGL(k_sel_hist<2>, g, b, 0, s, c, k0, k1, n, st, d);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, s, st, d);
    }
}

void mrg_topk_compact(KeySet ks, uint64_t n, TopkState *st, SortRec *out, uint64_t cap, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_topk_compact, dim3(stream_grid(n, SEL_WG)), dim3(SEL_WG), 0, s, ks, n, st, out, cap);
}

void mrg_topk_cand_last(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, uint32_t *cand_last, hipStream_t s) {
    if (m) hipLaunchKernelGGL(k_topk_cand_last, grid_for(m, 256), dim3(256), 0, s, r, m, ks, R, cand_last);
}

void mrg_topk_exceed(KeySet ks, const uint8_t *heap, uint64_t n, const SortRec *r, uint32_t R,
                     const uint32_t *cand_last, uint32_t *exceeded, hipStream_t s) {
    if (n)
        hipLaunchKernelGGL(k_topk_exceed, dim3(stream_grid(n, SEL_WG)), dim3(SEL_WG), 0, s, ks, heap, n, r, R,
                           cand_last, exceeded);
}

void mrg_topk_count_keys(const SortRec *r, uint64_t m, KeySet ks, uint32_t R, const uint32_t *cand_last,
                         const uint32_t *exceeded, uint64_t *keys, uint32_t *vals, TopkState *st, hipStream_t s) {
    if (m) hipLaunchKernelGGL(k_topk_count_keys, grid_for(m, 256), dim3(256), 0, s, r, m, ks, R, cand_last, exceeded, keys, vals, st);
}

void mrg_topk_gather(const SortRec *r, const uint32_t *vals, uint64_t m, SortRec *out, hipStream_t s) {
    if (m) hipLaunchKernelGGL(k_topk_gather, grid_for(m, 256), dim3(256), 0, s, r, vals, m, out);
}
