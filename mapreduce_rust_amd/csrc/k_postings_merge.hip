// k_postings_merge.hip -- the inverted indexes of the shards of one collection -> the index of the whole, on the
// device (gfx950).
//
// The shards partition the documents in ascending ranges, so the postings of a word are shard 0's, then shard
// 1's, ...: no step compares documents, the merge is a segmented copy.  mrg_vocab_postings_merge: sum -> scan ->
// place -> copy.
//   sum    one thread per word loops over the shards: the offsets of every shard are checked (they start at 0, do
//          not decrease, end at the shard's entries; atomicMin of word * 64 + shard otherwise) and the word's
//          frequencies summed into d_post_off, which the host layer scans in place (mrg_scan_u64).  Offsets that
//          pass lie in [0, entries]: the copy below cannot leave a shard's arrays or the output's entries.
//   place  one thread per word loops over the shards: dst[s][w] = the output position of shard s's first posting
//          of w, the scanned offset plus the frequencies of the lower shards (below 2^32: 4 bytes per cell); the
//          last document of a non-empty list must stand below the first of the next non-empty one (the seams:
//          atomicMin as above, naming the later shard).  Also counts the tiles that lie inside one word.
//   copy   one workgroup per (shard, tile of MRG_PMERGE_TILE consecutive source entries).  The words of the
//          tile's first and last entry by binary search over the shard's offsets.  One word: the tile is a
//          shifted copy -- 16-byte stores at the aligned output positions, fed by one 16-byte load where the
//          source is aligned alike and by two neighbouring ones otherwise.  Several words: a thread loads its
//          entries, one dword each, then finds the word of every entry by a search between the two words that
//          starts at the word of its previous entry -- over the words' offsets staged in LDS with their places
//          when the tile spans at most MRG_PMERGE_TILE words, over the offsets in memory otherwise.
// No workgroup waits for another; the atomics take a minimum or add to a counter of the diagnostics, none
// touches an offset or a posting: the outputs do not depend on scheduling.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int PMG_WG = 256;
constexpr int PMG_IPT = MRG_PMERGE_TILE / PMG_WG;
static_assert(MRG_PMERGE_TILE % (4 * PMG_WG) == 0 && PMG_IPT >= 1, "whole rounds of the workgroup per tile");
static_assert(MRG_SEARCH_MAX_SHARDS <= 64u, "the error cell holds word * 64 + shard");
// the copy kernel stages the offsets and places of up to PMG_LDS_WORDS words of a tile in LDS (16 KiB: 8 workgroups
// per CU stay resident)
constexpr uint32_t PMG_LDS_WORDS = MRG_PMERGE_TILE;
static_assert(8u * (2u * PMG_LDS_WORDS + 3u) * 4u <= 160u * 1024u, "8 workgroups per CU");

__global__ __launch_bounds__(PMG_WG) void k_pmerge_sum(PMergePlan A) {
    const uint64_t w = (uint64_t)blockIdx.x * PMG_WG + threadIdx.x;
    if (w > A.n_words) return;
    if (w == A.n_words) {  // the cell the scan turns into the total; an empty vocabulary has only off[0] to check
        if (w == 0)
            for (uint32_t s = 0; s < A.n_shards; ++s)
                if (A.sh[s].off[0] != 0) atomicMin(A.stat, (unsigned long long)s);
        A.post_off[w] = 0;
        return;
    }
    uint64_t sum = 0;
    for (uint32_t s = 0; s < A.n_shards; ++s) {
        const uint64_t a = A.sh[s].off[w], b = A.sh[s].off[w + 1];
        const bool bad = b < a || (w == 0 && a != 0) || (w + 1 == A.n_words && b != A.sh[s].n);
        if (bad) atomicMin(A.stat, (unsigned long long)(w * 64u + s));
        else sum += b - a;
    }
    A.post_off[w] = sum;
}

// tiles [t * T, min((t + 1) * T, n)) of a shard of n entries that lie inside [a, b), a < b <= n
__device__ __forceinline__ uint32_t pmg_tiles_inside(uint64_t a, uint64_t b, uint64_t n) {
    const uint64_t T = MRG_PMERGE_TILE, first = (a + T - 1) / T, full = b / T;
    uint32_t cnt = full > first ? (uint32_t)(full - first) : 0u;
    if (b == n && (n % T) && (n / T) * T >= a) ++cnt;  // the shard's last, short tile
    return cnt;
}

__global__ __launch_bounds__(PMG_WG) void k_pmerge_place(PMergePlan A) {
    const uint64_t w = (uint64_t)blockIdx.x * PMG_WG + threadIdx.x;
    uint32_t single = 0;
    if (w < A.n_words) {
        uint64_t pos = A.post_off[w];
        uint32_t last = 0;
        bool have = false;
        for (uint32_t s = 0; s < A.n_shards; ++s) {
            const PMergeShard S = A.sh[s];
            A.dst[(uint64_t)s * A.n_words + w] = (uint32_t)pos;
            const uint64_t a = S.off[w], b = S.off[w + 1];
            if (a == b) continue;
            if (have && S.docs[a] <= last) atomicMin(A.stat, (unsigned long long)(w * 64u + s));
            last = S.docs[b - 1u];
            have = true;
            single += pmg_tiles_inside(a, b, S.n);
            pos += b - a;
        }
    }
    single = mrg_wave_sum_lane0(single);
    if (__lane_id() == 0 && single) atomicAdd(A.stat + 1, (unsigned long long)single);
}

// out[0, len) = src[0, len), src = base + at of an array of n entries; the workgroup's threads together.
// The body goes in 16-byte stores at the aligned output positions; a store's four entries come from one aligned
// 16-byte load when the source is aligned like the output, else from the two aligned loads around them, and from
// four dword loads where one of those two would leave the array.
__device__ __forceinline__ void pmg_copy_run(const uint32_t *base, uint64_t n, uint64_t at, uint32_t *out, uint32_t len,
                                             uint32_t tid) {
    const uint32_t *src = base + at;
    const uint32_t head = min(len, (uint32_t)((4u - (((uintptr_t)out >> 2) & 3u)) & 3u));
    const uint32_t nvec = (len - head) >> 2, tail = head + 4u * nvec;
    const uint32_t r = (uint32_t)(((uintptr_t)(src + head) >> 2) & 3u);  // entries past a 16-byte boundary
    for (uint32_t g = tid; g < nvec; g += PMG_WG) {
        const uint32_t i = head + 4u * g;
        uint4 v;
        if (r == 0u) {
            v = *(const uint4 *)(src + i);
        } else if (at + i >= r && at + i - r + 8u <= n) {
            const uint4 *p = (const uint4 *)(src + i - r);
            const uint4 x = p[0], y = p[1];
            v = r == 1u ? make_uint4(x.y, x.z, x.w, y.x) : r == 2u ? make_uint4(x.z, x.w, y.x, y.y) : make_uint4(x.w, y.x, y.y, y.z);
        } else {
            v = make_uint4(src[i], src[i + 1u], src[i + 2u], src[i + 3u]);
        }
        *(uint4 *)(out + i) = v;
    }
    if (tid < head) out[tid] = src[tid];
    if (tid >= 64u && tail + (tid - 64u) < len) out[tail + (tid - 64u)] = src[tail + (tid - 64u)];
}

__global__ __launch_bounds__(PMG_WG) void k_pmerge_copy(PMergePlan A) {
    __shared__ uint32_t s_w[2];
    __shared__ uint32_t s_rel[PMG_LDS_WORDS + 1], s_dst[PMG_LDS_WORDS];
    const uint32_t tid = threadIdx.x;
    // the shard of this tile: the last s with tile0 <= blockIdx.x (a shard without entries has no tile)
    uint32_t s = 0;
    for (uint32_t lo = 0, hi = A.n_shards; hi - lo > 1u;) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (A.sh[m].tile0 <= blockIdx.x) s = lo = m;
        else hi = m;
    }
    const PMergeShard S = A.sh[s];
    const uint64_t t0 = (uint64_t)(blockIdx.x - S.tile0) * MRG_PMERGE_TILE;
    if (t0 >= S.n) return;  // (not with the host's tile0; keeps the reads inside the shard whatever was copied)
    const uint64_t t1 = min(t0 + MRG_PMERGE_TILE, S.n);
    const uint32_t nw = (uint32_t)A.n_words;
    if (tid < 2u) s_w[tid] = mrg_last_le(S.off, 0u, nw, tid ? t1 - 1u : t0);
    __syncthreads();
    const uint32_t w0 = s_w[0], w1 = s_w[1];
    const uint32_t *dst = A.dst + (uint64_t)s * A.n_words;
    if (w0 == w1) {  // a shifted copy
        const uint64_t d0 = (uint64_t)dst[w0] + (t0 - S.off[w0]);
        pmg_copy_run(S.docs, S.n, t0, A.docs + d0, (uint32_t)(t1 - t0), tid);
        if (A.tf) pmg_copy_run(S.tf, S.n, t0, A.tf + d0, (uint32_t)(t1 - t0), tid);
        return;
    }
    // several words: their offsets (relative to the first word's) and places go to LDS when they fit, which a tile
    // of single postings does; a tile that also spans empty words beyond that searches the offsets in memory
    const uint32_t span = w1 - w0 + 1u;
    const bool lds = span <= PMG_LDS_WORDS;
    const uint64_t o0 = S.off[w0];
    if (lds) {
        for (uint32_t i = tid; i <= span; i += PMG_WG) s_rel[i] = (uint32_t)(S.off[w0 + i] - o0);  // (w1 + 1 <= words)
        for (uint32_t i = tid; i < span; i += PMG_WG) s_dst[i] = dst[w0 + i];
        __syncthreads();
    }
    uint32_t dv[PMG_IPT], tv[PMG_IPT];  // the tile's entries of this thread, all loads in flight before the searches
#pragma unroll
    for (int k = 0; k < PMG_IPT; ++k) {
        const uint64_t pos = t0 + (uint64_t)k * PMG_WG + tid;
        dv[k] = pos < t1 ? S.docs[pos] : 0u;
        tv[k] = pos < t1 && A.tf ? S.tf[pos] : 0u;
    }
    uint32_t i = 0;  // the word, counted from w0: words ascend with the entries of a thread
#pragma unroll
    for (int k = 0; k < PMG_IPT; ++k) {
        const uint64_t pos = t0 + (uint64_t)k * PMG_WG + tid;
        if (pos >= t1) break;
        uint64_t d;
        if (lds) {
            const uint32_t p = (uint32_t)(pos - o0);
            uint32_t b = span;  // s_rel[i] <= p < s_rel[span]: off[w1 + 1] > t1 - 1 >= pos
            while (b - i > 1u) {
                const uint32_t m = i + ((b - i) >> 1);
                if (s_rel[m] <= p) i = m;
                else b = m;
            }
            d = (uint64_t)s_dst[i] + (p - s_rel[i]);
        } else {
            const uint32_t w = mrg_last_le(S.off, w0 + i, w1 + 1u, pos);
            i = w - w0;
            d = (uint64_t)dst[w] + (pos - S.off[w]);
        }
        A.docs[d] = dv[k];
        if (A.tf) A.tf[d] = tv[k];
    }
}

}  // namespace

void mrg_pmerge_launch_sum(const PMergePlan &p, hipStream_t s) {
    hipLaunchKernelGGL(k_pmerge_sum, dim3(grid_for(p.n_words + 1, PMG_WG)), dim3(PMG_WG), 0, s, p);
}

void mrg_pmerge_launch_place(const PMergePlan &p, hipStream_t s) {
    if (!p.n_words) return;
    hipLaunchKernelGGL(k_pmerge_place, dim3(grid_for(p.n_words, PMG_WG)), dim3(PMG_WG), 0, s, p);
}

void mrg_pmerge_launch_copy(const PMergePlan &p, hipStream_t s) {
    if (!p.n_tiles) return;
    hipLaunchKernelGGL(k_pmerge_copy, dim3((unsigned)p.n_tiles), dim3(PMG_WG), 0, s, p);
}
