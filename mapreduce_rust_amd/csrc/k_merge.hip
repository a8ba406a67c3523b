// k_merge.hip -- search over a sharded index: the collection's statistics from the shards, and the merge of the
// shards' result rows into the collection's top-k (gfx950).
//
// mrg_vocab_stats_add: k_stats_df adds the document frequencies of one shard, df[w] += post_off[w + 1] -
//   post_off[w], one thread per word; an offset that descends is reported (atomicMin of its word) and not added.
//   The document lengths are summed by k_srch_sum (k_search.hip).  Integers only: the order of the shards does
//   not matter.
// mrg_search_merge: k_merge, one workgroup per query.  The row of shard s holds n[s] candidates in the order of
//   the search, score descending, then document ascending; positive floats order as their bit patterns, so the
//   key of a candidate is (~bits, document) and a row's keys ascend strictly.  Every used entry is checked first
//   (a positive score that is no NaN, a key above its predecessor's; atomicMin of the flat index otherwise).
//   The rank of candidate (s, i) in the merged row is i + the number of keys of every other row that stand
//   before it: a binary search per row, counting keys <= in the rows of lower shards and keys < in the rows of
//   higher shards, which makes the shard the last key of the order.  Ranks below k_out are written; a candidate
//   at i >= k_out has a rank >= k_out and is not looked at, and a search stops once its rank reaches k_out.
//   The rows are staged in LDS when the n_shards * k_in cells fit MRG_MERGE_LDS_KEYS keys (k_merge<true>), and
//   read from global memory, which is the L2 after the first touch, otherwise (k_merge<false>).
// No workgroup waits for another; the only atomics take a minimum: no result depends on scheduling.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int STATS_WG = 256;
constexpr int MERGE_WG = 1024;       // the largest workgroup; rows with few candidates take MERGE_WG_SMALL
constexpr int MERGE_WG_SMALL = 256;
static_assert(MRG_MERGE_LDS_KEYS * 8u <= 64u * 1024u, "the staged rows of a query fit 64 KiB of LDS");
static_assert(MRG_SEARCH_MAX_K <= MRG_MERGE_LDS_KEYS, "one full row always takes the LDS path");
static_assert(MRG_SEARCH_MAX_SHARDS <= MERGE_WG_SMALL, "one thread per shard loads the row counts");

__global__ __launch_bounds__(STATS_WG) void k_stats_df(const uint64_t *post_off, uint64_t n_words, unsigned long long *df,
                                                      unsigned long long *err) {
    const uint64_t w = (uint64_t)blockIdx.x * STATS_WG + threadIdx.x;
    if (w >= n_words) return;  // (post_off has n_words + 1 entries)
    const uint64_t a = post_off[w], b = post_off[w + 1];
    if (b < a) atomicMin(err, (unsigned long long)w);
    else df[w] += b - a;  // (one thread per word)
}

// the key of the entry at flat index `at` of the input rows
__device__ __forceinline__ uint64_t merge_key_at(const MergePlan &M, uint64_t at) {
    return ((uint64_t)~M.in_bits[at] << 32) | M.in_docs[at];
}

template <bool LDS>
__global__ __launch_bounds__(MERGE_WG) void k_merge(MergePlan M, uint32_t q0) {
    __shared__ uint64_t s_k[LDS ? MRG_MERGE_LDS_KEYS : 1];
    __shared__ uint32_t s_n[MRG_SEARCH_MAX_SHARDS];
    const uint32_t q = q0 + blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    // (the host has checked every count against k_in; the min keeps the reads inside the rows whatever was copied)
    if (tid < M.n_shards) s_n[tid] = min(M.in_n[(uint64_t)tid * M.n_queries + q], M.k_in);
    __syncthreads();
    // the flat index of cell (s, i): below 2^32 (checked by the host)
    auto flat = [&](uint32_t s, uint32_t i) { return ((uint64_t)s * M.n_queries + q) * M.k_in + i; };

    // ---- every used entry: checked, and staged
    const uint32_t cells = M.n_shards * M.k_in;
    for (uint32_t c = tid; c < cells; c += nt) {
        const uint32_t s = c / M.k_in, i = c - s * M.k_in;
        if (i >= s_n[s]) continue;
        const uint64_t at = flat(s, i), key = merge_key_at(M, at);
        // the bits of a positive float that is no NaN: 1 .. 0x7F800000
        bool bad = M.in_bits[at] - 1u >= 0x7F800000u;
        if (i && merge_key_at(M, at - 1u) >= key) bad = true;
        if (bad) atomicMin(M.err, (unsigned long long)at);
        if (LDS) s_k[c] = key;
    }
    if (LDS) __syncthreads();
    auto key_of = [&](uint32_t s, uint32_t i) { return LDS ? s_k[s * M.k_in + i] : merge_key_at(M, flat(s, i)); };

    // ---- the ranks
    const uint32_t lim = min(M.k_in, M.k_out), cand = M.n_shards * lim;
    uint32_t *od = M.out_docs + (uint64_t)q * M.k_out, *ob = M.out_bits + (uint64_t)q * M.k_out;
    for (uint32_t c = tid; c < cand; c += nt) {
        const uint32_t s = c / lim, i = c - s * lim;
        if (i >= s_n[s]) continue;
        const uint64_t key = key_of(s, i);
        uint32_t rank = i;
        for (uint32_t o = 0; o < M.n_shards && rank < M.k_out; ++o) {
            if (o == s) continue;
            const bool le = o < s;  // an equal key of a lower shard stands before this one
            uint32_t lo = 0, hi = min(s_n[o], M.k_out);  // (k_out keys before it are as good as more)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const uint64_t v = key_of(o, mid);
                if (v < key || (le && v == key)) lo = mid + 1u;
                else hi = mid;
            }
            rank += lo;
        }
        // (a rank is below the number of used entries, so nothing is written from top_n on)
        if (rank < M.k_out) {
            od[rank] = (uint32_t)key;
            ob[rank] = ~(uint32_t)(key >> 32);
        }
    }
}

}  // namespace

void mrg_stats_launch_df(const uint64_t *post_off, uint64_t n_words, unsigned long long *df, unsigned long long *err,
                         hipStream_t s) {
    for (uint64_t at = 0; at < n_words; at += (uint64_t)STATS_WG << 22) {  // (a grid has fewer than 2^31 workgroups)
        const uint64_t n = std::min<uint64_t>(n_words - at, (uint64_t)STATS_WG << 22);
        hipLaunchKernelGGL(k_stats_df, dim3((unsigned)((n + STATS_WG - 1) / STATS_WG)), dim3(STATS_WG), 0, s, post_off + at, n,
                           df + at, err);
    }
}

void mrg_merge_launch(const MergePlan &m, hipStream_t s) {
    const bool lds = (uint64_t)m.n_shards * m.k_in <= MRG_MERGE_LDS_KEYS;
    const unsigned wg = (uint64_t)m.n_shards * std::min(m.k_in, m.k_out) <= 1024u ? MERGE_WG_SMALL : MERGE_WG;
    for (uint64_t q0 = 0; q0 < m.n_queries; q0 += 1u << 30) {  // (a grid has fewer than 2^31 workgroups)
        const unsigned g = (unsigned)std::min<uint64_t>(m.n_queries - q0, 1u << 30);
        if (lds) hipLaunchKernelGGL(k_merge<true>, dim3(g), dim3(wg), 0, s, m, (uint32_t)q0);
        else hipLaunchKernelGGL(k_merge<false>, dim3(g), dim3(wg), 0, s, m, (uint32_t)q0);
    }
}
