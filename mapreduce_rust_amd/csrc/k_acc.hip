// k_acc.hip -- the job's accumulator: a key table that outlives one map call (gfx950; DESIGN.md
// section 18).
//
// mrg_job_map_add maps one batch with the ordinary map + aggregation, which leaves the batch's distinct
// keys as a dense KeySet (counts summed, SipHash partition attached).  The kernels here fold such a
// KeySet into a persistent open-addressing table in HBM (SoA: k0, k1, 64-bit count, doc, partition;
// power-of-two capacity, load kept at or below 1/2 by the host), and turn the table back into a dense
// KeySet for the consumers:
//   k_acc_fold    one batch key per lane: insert-or-add.  A batch's keys are distinct, so no two lanes
//                 add to one key; they do race for empty slots, so slots are claimed word by word with
//                 the monotone CAS protocol of k_keys.hip table_add (k0, then k1, then doc: a slot whose
//                 words all equal the key is the key's slot for good).  Touches O(batch keys) slots.
//   k_acc_rehash  every full slot of the old table into a larger one (the only pass, beside the emit,
//                 that walks the table).
//   k_acc_emit    the full slots as a dense KeySet (len from the packed key, hoff = MRG_NO_HEAP).
//   k_acc_long    the batch's long keys (> 16 bytes) as long items over the concatenated heap; they are
//                 kept beside the table and re-grouped by the existing long-key path (mrg_agg.cpp acc_fold).
// Conventions (as k_topk.hip): wave64; every ballot / workgroup barrier is reached by all lanes -- lanes
// out of range are predicated off, never returned early; probe loops diverge per lane and reconverge
// before the next cross-lane operation; no scratch.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int ACC_WG = 256;
constexpr int ACC_NW = ACC_WG / 64;

inline unsigned acc_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + ACC_WG - 1) / ACC_WG); }

// first probe slot: the truncated hash (MRG_FLAG_DEBUG_HASH_BITS) picks the slot only, identity is
// always the full key (and doc)
__device__ __forceinline__ uint64_t acc_slot0(const AccTable &T, uint64_t a, uint64_t b, uint32_t d) {
    uint64_t h = mrg_key_mix(a, b, d);
    if (T.hash_bits) h &= (1ull << T.hash_bits) - 1u;
    return (h ^ (h >> 31)) & (T.cap - 1);
}

// Add c to key (a, b[, d]) of partition `part`, claiming a slot when the key is new.  Returns true when
// this call created the key (its last claiming CAS found the empty value).  `act` = false: no memory
// access at all.  Triangular probing reaches every slot of the power-of-two table; the host keeps the
// load at or below 1/2, so an empty slot always exists.
__device__ __forceinline__ bool acc_add(const AccTable &T, bool act, uint64_t a, uint64_t b, uint32_t d, uint64_t c,
                                        uint32_t part, bool idx) {
    bool fresh = false;
    if (act) {
        uint64_t slot = acc_slot0(T, a, b, d);
        for (uint64_t probe = 0; probe < T.cap; ++probe) {
            const unsigned long long x = atomicCAS((unsigned long long *)&T.k0[slot], MRG_EMPTY_K0, (unsigned long long)a);
            if (x == MRG_EMPTY_K0 || x == a) {
                const unsigned long long y =
                    atomicCAS((unsigned long long *)&T.k1[slot], MRG_EMPTY_K1, (unsigned long long)b);
                if (y == MRG_EMPTY_K1 || y == b) {
                    bool ok = true;
                    bool made = y == MRG_EMPTY_K1;
                    if (idx) {
                        const unsigned int z = atomicCAS(&T.doc[slot], MRG_EMPTY_DOC, d);
                        ok = z == MRG_EMPTY_DOC || z == d;
                        made = z == MRG_EMPTY_DOC;
                    }
                    if (ok) {
                        if (made) T.part[slot] = part;  // (one creator per slot; read by later kernels only)
                        atomicAdd((unsigned long long *)&T.cnt[slot], (unsigned long long)c);
                        fresh = made;
                        break;
                    }
                }
            }
            slot = (slot + probe + 1u) & (T.cap - 1);
        }
    }
    return fresh;
}

// keys created by this wave -> *created (one atomic per wave); reached by every lane
__device__ __forceinline__ void acc_count(unsigned long long *created, bool fresh) {
    const uint64_t m = __ballot(fresh);
    if (m && __lane_id() == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(created, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(ACC_WG) void k_acc_clear(AccTable T) {
    const uint64_t i = (uint64_t)blockIdx.x * ACC_WG + threadIdx.x;
    if (i < T.cap) {
        T.k0[i] = MRG_EMPTY_K0;
        T.k1[i] = MRG_EMPTY_K1;
        T.cnt[i] = 0ull;
        T.doc[i] = MRG_EMPTY_DOC;
        T.part[i] = 0u;
    }
}

__global__ __launch_bounds__(ACC_WG) void k_acc_fold(AccTable T, KeySet ks, uint64_t n, bool idx,
                                                    unsigned long long *created) {
    const uint64_t i = (uint64_t)blockIdx.x * ACC_WG + threadIdx.x;
    const bool act = i < n && ks.len[i] <= 16u;  // long keys are kept beside the table (k_acc_long)
    uint64_t a = 0, b = 0, c = 0;
    uint32_t d = MRG_EMPTY_DOC, p = 0;
    if (act) {
        a = ks.k0[i];
        b = ks.k1[i];
        c = ks.cnt[i];
        p = ks.part[i];
        if (idx) d = ks.doc[i];
    }
    const bool fresh = acc_add(T, act, a, b, d, c, p, idx);
    acc_count(created, fresh);
}

__global__ __launch_bounds__(ACC_WG) void k_acc_rehash(AccTable O, AccTable T, bool idx) {
    const uint64_t i = (uint64_t)blockIdx.x * ACC_WG + threadIdx.x;
    uint64_t a = MRG_EMPTY_K0, b = 0, c = 0;
    uint32_t d = MRG_EMPTY_DOC, p = 0;
    if (i < O.cap) {
        a = O.k0[i];
        b = O.k1[i];
        c = O.cnt[i];
        d = O.doc[i];
        p = O.part[i];
    }
    (void)acc_add(T, a != MRG_EMPTY_K0, a, b, d, c, p, idx);
}

__global__ __launch_bounds__(ACC_WG) void k_acc_emit(AccTable T, bool idx, KeySet out, uint64_t out_cap,
                                                    unsigned long long *counter) {
    __shared__ uint32_t s_w[ACC_NW];
    __shared__ unsigned long long s_base;
    static_assert(sizeof(uint32_t) * ACC_NW + sizeof(unsigned long long) <= 64 * 1024, "k_acc_emit LDS");
    const uint64_t i = (uint64_t)blockIdx.x * ACC_WG + threadIdx.x;
    uint64_t a = MRG_EMPTY_K0;
    if (i < T.cap) a = T.k0[i];
    const bool full = a != MRG_EMPTY_K0;
    const uint64_t j = mrg_wg_append<ACC_WG>(counter, full, s_w, &s_base);
    if (full && j < out_cap) {
        const uint64_t b = T.k1[i];
        out.k0[j] = a;
        out.k1[j] = b;
        out.cnt[j] = T.cnt[i];
        out.doc[j] = idx ? T.doc[i] : MRG_EMPTY_DOC;
        out.len[j] = mrg_short_len(a, b);
        out.part[j] = T.part[i];
        out.hoff[j] = MRG_NO_HEAP;
    }
}

// the long keys of a KeySet as long items [first + j] over a heap in which the KeySet's heap starts at
// heap_base; *counter (zeroed) = their number
__global__ __launch_bounds__(ACC_WG) void k_acc_long(KeySet ks, uint64_t n, uint64_t heap_base, uint64_t first,
                                                    uint64_t cap, uint64_t *start, uint32_t *rawlen, uint32_t *doc,
                                                    uint64_t *cnt, unsigned long long *counter) {
    const uint64_t i = (uint64_t)blockIdx.x * ACC_WG + threadIdx.x;
    const bool lng = i < n && ks.len[i] > 16u;
    const uint64_t m = __ballot(lng);
    unsigned long long base = 0;
    const int leader = m ? __ffsll((long long)m) - 1 : 0;
    if (m && (int)__lane_id() == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    const uint64_t j = first + base + (uint64_t)__popcll(m & mrg_lanemask_lt());
    if (lng && j < cap) {
        start[j] = heap_base + ks.hoff[i];
        rawlen[j] = ks.len[i];
        doc[j] = ks.doc[i];
        cnt[j] = ks.cnt[i];
    }
}

}  // namespace

void mrg_acc_launch_clear(const AccTable &t, hipStream_t s) {
    hipLaunchKernelGGL(k_acc_clear, dim3(acc_grid(t.cap)), dim3(ACC_WG), 0, s, t);
}
void mrg_acc_launch_fold(const AccTable &t, KeySet ks, uint64_t n, bool indexer, unsigned long long *created,
                         hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_acc_fold, dim3(acc_grid(n)), dim3(ACC_WG), 0, s, t, ks, n, indexer, created);
}
void mrg_acc_launch_rehash(const AccTable &from, const AccTable &to, bool indexer, hipStream_t s) {
    hipLaunchKernelGGL(k_acc_rehash, dim3(acc_grid(from.cap)), dim3(ACC_WG), 0, s, from, to, indexer);
}
void mrg_acc_launch_emit(const AccTable &t, bool indexer, KeySet out, uint64_t out_cap, unsigned long long *counter,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_acc_emit, dim3(acc_grid(t.cap)), dim3(ACC_WG), 0, s, t, indexer, out, out_cap, counter);
}
void mrg_acc_launch_long(KeySet ks, uint64_t n, uint64_t heap_base, uint64_t first, uint64_t cap, uint64_t *start,
                         uint32_t *rawlen, uint32_t *doc, uint64_t *cnt, unsigned long long *counter, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_acc_long, dim3(acc_grid(n)), dim3(ACC_WG), 0, s, ks, n, heap_base, first, cap, start, rawlen,
                       doc, cnt, counter);
}
