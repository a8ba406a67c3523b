// k_decode.hip -- ids -> text, the inverse of k_encode.hip's encoder (gfx950).
//
// mrg_vocab_decode: every id becomes its word's bytes and one separator byte, ' ' inside a document and
// '\n' after the document's last id.  One wave per chunk of 256 ids, 4 ids per lane (one 16-byte load).
// Three launches, as the encoder's, with no wait between workgroups: order comes from the scan only.
//   count    output bytes of each chunk: the sum of wlen[id] + 1 (wlen: the id-indexed length array of
//            the vocabulary's block); the first id that is not in the vocabulary by atomicMin
//   bound    for every document boundary: the bytes of its chunk's ids before it (+ the scanned chunk
//            base = the document's first output byte)
//   emit     per-id output offsets from a wave scan.  The chunk's output is staged in per-wave LDS in
//            windows of DEC_WIN bytes that are 16-byte aligned in the destination, and every window
//            goes out as 16-byte stores per lane; only the 16-byte granules that the chunk shares with its
//            neighbours (the chunk's first and last bytes) are stored bytewise.  A word of at most 16
//            bytes comes from the id-indexed packed-key array (one 16-byte load per id); a longer word is
//            copied from the vocabulary's text by the whole wave, one window's share at a time, so the
//            LDS a chunk needs does not depend on its words' lengths.
// The document's last ids come from a bitmap (one bit per id) built from the offsets.
// No workgroup barrier, no atomics on the output: waves are independent, LDS is per-wave.  The chunk
// loop, the window loop and the long-word loop have wave-uniform trip counts (no lane leaves before a
// ballot / shuffle); per-lane loops reconverge before every cross-lane step.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int DEC_WG = 256;
constexpr int DEC_NW = DEC_WG / 64;
constexpr uint32_t DEC_WIN = 2048;  // bytes of one LDS window: two 16-byte stores per lane
static_assert(MRG_DEC_CHUNK == 64u * 4u, "4 ids per lane");
static_assert(DEC_WIN % 1024u == 0, "a window is whole rounds of 64 x 16 bytes");

#define DEC_UNK 0xFFFFFFFFu

// workgroups of the chunk loop: 8 per CU (all resident), each wave striding over the chunks
unsigned dec_grid(uint64_t nchunks) {
    static int cus[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int cu = (dev >= 0 && dev < 64) ? cus[dev] : 0;
    if (cu == 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        if (dev >= 0 && dev < 64) cus[dev] = cu;
    }
    const uint64_t need = (nchunks + DEC_NW - 1) / DEC_NW;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cu * 8u));
}

struct DecArgs {
    DecPlan P;
    const uint32_t *wlen;      // [n]
    const uint64_t *pk;        // [2 n]
    const uint8_t *text;
    const uint64_t *line_off;  // [n + 1]
    uint64_t n;
};

// The lane's four ids of a chunk: id[j] at position p0 + j.  present bit j: the position lies in
// [lo, hi) and the id is in the vocabulary (or is UNK with unk bytes to write); len[j] = the bytes of its
// word (0 where not present).  REPORT: an id that is not in the vocabulary goes to *err.
template <bool REPORT>
__device__ __forceinline__ uint32_t dec_load(const DecArgs &A, uint64_t p0, uint32_t (&id)[4], uint32_t (&len)[4]) {
    const DecPlan &P = A.P;
    uint32_t present = 0;
    id[0] = id[1] = id[2] = id[3] = DEC_UNK;
    if (p0 >= P.lo && p0 + 4u <= P.hi) {
        const uint4 v = *reinterpret_cast<const uint4 *>(P.in + p0);
        id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
        present = 0xFu;
    } else if (p0 + 4u > P.lo && p0 < P.hi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t q = p0 + (uint32_t)j;
            if (q >= P.lo && q < P.hi) {
                id[j] = P.in[q];
                present |= 1u << j;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        len[j] = 0;
        if ((present >> j) & 1u) {
            bool ok = true;
            if (id[j] == DEC_UNK) {
                len[j] = P.unk_len;
                ok = P.unk_len != 0u;
            } else if ((uint64_t)id[j] < A.n) {
                len[j] = A.wlen[id[j]];
            } else {
                ok = false;
            }
            if (!ok) {
                present &= ~(1u << j);
                if (REPORT) atomicMin(P.err, (unsigned long long)(p0 + (uint32_t)j));
            }
        }
    }
    return present;
}

enum { DEC_COUNT = 0, DEC_BOUND = 1 };

template <int MODE>
__global__ __launch_bounds__(DEC_WG) void k_dec_count(DecArgs A) {
    const DecPlan &P = A.P;
    const uint32_t wv = threadIdx.x >> 6, lane = __lane_id();
    const uint64_t first = (uint64_t)blockIdx.x * DEC_NW + wv, stride = (uint64_t)gridDim.x * DEC_NW;
    const uint64_t n_items = MODE == DEC_BOUND ? (uint64_t)P.n_docs + 1u : P.nchunks;
    for (uint64_t item = first; item < n_items; item += stride) {
        uint64_t chunk = item, limit = ~0ull;
        if (MODE == DEC_BOUND) {
            limit = P.tok_off[item];
            chunk = limit / MRG_DEC_CHUNK;
        }
        uint64_t sum = 0;
        if (chunk < P.nchunks) {  // (bound: a boundary at the very end may lie past the last chunk)
            const uint64_t p0 = chunk * MRG_DEC_CHUNK + 4u * lane;
            uint32_t id[4], len[4];
            const uint32_t present = dec_load<MODE == DEC_COUNT>(A, p0, id, len);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((present >> j) & 1u) && p0 + (uint32_t)j < limit) sum += (uint64_t)len[j] + 1u;
        }
        sum = mrg_wave_sum(sum);
        if (lane == 0) {
            if (MODE == DEC_COUNT) P.cnt[chunk] = sum;
            else P.out_off[item] = P.cnt[min(chunk, P.nchunks)] + sum;
        }
    }
}

__global__ __launch_bounds__(DEC_WG) void k_dec_emit(DecArgs A) {
    const DecPlan &P = A.P;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[DEC_NW][DEC_WIN];
    const uint32_t wv = threadIdx.x >> 6, lane = __lane_id();
    uint8_t *const so = s_out[wv];
    const uint64_t first = (uint64_t)blockIdx.x * DEC_NW + wv, stride = (uint64_t)gridDim.x * DEC_NW;
    // positions below are byte addresses of the destination, so that a window's 16-byte granules are aligned
    const uint64_t out_lo = (uint64_t)(uintptr_t)P.out, out_hi = out_lo + P.out_n;
    for (uint64_t chunk = first; chunk < P.nchunks; chunk += stride) {
        const uint64_t p0 = chunk * MRG_DEC_CHUNK + 4u * lane;
        uint32_t id[4], len[4];
        const uint32_t present = dec_load<false>(A, p0, id, len);
        const uint32_t last4 = (P.bnd[p0 >> 5] >> (uint32_t)(p0 & 31u)) & 0xFu;  // a document's last id: '\n' after it
        // a short word's bytes (packed), or a long word's address in the vocabulary's text
        uint64_t ka[4], kb[4];
        uint64_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ka[j] = kb[j] = 0;
            if ((present >> j) & 1u) {
                mine += (uint64_t)len[j] + 1u;
                if (id[j] == DEC_UNK) {
                    ka[j] = len[j] <= 16u ? P.unk_k0 : (uint64_t)(uintptr_t)P.unk;
                    kb[j] = P.unk_k1;
                } else if (len[j] <= 16u) {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(A.pk + 2ull * id[j]);
                    ka[j] = v.x;
                    kb[j] = v.y;
                } else {
                    ka[j] = (uint64_t)(uintptr_t)(A.text + A.line_off[id[j]]);
                }
            }
        }
        // ---- where this lane's bytes go (every lane of the wave is here)
        const uint64_t x = mrg_wave_scan_incl(mine);
        const uint64_t total = (uint64_t)__shfl((unsigned long long)x, 63);
        const uint64_t gs = out_lo + P.cnt[chunk], ge = min(gs + total, out_hi);  // the chunk's bytes
        uint64_t at[4];  // first byte of id j
        {
            uint64_t a = gs + (x - mine);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                at[j] = a;
                if ((present >> j) & 1u) a += (uint64_t)len[j] + 1u;
            }
        }
        for (uint64_t w = gs & ~15ull; w < ge; w += DEC_WIN) {  // (wave-uniform)
            const uint64_t we = w + DEC_WIN;
            // ---- short words and separators, by their lane (offsets from the window's first byte)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!((present >> j) & 1u)) continue;
                const int64_t d = (int64_t)(at[j] - w), e = d + (int64_t)len[j];  // the word, its separator
                if (e < 0 || d >= (int64_t)DEC_WIN) continue;
                if (len[j] <= 16u) {
                    const int32_t d32 = (int32_t)d;  // (> -17)
                    for (uint32_t t = 0; t < len[j]; ++t) {
                        const int32_t a = d32 + (int32_t)t;
                        if (a >= 0 && a < (int32_t)DEC_WIN) so[a] = (uint8_t)mrg_key_byte(ka[j], kb[j], t);
                    }
                }
                if (e < (int64_t)DEC_WIN) so[e] = ((last4 >> j) & 1u) ? (uint8_t)'\n' : (uint8_t)' ';
            }
            // ---- long words, by the whole wave: the bytes of each that fall into this window
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool lng = ((present >> j) & 1u) && len[j] > 16u && at[j] + len[j] > w && at[j] < we;
                for (uint64_t m = __ballot(lng); m; m &= m - 1u) {
                    const int src = __builtin_ctzll(m);
                    const uint64_t a0 = (uint64_t)__shfl((unsigned long long)at[j], src);
                    const uint64_t ptr = (uint64_t)__shfl((unsigned long long)ka[j], src);
                    const uint32_t L = (uint32_t)__shfl((int)len[j], src);
                    const uint8_t *from = reinterpret_cast<const uint8_t *>((uintptr_t)ptr);
                    const uint64_t b0 = max(a0, w), b1 = min(a0 + L, we);
                    for (uint64_t a = b0 + lane; a < b1; a += 64u) so[a - w] = from[a - a0];
                }
            }
            mrg_wave_sync_lds();
            // ---- flush: whole 16-byte granules inside the chunk's bytes as one store, the others bytewise
#pragma unroll
            for (uint32_t r = 0; r < DEC_WIN / 1024u; ++r) {
                const uint32_t q = r * 1024u + 16u * lane;
                const uint64_t g = w + q;
                if (g >= gs && g + 16u <= ge) {
                    *reinterpret_cast<uint4 *>((uintptr_t)g) = *reinterpret_cast<const uint4 *>(so + q);
                } else if (g + 16u > gs && g < ge) {
#pragma unroll 1
                    for (uint32_t b = 0; b < 16u; ++b)
                        if (g + b >= gs && g + b < ge) *reinterpret_cast<uint8_t *>((uintptr_t)(g + b)) = so[q + b];
                }
            }
            mrg_wave_sync_lds();  // the next window reuses this wave's LDS
        }
    }
}

// bit p of the bitmap for the last id of every non-empty document
__global__ __launch_bounds__(DEC_WG) void k_dec_bounds(const uint64_t *tok_off, uint32_t n_docs, uint32_t *bnd) {
    const uint64_t i = (uint64_t)blockIdx.x * DEC_WG + threadIdx.x;
    if (i < (uint64_t)n_docs && tok_off[i + 1] > tok_off[i]) {
        const uint64_t p = tok_off[i + 1] - 1u;
        atomicOr(&bnd[p >> 5], 1u << (uint32_t)(p & 31u));
    }
}

DecArgs dec_args(const DecPlan &P, const VocTable &t, const VocWords &w) {
    DecArgs A{};
    A.P = P;
    A.wlen = w.wlen;
    A.pk = w.pk;
    A.text = t.text;
    A.line_off = t.line_off;
    A.n = t.n;
    return A;
}

}  // namespace

uint64_t mrg_dec_bitmap_words(uint64_t nchunks) { return nchunks * (MRG_DEC_CHUNK / 32u) + 8u; }

void mrg_dec_launch_bounds(const DecPlan &P, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_bounds, dim3(grid_for(P.n_docs, DEC_WG)), dim3(DEC_WG), 0, s, P.tok_off, P.n_docs, P.bnd);
}
void mrg_dec_launch_count(const DecPlan &P, const VocTable &t, const VocWords &w, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_count<DEC_COUNT>, dim3(dec_grid(P.nchunks)), dim3(DEC_WG), 0, s, dec_args(P, t, w));
}
void mrg_dec_launch_offsets(const DecPlan &P, const VocTable &t, const VocWords &w, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_count<DEC_BOUND>, dim3(grid_for((uint64_t)P.n_docs + 1, DEC_NW)), dim3(DEC_WG), 0, s,
                       dec_args(P, t, w));
}
void mrg_dec_launch_emit(const DecPlan &P, const VocTable &t, const VocWords &w, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_emit, dim3(dec_grid(P.nchunks)), dim3(DEC_WG), 0, s, dec_args(P, t, w));
}
