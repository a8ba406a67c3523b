// k_encode.hip -- a frozen word -> id table and the text -> id encoder (gfx950).
//
// Vocabulary (mrg_job_vocab): the ranked "word count\n" lines of mrg_job_topk, copied into memory the
// vocabulary owns, plus an open-addressing table (SoA: k0, k1, id; power-of-two capacity, load <= 1/2)
// built by one kernel with the slot-claim protocol of k_acc.hip (k0, then k1, then id, each by CAS).
//   short word (<= 16 bytes)   k0, k1 = the packed key: identity by itself
//   long word                  k0 = 64-bit hash of the bytes (top bit set), k1 = 0xFF tag byte | length
//                              (no packed key holds a 0xFF byte), identity = byte compare against the
//                              vocabulary's own text at line_off[id]
// MRG_FLAG_DEBUG_HASH_BITS truncates the slot hash and the long words' stored hash.
// mrg_vocab_from_text builds the same object from "word count\n" text: k_voc_check (one lane per line:
// the line's form, the word's UTF-8 and \w classes, its length), the same build, then k_voc_verify (every
// word looked up again must find its own line: a word on two lines does not).  k_voc_words fills the
// id-indexed packed words that k_decode.hip reads.
//
// Encode (mrg_vocab_encode): tokens exactly as wc::map makes them (src/app/wc.rs:6-13), in input order.
// One wave per 1 KiB chunk, 16 bytes per lane (one 16-byte load).  Three launches of the same chunk
// routine, tokenizing twice as k_text.hip does:
//   count    tokens (with a non-empty key) starting in each chunk; UTF-8 validation
//   bound    for every document boundary: tokens of its chunk that start before it (+ the scanned
//            chunk base = the document's first output index)
//   emit     ids to out[base of the chunk + rank inside it]
// Byte classes come from SWAR arithmetic on the four loaded words (\w, White_Space, >= 0x80, UTF-8 lead),
// as 16-bit masks per lane.  Token starts: an ASCII non-space byte after an ASCII White_Space byte or at a
// document start is a start for certain (previous lane's last bits through a shuffle); the only other
// candidates -- a non-ASCII lead byte, an ASCII byte right after a non-ASCII byte -- are rare and decided
// exactly (mrg_utf8_decode + mrg_uclass of the codepoint and of the one before it).  Token ends: the next
// ASCII White_Space byte or document start, from the lane's own mask or, through one ballot of the lanes
// that hold one, the next such lane's mask in LDS.  A token without a non-ASCII byte before that end is
// packed from LDS; one with such a byte (it may end earlier, at a non-ASCII White_Space codepoint), or
// longer than 16 key bytes, or running more than 16 bytes past the chunk's end (the one token that crosses
// it gets the next 16 bytes in registers), goes to the exact walker over global memory:
// the fallback is taken per token, inside the wave's chunk.  A token belongs to the chunk (lane) where it
// starts; its owner reads on past the chunk's end to the next White_Space or document end.
// Document boundaries come from a bitmap (one bit per input byte) built from the offsets.
// No workgroup barrier and no wait between workgroups anywhere: waves are independent, LDS is
// per-wave.  Conventions as k_topk.hip / k_acc.hip: the chunk loop's trip count is wave-uniform (no lane
// leaves before a ballot / shuffle), per-lane loops reconverge before every cross-lane step.
#include <algorithm>

#include "mrg_device.h"
#include "mrg_internal.h"

namespace {

constexpr int ENC_WG = 256;
constexpr int ENC_NW = ENC_WG / 64;
constexpr uint32_t ENC_LANE_TOK = 16;  // token starts in one lane's 16 bytes: every byte can start a document

#define VOC_EMPTY_ID 0xFFFFFFFFu
#define VOC_LONG_TAG 0xFF00000000000000ull
#define VOC_UNK 0xFFFFFFFFu

// workgroups of the chunk loop: 8 per CU (all resident), each wave striding over the chunks
unsigned chunk_grid(uint64_t ntiles) {
    static int cus[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int cu = (dev >= 0 && dev < 64) ? cus[dev] : 0;
    if (cu == 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) cu = 256;
        if (dev >= 0 && dev < 64) cus[dev] = cu;
    }
    const uint64_t need = (ntiles + ENC_NW - 1) / ENC_NW;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cu * 8u));
}

// ---------------------------------------------------------------- keys
__device__ __forceinline__ uint64_t voc_fold(uint64_t h, uint64_t w) {
    return mrg_fmix64(h ^ w) + 0x9E3779B97F4A7C15ull;
}

// A key pushed byte by byte: the packed 16-byte prefix and, beyond it, a hash over the key's 8-byte
// big-endian words (zero padded), finished with the length.
struct VocKey {
    uint64_t k0 = 0, k1 = 0, cur = 0, h = 0;
    uint32_t L = 0;
    __device__ __forceinline__ void push(uint32_t b) {
        if (L < 16u) {
            mrg_key_append(k0, k1, L, b);
        } else {
            if (L == 16u) h = voc_fold(voc_fold(0x6d72677675636162ull, k0), k1);
            cur |= (uint64_t)(b & 0xFFu) << (56u - 8u * (L & 7u));
            if ((L & 7u) == 7u) {
                h = voc_fold(h, cur);
                cur = 0;
            }
        }
        ++L;
    }
    // the table words of a long key
    __device__ __forceinline__ uint64_t long_a(uint32_t hash_bits) const {
        uint64_t x = (L & 7u) ? voc_fold(h, cur) : h;
        x = mrg_fmix64(x ^ (uint64_t)L);
        if (hash_bits) x &= (1ull << hash_bits) - 1u;
        return x | (1ull << 63);
    }
    __device__ __forceinline__ uint64_t long_b() const { return VOC_LONG_TAG | (uint64_t)L; }
};

__device__ __forceinline__ uint64_t voc_slot0(const VocTable &T, uint64_t a, uint64_t b) {
    uint64_t h = mrg_key_hash32(a, b, 0u);  // (one 32-bit multiply; tables beyond 2^32 slots only probe longer)
    if (T.hash_bits) h &= (1ull << T.hash_bits) - 1u;
    return h & (T.cap - 1);
}

// ---------------------------------------------------------------- vocabulary build
// line j of the ranked records: its length in bytes ("word count\n"), the word's length, and the number
// of lines kept by min_count (counts descend: the kept lines are a prefix); len64[m] = 0 for the scan
__global__ __launch_bounds__(ENC_WG) void k_voc_lines(const SortRec *top, uint64_t m, KeySet ks, uint64_t min_count,
                                                     uint64_t *len64, uint32_t *wlen, unsigned long long *nkeep) {
    const uint64_t j = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (j == m) len64[j] = 0ull;
    if (j < m) {
        const uint32_t e = top[j].idx;
        const uint64_t c = ks.cnt[e];
        const uint32_t l = ks.len[e];
        len64[j] = (uint64_t)l + 2u + mrg_ndigits(c);
        wlen[j] = l;
        const bool next = j + 1 < m && ks.cnt[top[j + 1].idx] >= min_count;
        if (c >= min_count && !next) *nkeep = j + 1;  // (exactly one such j, or none)
    }
}

__global__ __launch_bounds__(ENC_WG) void k_voc_clear(VocTable T) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i < T.cap) {
        T.k0[i] = MRG_EMPTY_K0;
        T.k1[i] = MRG_EMPTY_K1;
        T.id[i] = VOC_EMPTY_ID;
    }
}

// word i -> slot (key, id = i).  The words are distinct; two long words may still share (hash, length),
// so the id word is claimed too and the loser probes on.  Triangular probing reaches every slot of the
// power-of-two table and the load is at most 1/2: a word that finds no slot is a bug (*fail).
__global__ __launch_bounds__(ENC_WG) void k_voc_insert(VocTable T, const uint32_t *wlen, unsigned long long *fail) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i < T.n) {
        const uint8_t *w = T.text + T.line_off[i];
        const uint32_t L = wlen[i];
        VocKey kb;
        for (uint32_t j = 0; j < L; ++j) kb.push(w[j]);
        const uint64_t a = L <= 16u ? kb.k0 : kb.long_a(T.hash_bits);
        const uint64_t b = L <= 16u ? kb.k1 : kb.long_b();
        uint64_t slot = voc_slot0(T, a, b);
        bool placed = false;
        for (uint64_t probe = 0; probe < T.cap; ++probe) {
            const unsigned long long x = atomicCAS((unsigned long long *)&T.k0[slot], MRG_EMPTY_K0, (unsigned long long)a);
            if (x == MRG_EMPTY_K0 || x == a) {
                const unsigned long long y =
                    atomicCAS((unsigned long long *)&T.k1[slot], MRG_EMPTY_K1, (unsigned long long)b);
                if (y == MRG_EMPTY_K1 || y == b) {
                    const unsigned int z = atomicCAS(&T.id[slot], VOC_EMPTY_ID, (unsigned int)i);
                    if (z == VOC_EMPTY_ID) {
                        placed = true;
                        break;
                    }
                }
            }
            slot = (slot + probe + 1u) & (T.cap - 1);
        }
        if (!placed) atomicAdd(fail, 1ull);
    }
}

// The id-indexed packed words of mrg_vocab_decode: the first 16 bytes of word i as (k0, k1).
__global__ __launch_bounds__(ENC_WG) void k_voc_words(VocTable T, VocWords W) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i < T.n) {
        const uint8_t *w = T.text + T.line_off[i];
        const uint32_t L = min(W.wlen[i], 16u);
        uint64_t k0 = 0, k1 = 0;
        for (uint32_t j = 0; j < L; ++j) mrg_key_append(k0, k1, j, w[j]);
        W.pk[2 * i] = k0;
        W.pk[2 * i + 1] = k1;
    }
}

// ---------------------------------------------------------------- encode
struct EncArgs {
    const uint8_t *in;        // 16-byte aligned; positions below are byte offsets from it
    uint64_t lo, hi;          // the documents' bytes are [lo, hi); lo < 1024
    uint64_t ntiles;          // 1 KiB chunks over [0, hi)
    const uint32_t *bnd;      // bit p set: a document starts (or the input ends) at byte p
    const uint64_t *doc_off;  // [n_docs + 1]
    uint32_t n_docs;
    uint64_t *cnt;            // [ntiles + 1] count: tokens per chunk; afterwards scanned in place
    uint64_t *tok_off;        // [n_docs + 1] bound: first output index of each document
    uint32_t *out;            // emit
    uint64_t out_n;           // ids the count pass found (= the scanned total): nothing is written beyond
    unsigned long long *err;  // first invalid byte (atomicMin)
    unsigned long long *info; // [0] tokens [1] UNK [2] long tokens [3] non-ASCII chunks [4] table probes
};

enum { ENC_COUNT = 0, ENC_EMIT = 1, ENC_BOUND = 2 };

__device__ __forceinline__ bool bnd_bit(const EncArgs &A, uint64_t p) {
    return (A.bnd[p >> 5] >> (uint32_t)(p & 31u)) & 1u;
}
// a document boundary inside the codepoint [p, p + l)
__device__ __forceinline__ bool bnd_inside(const EncArgs &A, uint64_t p, int l) {
    bool b = false;
    for (int j = 1; j < l; ++j) b = b || bnd_bit(A, p + (uint64_t)j);
    return b;
}

// Is the codepoint before p White_Space (or does a document start at p)?  Exact.
__device__ __forceinline__ bool prev_space(const EncArgs &A, uint64_t p) {
    if (p <= A.lo || bnd_bit(A, p)) return true;
    const uint32_t b = A.in[p - 1];
    if (b < 0x80u) return (b - 9u < 5u) | (b == 0x20u);
    uint32_t k = 1;
    while (k <= 3u && p >= A.lo + k + 1u && mrg_is_cont(A.in[p - k])) ++k;
    if (k > 4u || p < A.lo + k) return false;
    const uint64_t q = p - k;
    auto rd = [&](uint64_t x) -> uint32_t { return A.in[x]; };
    uint32_t cp, raw;
    const int l = mrg_utf8_decode(rd, q, A.hi, &cp, &raw);
    if (l == 0 || q + (uint64_t)l != p) return false;  // invalid: reported by the chunk that holds it
    return mrg_uclass(cp) == MRG_CLS_S;
}

// Table lookup; same(id) decides a long candidate.  Read-only: the table is complete.
template <class SAME>
__device__ __forceinline__ uint32_t voc_find(const VocTable &T, uint64_t a, uint64_t b, bool lng, SAME &&same,
                                             uint32_t &probes) {
    uint64_t slot = voc_slot0(T, a, b);
    uint32_t id = VOC_UNK;
    for (uint64_t probe = 0; probe < T.cap; ++probe) {
        ++probes;
        // (the three words of the slot are loaded together: one memory latency per probe, not three)
        const uint64_t x = T.k0[slot], y = T.k1[slot];
        const uint32_t cand = T.id[slot];
        if (x == MRG_EMPTY_K0) break;
        if (x == a && y == b) {
            if (!lng || same(cand)) {
                id = cand;
                break;
            }
        }
        slot = (slot + probe + 1u) & (T.cap - 1);
    }
    return id;
}

struct EncStat {
    uint32_t tokens = 0, unk = 0, lng = 0, probes = 0;
};

// The walker's view of the input and of the boundary bitmap: one aligned word at a time, kept in
// registers (a token's bytes are 1-2 loads instead of one dependent load per byte).
struct ByteRd {
    const uint8_t *in;
    uint64_t hi;
    mutable uint64_t idx, w;
    __device__ __forceinline__ ByteRd(const uint8_t *p, uint64_t end) : in(p), hi(end), idx(~0ull), w(0) {}
    __device__ __forceinline__ uint32_t operator()(uint64_t x) const {
        const uint64_t i = x >> 3;
        if (i != idx) {
            idx = i;
            if ((i << 3) + 8u <= hi) {
                w = *reinterpret_cast<const uint64_t *>(in + (i << 3));
            } else {  // the input's last, partial word: bytewise, nothing read at or beyond hi
                w = 0;
                for (uint64_t q = i << 3; q < hi; ++q) w |= (uint64_t)in[q] << (8u * (uint32_t)(q & 7u));
            }
        }
        return (uint32_t)(w >> (8u * (uint32_t)(x & 7u))) & 0xFFu;
    }
};
struct BndRd {
    const uint32_t *b;
    mutable uint64_t idx;
    mutable uint32_t w;
    __device__ __forceinline__ explicit BndRd(const uint32_t *p) : b(p), idx(~0ull), w(0) {}
    __device__ __forceinline__ bool operator()(uint64_t p) const {
        const uint64_t i = p >> 5;
        if (i != idx) {
            idx = i;
            w = b[i];
        }
        return (w >> (uint32_t)(p & 31u)) & 1u;
    }
};

// The token starting at byte a, walked exactly over global memory to the next White_Space codepoint,
// document boundary or the end of the input.  Returns whether its key is non-empty; FULL: *id = its id.
template <bool FULL>
__device__ __forceinline__ bool tok_slow(const EncArgs &A, const VocTable &T, uint64_t a, uint32_t *id, EncStat &st) {
    const ByteRd rd(A.in, A.hi);
    const BndRd bnd(A.bnd);
    VocKey kb;
    uint64_t p = a;
    while (p < A.hi) {
        if (p > a && bnd(p)) break;
        uint32_t cp, raw;
        const int l = mrg_utf8_decode(rd, p, A.hi, &cp, &raw);
        if (!l) break;  // invalid: reported by the count pass of its chunk
        bool cut = false;  // a document boundary inside the codepoint (invalid too)
        for (int j = 1; j < l; ++j) cut = cut || bnd(p + (uint64_t)j);
        if (cut) break;
        const uint32_t cl = mrg_uclass(cp);
        if (cl == MRG_CLS_S) break;
        if (cl == MRG_CLS_W) {
            if (!FULL) return true;
            for (int b = 0; b < l; ++b) kb.push((raw >> (8 * b)) & 0xFFu);
        }
        p += (uint64_t)l;
    }
    if (kb.L == 0u) return false;
    if (kb.L <= 16u) {
        *id = voc_find(T, kb.k0, kb.k1, false, [](uint32_t) { return true; }, st.probes);
    } else {
        ++st.lng;
        const uint64_t e = p;
        auto same = [&](uint32_t cand) -> bool {  // the key's bytes against the vocabulary's own copy
            const uint8_t *w = T.text + T.line_off[cand];
            const ByteRd rd2(A.in, A.hi);
            uint32_t j = 0;
            bool eq = true;
            for (uint64_t q = a; q < e && eq;) {
                uint32_t cp, raw;
                int l = mrg_utf8_decode(rd2, q, e, &cp, &raw);
                if (!l) l = 1;  // (walked once already)
                if (mrg_uclass(cp) == MRG_CLS_W)
                    for (int b = 0; b < l; ++b) eq = eq && w[j++] == (uint8_t)(raw >> (8 * b));
                q += (uint64_t)l;
            }
            return eq;
        };
        *id = voc_find(T, kb.long_a(T.hash_bits), kb.long_b(), true, same, st.probes);
    }
    return true;
}

// top bit of every byte of m -> 4 bits (byte j -> bit j)
__device__ __forceinline__ uint32_t msb4(uint32_t m) { return (((m & 0x80808080u) >> 7) * 0x10204080u) >> 28; }
// per byte of x7 (bytes < 0x80): 0x80 where lo <= byte < hi
__device__ __forceinline__ uint32_t in_range(uint32_t x7, uint32_t lo, uint32_t hi) {
    const uint32_t y = x7 | 0x80808080u;
    return (y - lo * 0x01010101u) & ~(y - hi * 0x01010101u);
}

// 16-bit masks of the 16 bytes in w[0..4): \w and White_Space (ASCII bytes only), byte >= 0x80, UTF-8 lead
__device__ __forceinline__ void classes16(const uint32_t (&w)[4], uint32_t &W16, uint32_t &S16, uint32_t &H16,
                                          uint32_t &L16) {
    W16 = S16 = H16 = L16 = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x7 = w[k] & 0x7F7F7F7Fu, lc = x7 | 0x20202020u;
        const uint32_t wm = in_range(x7, '0', '9' + 1) | in_range(lc, 'a', 'z' + 1) | in_range(x7, '_', '_' + 1);
        const uint32_t sm = in_range(x7, 9, 14) | in_range(x7, 0x20, 0x21);
        W16 |= msb4(wm & ~w[k]) << (4 * k);
        S16 |= msb4(sm & ~w[k]) << (4 * k);
        H16 |= msb4(w[k]) << (4 * k);
        L16 |= msb4(w[k] & (w[k] << 1)) << (4 * k);  // 11xxxxxx
    }
}

// any bit of the per-lane 16-bit masks m[0..64) set at chunk positions [q, e)
__device__ __forceinline__ bool any_bit(const uint16_t *m, uint32_t q, uint32_t e) {
    bool any = false;
    for (uint32_t pos = q; pos < e && !any;) {
        const uint32_t sh = pos & 15u, span = min(16u - sh, e - pos);
        any = (((uint32_t)m[pos >> 4] >> sh) & ((1u << span) - 1u)) != 0u;
        pos += span;
    }
    return any;
}

template <int MODE>
__global__ __launch_bounds__(ENC_WG) void k_enc(EncArgs A, VocTable T) {
    // the chunk's bytes, word k of lane l at [k * 64 + l] (lanes reading near their own bytes hit distinct
    // banks); the ids of a lane's tokens, token i of lane l at [i * 64 + l]
    __shared__ uint32_t s_b[ENC_NW][256];
    __shared__ uint16_t s_brk[ENC_NW][64], s_w[ENC_NW][64], s_h[ENC_NW][64];
    __shared__ uint32_t s_ids[ENC_NW][64 * ENC_LANE_TOK];
    static_assert(sizeof(uint32_t) * ENC_NW * 256 + 3 * sizeof(uint16_t) * ENC_NW * 64 +
                          sizeof(uint32_t) * ENC_NW * 64 * ENC_LANE_TOK <= 64 * 1024, "k_enc LDS");
    const uint32_t wv = threadIdx.x >> 6, lane = __lane_id();
    // A wave takes chunks first, first + stride, ...: everything in the loop is wave-uniform control flow,
    // and the diagnostics cost one set of atomics per wave, not per chunk.
    const uint64_t first = (uint64_t)blockIdx.x * ENC_NW + wv, stride = (uint64_t)gridDim.x * ENC_NW;
    const uint64_t n_items = MODE == ENC_BOUND ? (uint64_t)A.n_docs + 1u : A.ntiles;
    EncStat st;
    uint32_t n_tok = 0, n_na = 0;
    for (uint64_t item = first; item < n_items; item += stride) {
    uint64_t tile = item, limit = ~0ull;
    if (MODE == ENC_BOUND) {
        limit = A.doc_off[item];
        tile = limit >> 10;
    }
    const bool have = tile < A.ntiles;  // (bound: a boundary at the very end may lie past the last chunk)
    const uint64_t t0 = tile << 10, p0 = t0 + 16u * lane;
    uint32_t nv = 0;  // tokens of this lane
    bool nonascii = false;
    if (have) {
        // ---- load: one 16-byte load per lane; bytes outside [lo, hi) read as spaces
        uint32_t w[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
        if (p0 >= A.lo && p0 + 16u <= A.hi) {
            const uint4 v = *reinterpret_cast<const uint4 *>(A.in + p0);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if (p0 + 16u > A.lo && p0 < A.hi) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t x = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t q = p0 + 4u * k + j;
                    const uint32_t c = (q >= A.lo && q < A.hi) ? A.in[q] : 0x20u;
                    x |= c << (8 * j);
                }
                w[k] = x;
            }
        }
        // ---- classes by arithmetic: \w, White_Space (exact for bytes < 0x80), >= 0x80, UTF-8 lead bytes
        uint32_t W16, S16, H16, L16;
        classes16(w, W16, S16, H16, L16);
        const uint32_t B16 = (A.bnd[p0 >> 5] >> (uint32_t)(p0 & 31u)) & 0xFFFFu;
        nonascii = __ballot(H16 != 0u) != 0ull;
        // ---- the byte before each byte: the previous lane's last bit (lane 0: the byte before the chunk)
        const uint32_t upS = (uint32_t)__shfl_up((int)S16, 1), upH = (uint32_t)__shfl_up((int)H16, 1);
        uint32_t cS = (upS >> 15) & 1u, cH = (upH >> 15) & 1u;
        if (lane == 0) {
            cS = 1u;
            cH = 0u;
            if (t0 > A.lo) {
                const uint32_t pb = A.in[t0 - 1];
                cH = pb >> 7;
                cS = ((pb - 9u < 5u) | (pb == 0x20u)) ? 1u : 0u;
            }
        }
        const uint32_t prevS = ((S16 << 1) | cS) & 0xFFFFu, prevH = ((H16 << 1) | cH) & 0xFFFFu;
        const uint32_t brk = S16 | B16;  // ASCII White_Space and document starts: every token ends at or before one
        // certain starts: an ASCII non-space byte after an ASCII White_Space byte or at a document start
        uint32_t T16 = ~S16 & ~H16 & (prevS | B16) & 0xFFFFu;
        // to be decided exactly (rare): a non-ASCII lead byte, or an ASCII non-space byte after a non-ASCII byte
        uint32_t U16 = ((H16 & L16) | (~S16 & ~H16 & prevH & ~B16)) & 0xFFFFu;
        auto rd = [&](uint64_t x) -> uint32_t { return A.in[x]; };
        if (MODE == ENC_COUNT) {
            // str::from_utf8 acceptance by byte (k_text.hip k_utf8_check), per document
            for (uint32_t hb = H16; hb; hb &= hb - 1u) {
                const uint64_t i = p0 + (uint32_t)__builtin_ctz(hb);
                const uint32_t b = A.in[i];
                if (!mrg_is_cont(b)) {
                    uint32_t cp, raw;
                    const int l = mrg_utf8_decode(rd, i, A.hi, &cp, &raw);
                    if (!l || bnd_inside(A, i, l)) atomicMin(A.err, (unsigned long long)i);
                    continue;
                }
                uint32_t k = 1;
                while (k <= 3u && i >= A.lo + k && mrg_is_cont(A.in[i - k])) ++k;
                if (k > 3u || i < A.lo + k || (uint32_t)mrg_utf8_len(A.in[i - k]) <= k)
                    atomicMin(A.err, (unsigned long long)i);
            }
        }
        for (; U16; U16 &= U16 - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(U16);
            const uint64_t p = p0 + j;
            bool start = true;
            if ((H16 >> j) & 1u) {  // the codepoint itself may be White_Space (or invalid: reported by the count pass)
                uint32_t cp, raw;
                const int l = mrg_utf8_decode(rd, p, A.hi, &cp, &raw);
                start = l && mrg_uclass(cp) != MRG_CLS_S;
            }
            if (start && prev_space(A, p)) T16 |= 1u << j;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_b[wv][k * 64 + lane] = w[k];
        s_brk[wv][lane] = (uint16_t)brk;
        s_w[wv][lane] = (uint16_t)W16;
        s_h[wv][lane] = (uint16_t)H16;
        const uint64_t LB = __ballot(brk != 0u);
        mrg_wave_sync_lds();
        while (T16) {  // (per lane; reconverges before the scan below)
            const uint32_t j = (uint32_t)__builtin_ctz(T16);
            T16 &= T16 - 1u;
            const uint32_t q = 16u * lane + j;
            if (MODE == ENC_BOUND && t0 + q >= limit) break;
            const uint32_t own = brk & ~((2u << j) - 1u);
            int e = -1;  // the first ASCII White_Space byte / document start after q inside the chunk
            if (own) {
                e = (int)(16u * lane + (uint32_t)__builtin_ctz(own));
            } else {
                const uint64_t m = lane == 63u ? 0ull : LB & (~0ull << (lane + 1u));
                if (m) {
                    const uint32_t l2 = (uint32_t)__builtin_ctzll(m);
                    e = (int)(16u * l2 + (uint32_t)__builtin_ctz((uint32_t)s_brk[wv][l2]));
                }
            }
            bool valid = false;
            uint32_t id = VOC_UNK;
            // A token that runs to the chunk's end (at most one per chunk): the next 16 bytes in registers.
            // If they hold its end with no non-ASCII byte before it, the token stays on the fast path.
            uint32_t tw[4] = {0u, 0u, 0u, 0u}, tW = 0u, tail = 0u;
            bool slow = e >= 0 && any_bit(s_h[wv], q, (uint32_t)e);
            if (e < 0) {
                slow = true;
                // (emit only: the count pass needs just the first \w byte, which the walker finds at once)
                if (MODE == ENC_EMIT && t0 + 1040u <= A.hi && !any_bit(s_h[wv], q, 1024u)) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(A.in + t0 + 1024u);
                    tw[0] = v.x; tw[1] = v.y; tw[2] = v.z; tw[3] = v.w;
                    uint32_t tS, tH, tL;
                    classes16(tw, tW, tS, tH, tL);
                    const uint32_t tb = tS | (A.bnd[(t0 + 1024u) >> 5] & 0xFFFFu);
                    if (tb) {
                        tail = (uint32_t)__builtin_ctz(tb);
                        if ((tH & ((1u << tail) - 1u)) == 0u) {
                            slow = false;
                            e = 1024;
                        }
                    }
                }
            }
            if (slow) {
                // runs on beyond those bytes, or holds non-ASCII bytes (it may end earlier, at a non-ASCII
                // White_Space codepoint): the exact walker
                valid = tok_slow<MODE == ENC_EMIT>(A, T, t0 + q, &id, st);
            } else if (MODE != ENC_EMIT) {
                valid = any_bit(s_w[wv], q, (uint32_t)e) || (tW & ((1u << tail) - 1u)) != 0u;
            } else {
                uint64_t k0 = 0, k1 = 0;
                uint32_t L = 0;
                for (uint32_t pos = q; pos < (uint32_t)e && L <= 16u; ++pos)
                    if (((uint32_t)s_w[wv][pos >> 4] >> (pos & 15u)) & 1u) {
                        if (L < 16u)
                            mrg_key_append(k0, k1, L, (s_b[wv][((pos >> 2) & 3u) * 64u + (pos >> 4)] >> (8u * (pos & 3u))) & 0xFFu);
                        ++L;
                    }
                for (uint32_t j = 0; j < tail && L <= 16u; ++j)
                    if ((tW >> j) & 1u) {
                        const uint32_t x = j < 8u ? (j < 4u ? tw[0] : tw[1]) : (j < 12u ? tw[2] : tw[3]);
                        if (L < 16u) mrg_key_append(k0, k1, L, (x >> (8u * (j & 3u))) & 0xFFu);
                        ++L;
                    }
                if (L > 16u) {
                    valid = tok_slow<true>(A, T, t0 + q, &id, st);
                } else if (L) {
                    valid = true;
                    id = voc_find(T, k0, k1, false, [](uint32_t) { return true; }, st.probes);
                }
            }
            if (valid) {
                if (MODE == ENC_EMIT) s_ids[wv][nv * 64u + lane] = id;
                st.unk += id == VOC_UNK;
                ++nv;
            }
        }
    }
    // ---- rank of this lane's tokens inside the chunk (every lane of the wave is here)
    const uint32_t x = mrg_wave_scan_incl(nv);
    const uint32_t excl = x - nv, total = (uint32_t)__shfl((int)x, 63);
    if (MODE == ENC_COUNT) {
        if (lane == 0) A.cnt[tile] = total;
        n_na += nonascii ? 1u : 0u;
    } else if (MODE == ENC_BOUND) {
        if (lane == 0) A.tok_off[item] = A.cnt[min(tile, A.ntiles)] + total;
    } else {
        const uint64_t base = A.cnt[tile] + excl;
        for (uint32_t i = 0; i < nv; ++i)
            if (base + i < A.out_n) A.out[base + i] = s_ids[wv][i * 64u + lane];
        n_tok += total;
    }
    mrg_wave_sync_lds();  // the next chunk reuses this wave's LDS
    }
    if (MODE == ENC_COUNT) {
        if (lane == 0 && n_na) atomicAdd(&A.info[3], (unsigned long long)n_na);
    } else if (MODE == ENC_EMIT) {
        const uint32_t unk = mrg_wave_sum(st.unk), lng = mrg_wave_sum(st.lng), pr = mrg_wave_sum(st.probes);
        if (lane == 0) {
            if (n_tok) atomicAdd(&A.info[0], (unsigned long long)n_tok);
            if (unk) atomicAdd(&A.info[1], (unsigned long long)unk);
            if (lng) atomicAdd(&A.info[2], (unsigned long long)lng);
            if (pr) atomicAdd(&A.info[4], (unsigned long long)pr);
        }
    }
}

// ---------------------------------------------------------------- vocabulary from text
// Line i = text[line_off[i], line_off[i + 1]), the last byte its '\n' (the host cut the lines there):
// valid UTF-8 (checked first, over the whole line: MRG_EUTF8 whatever else is wrong with it), then
// `word`, one ' ', 1 to 20 ASCII digits; the word non-empty, every codepoint \w.  One lane per line; the
// first bad line wins by atomicMin on line * 4 + reason.
__global__ __launch_bounds__(ENC_WG) void k_voc_check(VocTable T, uint32_t *wlen, unsigned long long *err) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i >= T.n) return;
    const uint64_t lo = T.line_off[i], hi = T.line_off[i + 1] - 1u;  // [lo, hi): the line without its '\n'
    const uint8_t *t = T.text;
    auto rd = [&](uint64_t x) -> uint32_t { return t[x]; };
    // one pass over the line: its UTF-8, the first space (hi: none) and whether every codepoint before it is \w
    uint32_t bad = 3u;
    uint64_t sp = hi;
    bool word = true;
    for (uint64_t p = lo; p < hi;) {
        uint32_t cp = 0, raw;
        const int l = mrg_utf8_decode(rd, p, hi, &cp, &raw);
        if (!l) {
            bad = MRG_VOC_BAD_UTF8;
            break;
        }
        if (sp == hi) {
            if (cp == 0x20u) sp = p;
            else if (mrg_uclass(cp) != MRG_CLS_W) word = false;
        }
        p += (uint64_t)l;
    }
    if (bad == 3u) {
        const uint64_t nd = hi > sp ? hi - sp - 1u : 0u;  // bytes after the space
        bool form = sp > lo && sp < hi && nd >= 1u && nd <= 20u;
        for (uint64_t q = sp + 1u; form && q < hi; ++q) form = (uint32_t)t[q] - '0' < 10u;
        if (!form) bad = MRG_VOC_BAD_FORM;
        else if (!word) bad = MRG_VOC_BAD_CLASS;
    }
    wlen[i] = bad == 3u ? (uint32_t)(sp - lo) : 0u;
    if (bad != 3u) atomicMin(err, (unsigned long long)(i * 4u + bad));
}

// Word i looked up in the finished table must find id i: a word that stands on two lines finds the
// other line from at least one of them.  Long candidates are compared byte for byte.
__global__ __launch_bounds__(ENC_WG) void k_voc_verify(VocTable T, const uint32_t *wlen, unsigned long long *dup) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i >= T.n) return;
    const uint8_t *w = T.text + T.line_off[i];
    const uint32_t L = wlen[i];
    VocKey kb;
    for (uint32_t j = 0; j < L; ++j) kb.push(w[j]);
    uint32_t probes = 0, id;
    if (L <= 16u) {
        id = voc_find(T, kb.k0, kb.k1, false, [](uint32_t) { return true; }, probes);
    } else {
        auto same = [&](uint32_t cand) -> bool {
            if (wlen[cand] != L) return false;
            const uint8_t *x = T.text + T.line_off[cand];
            bool eq = true;
            for (uint32_t j = 0; j < L && eq; ++j) eq = x[j] == w[j];
            return eq;
        };
        id = voc_find(T, kb.long_a(T.hash_bits), kb.long_b(), true, same, probes);
    }
    if (id != (uint32_t)i) atomicMin(dup, (unsigned long long)i);
}

// bit p of the boundary bitmap for every document offset (the end of the input included)
__global__ __launch_bounds__(ENC_WG) void k_enc_bounds(const uint64_t *doc_off, uint32_t n_docs, uint32_t *bnd) {
    const uint64_t i = (uint64_t)blockIdx.x * ENC_WG + threadIdx.x;
    if (i <= (uint64_t)n_docs) {
        const uint64_t p = doc_off[i];
        atomicOr(&bnd[p >> 5], 1u << (uint32_t)(p & 31u));
    }
}

}  // namespace

void mrg_voc_launch_lines(const SortRec *top, uint64_t m, KeySet ks, uint64_t min_count, uint64_t *len64,
                          uint32_t *wlen, unsigned long long *nkeep, hipStream_t s) {
    hipLaunchKernelGGL(k_voc_lines, dim3(grid_for(m + 1, ENC_WG)), dim3(ENC_WG), 0, s, top, m, ks, min_count, len64, wlen, nkeep);
}
void mrg_voc_launch_build(const VocTable &t, const uint32_t *wlen, unsigned long long *fail, hipStream_t s) {
    hipLaunchKernelGGL(k_voc_clear, dim3(grid_for(t.cap, ENC_WG)), dim3(ENC_WG), 0, s, t);
    if (t.n) hipLaunchKernelGGL(k_voc_insert, dim3(grid_for(t.n, ENC_WG)), dim3(ENC_WG), 0, s, t, wlen, fail);
}

void mrg_voc_launch_words(const VocTable &t, const VocWords &w, hipStream_t s) {
    if (t.n) hipLaunchKernelGGL(k_voc_words, dim3(grid_for(t.n, ENC_WG)), dim3(ENC_WG), 0, s, t, w);
}
void mrg_voc_launch_check(const VocTable &t, uint32_t *wlen, unsigned long long *err, hipStream_t s) {
    if (t.n) hipLaunchKernelGGL(k_voc_check, dim3(grid_for(t.n, ENC_WG)), dim3(ENC_WG), 0, s, t, wlen, err);
}
void mrg_voc_launch_verify(const VocTable &t, const uint32_t *wlen, unsigned long long *dup, hipStream_t s) {
    if (t.n) hipLaunchKernelGGL(k_voc_verify, dim3(grid_for(t.n, ENC_WG)), dim3(ENC_WG), 0, s, t, wlen, dup);
}

uint64_t mrg_enc_bitmap_words(uint64_t ntiles) { return ntiles * 32u + 8u; }

static EncArgs enc_args(const EncPlan &P) {
    EncArgs A{};
    A.in = P.in;
    A.lo = P.lo;
    A.hi = P.hi;
    A.ntiles = P.ntiles;
    A.bnd = P.bnd;
    A.doc_off = P.doc_off;
    A.n_docs = P.n_docs;
    A.cnt = P.cnt;
    A.tok_off = P.tok_off;
    A.out = P.out;
    A.out_n = P.out_n;
    A.err = P.err;
    A.info = P.info;
    return A;
}
void mrg_enc_launch_bounds(const EncPlan &P, hipStream_t s) {
    hipLaunchKernelGGL(k_enc_bounds, dim3(grid_for((uint64_t)P.n_docs + 1, ENC_WG)), dim3(ENC_WG), 0, s, P.doc_off, P.n_docs,
                       P.bnd);
}
void mrg_enc_launch_count(const EncPlan &P, const VocTable &t, hipStream_t s) {
    hipLaunchKernelGGL(k_enc<ENC_COUNT>, dim3(chunk_grid(P.ntiles)), dim3(ENC_WG), 0, s, enc_args(P), t);
}
void mrg_enc_launch_offsets(const EncPlan &P, const VocTable &t, hipStream_t s) {
    hipLaunchKernelGGL(k_enc<ENC_BOUND>, dim3(grid_for((uint64_t)P.n_docs + 1, ENC_NW)), dim3(ENC_WG), 0, s, enc_args(P),
                       t);
}
void mrg_enc_launch_emit(const EncPlan &P, const VocTable &t, hipStream_t s) {
    hipLaunchKernelGGL(k_enc<ENC_EMIT>, dim3(chunk_grid(P.ntiles)), dim3(ENC_WG), 0, s, enc_args(P), t);
}
